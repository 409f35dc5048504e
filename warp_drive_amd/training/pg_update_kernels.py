"""Trainer's A2C / PPO update for the in-kernel policies as five launches (csrc/kernels/pg_update.hip, code object
wd_kernels_pg.hsaco; the returns entry is wd_kernels_update.hsaco's):

    HipPgValues_H<H>_O<O>     values [T, E] of the recorded rows
    HipDiscountedReturns      the existing entry on `values` (w = 1, v_col = 0): returns and advantages [T, E]
    HipPgGradients_H<H>_O<O>  forward, the objective's gradient, backward: one partial of the eight tensors per block
    HipPgReduce               partials -> flat gradient, per-tensor sums of squares, the four sums of the objective
    HipPgApply                clip, Adam, refill of the rollout's packed policy

`trainer.fused_update: "all"` selects it (opt-in; training/trainer.py).  `admitted_shape` says which policies it serves;
`PgUpdateKernels` holds the launch wrappers, their geometry fixed from E, T, H, O, A and the compute-unit count;
`FlatPolicy` makes the parameters of a FullyConnected views of one flat float32 buffer in the kernels' layout, so the
kernels update the module in place and the module remains the source of truth.

Layout (the order of the module's parameters): W0 [H][O], b0 [H], W1 [H][H], b1 [H], Wp [A][H], bp [A], Wv [1][H], bv [1].
Its first six tensors are pack_rollout_policy's layout."""
import logging

import numpy as np
import torch

HIDDEN = (32, 64)          # widths the code object has entries for
OBS_SIZES = (2, 4, 6)      # MountainCar, Cartpole, Acrobot
MAX_ACTIONS = 8
TILE = 128                 # rows per tile = threads per block of HipPgGradients (its __launch_bounds__)
LD = TILE + 4              # row stride of the arrays it stages in LDS
VALUES_MAX_THREADS = 256   # __launch_bounds__ of HipPgValues
RETURNS_THREADS = 256      # __launch_bounds__ of HipDiscountedReturns
REDUCE_THREADS = 1024      # block size HipPgReduce is written for
TENSORS = 8
REDUCE_BLOCKS = TENSORS + 1   # eight parameter tensors + the four sums
SUMS = 4                   # sum logp * adv, sum entropy, sum (v - ret)^2, sum adv
APPLY_THREADS = 256
LDS_LIMIT = 160 * 1024
RETURNS_ENTRY = "HipDiscountedReturns"
_NULL = np.uint64(0)


def net_floats(H, O, A):
    return H * O + H + H * H + H + A * H + A + H + 1


def packed_floats(H, O, A):
    """pack_rollout_policy's tensor: everything but the value head"""
    return net_floats(H, O, A) - H - 1


def _pad4(n):
    return (n + 3) & ~3


def tensor_slices(H, O, A):
    """(offset, shape) of the eight parameter tensors inside the flat buffer"""
    out, at = [], 0
    for shape in ((H, O), (H,), (H, H), (H,), (A, H), (A,), (1, H), (1,)):
        out.append((at, shape))
        at += int(np.prod(shape))
    assert at == net_floats(H, O, A)
    return out


def values_lds_bytes(H, O):
    """the network's copy in LDS: eight head rows and eight bias slots whatever A is (the value head then starts on a
    16-byte boundary)"""
    return 4 * _pad4(net_floats(H, O, MAX_ACTIONS))


def gradients_lds_bytes(H, O):
    return values_lds_bytes(H, O) + 4 * (2 * H * LD + O * LD + (MAX_ACTIONS + 1) * LD + SUMS * LD)


def kernel_names(H, O):
    """the five launches, in order"""
    return [f"HipPgValues_H{H}_O{O}", RETURNS_ENTRY, f"HipPgGradients_H{H}_O{O}", "HipPgReduce", "HipPgApply"]


def all_kernel_names():
    """every entry of wd_kernels_pg.hsaco"""
    return sorted({n for H in HIDDEN for O in OBS_SIZES for n in kernel_names(H, O)} - {RETURNS_ENTRY})


def _admitted_tail(fc_dims, obs_size, obs_sizes, obs_takes, dtype, normalize_return, normalize_advantage, neg_pos_env_ratio,
                   world_size, algorithm, one_launch_rollout):
    """the checks both admission functions end with, in their order; `obs_sizes` are the observation sizes of the caller's
    kernels and `obs_takes` its words for them"""
    dims = [int(d) for d in fc_dims]
    if len(dims) != 2:
        return False, f"{len(dims)} hidden layers: the update kernels take two"
    if dims[0] != dims[1]:
        return False, f"the hidden layers have unequal widths {dims}"
    if dims[0] not in HIDDEN:
        return False, f"hidden width {dims[0]}: the update kernels exist for {list(HIDDEN)}"
    if int(obs_size) not in obs_sizes:
        return False, f"observation size {obs_size}: {obs_takes}"
    if dtype != torch.float32:
        return False, f"{dtype}: the update kernels are float32"
    if normalize_return:
        return False, "normalize_return: the returns are normalised by the framework path only"
    if normalize_advantage:
        return False, "normalize_advantage: the advantages are normalised by the framework path only"
    if neg_pos_env_ratio > 0:
        return False, "neg_pos_env_ratio: the replicas are down-sampled by the framework path only"
    if world_size != 1:
        return False, f"{world_size} ranks: the update kernels run in a single process"
    if str(algorithm).upper() not in ("A2C", "PPO"):
        return False, f"algorithm {algorithm}: the update kernels form the A2C / PPO gradient"
    if not one_launch_rollout:   # (asked last: a shape the rollout kernels refuse is named by what is wrong with it)
        return False, "the rollout is per tick: the update kernels go with the one-launch rollout"
    return True, ""


def admitted_shape(one_launch_rollout, n_policies, n_agents, head_sizes, fc_dims, obs_size, dtype, normalize_return,
                   normalize_advantage, neg_pos_env_ratio, world_size, algorithm):
    """(True, "") when the update kernels serve this policy, else (False, why)"""
    if n_policies != 1:
        return False, f"{n_policies} policies: the update kernels train one"
    if n_agents != 1:
        return False, f"{n_agents} agents: the update kernels train one per replica"
    heads = [int(a) for a in head_sizes]
    if len(heads) != 1:
        return False, f"{len(heads)} action heads: the update kernels take one"
    if not 1 <= heads[0] <= MAX_ACTIONS:
        return False, f"{heads[0]} actions: the update kernels take 1 to {MAX_ACTIONS}"
    return _admitted_tail(fc_dims, obs_size, OBS_SIZES, f"the update kernels exist for {list(OBS_SIZES)}", dtype,
                          normalize_return, normalize_advantage, neg_pos_env_ratio, world_size, algorithm, one_launch_rollout)


def policy_parameters(model):
    """the eight parameters of a two-hidden-layer, one-head FullyConnected in the kernels' order"""
    layers = [model.fc["0"][0], model.fc["1"][0], model.policy_head[0], model.vf_head]
    return [p for layer in layers for p in (layer.weight, layer.bias)]


class FlatPolicy:
    """`flat` [P] float32; every parameter of the module becomes a view of it (same values), so a kernel that writes `flat`
    has updated the module, and `load_state_dict` / `copy_` on the module write `flat`."""

    def __init__(self, model):
        assert len(model.fc) == 2 and len(model.policy_head) == 1, "not a network of the update kernels"
        params = policy_parameters(model)
        H, O, A = int(params[0].shape[0]), int(params[0].shape[1]), int(params[4].shape[0])
        slices = tensor_slices(H, O, A)
        assert [tuple(p.shape) for p in params] == [s for _, s in slices], "not the layout of the update kernels"
        assert [id(p) for p in params] == [id(p) for p in model.parameters()], "not the order of the module's parameters"
        self.H, self.O, self.A = H, O, A
        self.flat = torch.empty(net_floats(H, O, A), dtype=torch.float32, device=params[0].device)
        with torch.no_grad():
            for p, (at, shape) in zip(params, slices):
                view = self.flat[at:at + p.numel()].view(shape)
                view.copy_(p.detach().float())
                p.data = view
        self.params = params

    def bound(self):
        """every parameter still is the view it was made (nobody has re-assigned `.data`)"""
        return all(p.data_ptr() == self.flat.data_ptr() + 4 * at
                   for p, (at, _) in zip(self.params, tensor_slices(self.H, self.O, self.A)))


class _PgUpdateLaunches:
    """What PgUpdateKernels and PgGridworldUpdateKernels share: the geometry rules, the buffers the launches hand to each
    other and the five wrappers, written on rows = T * E * n recorded rows (n agents of the policy per replica), the P
    floats of the network, the floats of the rollout's packed policy and the Apply grid.  A class supplies its entry names,
    n, the two LDS sizes, the packed size and `_shape_args`.  Blocks and grids: the gradient kernel's block is its tile
    (TILE threads) and its grid one block per tile up to one per compute unit (the rest are grid-stride trips); the value
    kernel takes the largest block of 64 / 128 / 256 threads that still gives every compute unit one; Apply has one thread
    per float of the larger of the network and the packed policy."""

    def _setup(self, function_manager, names, batch_shape, H, O, A, values_lds, gradients_lds, packed_floats, device,
               compute_units):
        self.T, self.E = int(batch_shape[0]), int(batch_shape[1])
        self.n = int(batch_shape[2]) if len(batch_shape) == 3 else 1
        assert self.E >= 1 and self.T >= 1 and self.n >= 1, batch_shape
        self.H, self.O, self.A = int(H), int(O), int(A)
        self.device = torch.device(device)
        if compute_units is None:
            compute_units = torch.cuda.get_device_properties(self.device).multi_processor_count
        self.compute_units = int(compute_units)
        self.P = net_floats(H, O, A)
        self.packed_floats = int(packed_floats)
        self.names = names
        function_manager.initialize_functions(self.names)
        (self.fn_values, self.fn_returns, self.fn_gradients, self.fn_reduce,
         self.fn_apply) = (function_manager.get_function(n) for n in self.names)
        # ---- geometry
        self.rows = self.T * self.E * self.n
        block = VALUES_MAX_THREADS
        while block > 64 and -(-self.rows // block) < self.compute_units:
            block //= 2
        self.values_block = block
        self.values_grid = max(1, min(-(-self.rows // block), 8 * self.compute_units))
        self.values_lds = values_lds
        self.returns_grid = -(-(self.E * self.n) // RETURNS_THREADS)
        self.tiles = -(-self.rows // TILE)
        self.gradients_grid = max(1, min(self.tiles, self.compute_units))
        self.gradients_lds = gradients_lds
        self.apply_grid = -(-max(self.P, self.packed_floats) // APPLY_THREADS)
        assert max(self.values_lds, self.gradients_lds) <= LDS_LIMIT
        # ---- what the launches hand to each other
        f32 = dict(dtype=torch.float32, device=self.device)
        self.values = torch.zeros(batch_shape, **f32)
        self.returns = torch.zeros(batch_shape, **f32)
        self.advantages = torch.zeros(batch_shape, **f32)
        self.partials = torch.zeros((self.gradients_grid, self.P + SUMS), **f32)
        self.grads = torch.zeros(self.P, **f32)
        self.sumsq = torch.zeros(TENSORS, **f32)
        self.sums = torch.zeros(SUMS, **f32)

    # ------------------------------------------------------------------------------------------------ the launches
    def _check_batch(self, t, tail, dtype=torch.float32, rows=None):
        rows = self.rows if rows is None else rows
        assert t.dtype == dtype and t.is_contiguous() and t.numel() == rows * tail, (tuple(t.shape), rows, tail)

    def _check_flat(self, *tensors, numel=None):
        for t in tensors:
            assert t.numel() == (self.P if numel is None else numel) and t.dtype == torch.float32 and t.is_contiguous()

    def _shape_args(self, per_row):
        """the shape arguments of an entry: `per_row` for Values and Gradients, else Reduce and Apply"""
        raise NotImplementedError

    def compute_values(self, obs, theta, out=None, block=None, grid=None):
        """values [T, E(, n)] = v(obs); obs [T, E, n, O]"""
        out = self.values if out is None else out
        self._check_batch(obs, self.O)
        assert obs.shape[-1] == self.O, tuple(obs.shape)
        self._check_flat(theta)
        self._check_flat(out, numel=self.rows)
        block = self.values_block if block is None else int(block)
        assert block % 64 == 0 and 64 <= block <= VALUES_MAX_THREADS
        self.fn_values(obs, theta, np.int64(self.rows), *self._shape_args(True), out, block=(block, 1, 1),
                       grid=(self.values_grid if grid is None else int(grid), 1), shared=self.values_lds)
        return out

    def discounted_returns(self, rewards, done, gamma, values=None, returns=None, advantages=None):
        """(returns, returns - values) [T, E(, n)] from the existing HipDiscountedReturns: n agents, an output row of width 1
        whose column 0 is the value; done [T, E] is the replica's"""
        values = self.values if values is None else values
        returns = self.returns if returns is None else returns
        advantages = self.advantages if advantages is None else advantages
        self._check_batch(rewards, 1)
        self._check_batch(done, 1, torch.int32, rows=self.T * self.E)
        self._check_flat(values, returns, advantages, numel=self.rows)
        self.fn_returns(rewards, done, values, np.int32(1), np.int32(0), np.float32(gamma), np.int32(self.T), np.int32(self.E),
                        np.int32(self.n), returns, advantages, block=(RETURNS_THREADS, 1, 1), grid=(self.returns_grid, 1),
                        shared=0)
        return returns, advantages

    def gradients(self, obs, actions, theta, ent_coeff, vf_coeff, advantages=None, returns=None, partials=None):
        """per-block partials [blocks, P + 4]: the gradient of
        mean(-logp(a) adv) + vf_coeff mean((v - ret)^2) - ent_coeff mean(entropy) over the rows, then the block's four
        sums; the grid is the number of rows of `partials`"""
        advantages = self.advantages if advantages is None else advantages
        returns = self.returns if returns is None else returns
        partials = self.partials if partials is None else partials
        self._check_batch(obs, self.O)
        assert obs.shape[-1] == self.O, tuple(obs.shape)
        self._check_batch(actions, 1, torch.int32)
        self._check_flat(advantages, returns, numel=self.rows)
        self._check_flat(theta)
        assert partials.dim() == 2 and partials.shape[1] == self.P + SUMS and partials.is_contiguous()
        assert partials.dtype == torch.float32
        self.fn_gradients(obs, actions, advantages, returns, theta, np.int64(self.rows), *self._shape_args(True),
                          np.float32(1.0 / self.rows), np.float32(ent_coeff), np.float32(vf_coeff), partials,
                          block=(TILE, 1, 1), grid=(int(partials.shape[0]), 1), shared=self.gradients_lds)
        return partials

    def reduce(self, partials=None, grads=None, sumsq=None, sums=None):
        """flat gradient [P], sums of squares per tensor [8], the four sums"""
        partials = self.partials if partials is None else partials
        grads, sumsq, sums = (self.grads if grads is None else grads, self.sumsq if sumsq is None else sumsq,
                              self.sums if sums is None else sums)
        assert partials.shape[1] == self.P + SUMS and partials.is_contiguous() and partials.dtype == torch.float32
        assert grads.numel() == self.P and sumsq.numel() == TENSORS and sums.numel() == SUMS
        self.fn_reduce(partials, np.int32(partials.shape[0]), *self._shape_args(False), grads, sumsq, sums,
                       block=(REDUCE_THREADS, 1, 1), grid=(REDUCE_BLOCKS, 1), shared=0)
        return grads, sumsq, sums

    def apply(self, theta, exp_avg, exp_avg_sq, step, lr, max_norm=None, packed=None, grads=None, sumsq=None,
              betas=(0.9, 0.999), eps=1e-8):
        """clip (max_norm None or <= 0: off), Adam step number `step` (1 for the first), and the rollout's packed policy.
        step_size = lr / (1 - beta1^step) and sqrt(1 - beta2^step) are Python floats, as in torch.optim.Adam."""
        grads, sumsq = self.grads if grads is None else grads, self.sumsq if sumsq is None else sumsq
        self._check_flat(theta, exp_avg, exp_avg_sq, grads)
        assert step >= 1 and sumsq.numel() == TENSORS
        if packed is not None:
            self._check_flat(packed, numel=self.packed_floats)
        beta1, beta2 = betas
        bc1, bc2 = 1 - beta1 ** float(step), 1 - beta2 ** float(step)
        self.fn_apply(theta, exp_avg, exp_avg_sq, grads, sumsq, _NULL if packed is None else packed, *self._shape_args(False),
                      np.float32(max_norm if max_norm else 0.0), np.float32(lr / bc1), np.float32(bc2 ** 0.5),
                      np.float32(1 - beta1), np.float32(beta2), np.float32(1 - beta2), np.float32(eps),
                      block=(APPLY_THREADS, 1, 1), grid=(self.apply_grid, 1), shared=0)

    # ------------------------------------------------------------------------------------------------ reading back
    def gradient_norm(self, sumsq=None):
        """the 2-norm of the whole gradient before clipping, from the reduce launch (reads the device)"""
        return float(torch.sqrt((self.sumsq if sumsq is None else sumsq).double().sum()))

    def metrics(self, rewards, actions, ent_coeff, vf_coeff, ppo):
        """the metric dict of losses.A2C.compute_loss_and_metrics_from_logits from what the launches left behind: values,
        returns, advantages and the four sums (reads the device; call after `reduce`); rewards [T, E, n], actions
        [T, E, n, 1]"""
        R = float(self.rows)
        s_pg, s_ent, s_vf, s_adv = (float(v) for v in self.sums.double().tolist())
        policy_loss = -(s_adv if ppo else s_pg) / R   # PPO at ratio 1: min(ratio * A, clamp(ratio) * A) = A
        vf_loss, entropy = s_vf / R, s_ent / R
        adv, ret = self.advantages.reshape(self.T, self.E, self.n), self.returns.reshape(self.T, self.E, self.n)
        var_explained = torch.clamp(1 - adv.var() / (ret.var() + 1.0e-10), min=-1.0)
        m = {
            "VF loss coefficient": vf_coeff, "Entropy coefficient": ent_coeff,
            "Total loss": float(np.float32(policy_loss + vf_coeff * vf_loss - ent_coeff * entropy)),
            "Policy loss": policy_loss, "Value function loss": vf_loss,
            "Mean rewards": rewards.mean().item(), "Max. rewards": rewards.max().item(),
            "Min. rewards": rewards.min().item(), "Mean value function": self.values.mean().item(),
            "Mean advantages": adv.mean().item(), "Mean (norm.) advantages": adv.mean().item(),
            "Mean (discounted) returns": ret.mean().item(), "Mean normalized returns": ret.mean().item(),
            "Mean entropy": entropy, "Variance explained by the value function": var_explained.item(),
        }
        af = actions.reshape(self.T, self.E, self.n, -1).float()
        over_agents, over_time, over_envs = (af.std(dim=d).mean(dim=(0, 1)) for d in (2, 0, 1))
        for h in range(af.shape[-1]):
            m[f"Std. of action_{h} over agents"] = over_agents[h].item()
            m[f"Std. of action_{h} over envs"] = over_envs[h].item()
            m[f"Std. of action_{h} over time"] = over_time[h].item()
        return m


class PgUpdateKernels(_PgUpdateLaunches):
    """The five launches for one (E, T, H, O, A): one agent per replica, every entry takes (H, O, A)."""

    def __init__(self, function_manager, E, T, H, O, A, device, compute_units=None):
        assert H in HIDDEN and O in OBS_SIZES and 1 <= A <= MAX_ACTIONS, (H, O, A)
        self._setup(function_manager, kernel_names(H, O), (T, E), H, O, A, values_lds_bytes(H, O), gradients_lds_bytes(H, O),
                    packed_floats(H, O, A), device, compute_units)

    def _shape_args(self, per_row):
        return np.int32(self.H), np.int32(self.O), np.int32(self.A)


def log_refusal(policy, reason):
    logging.info(f"trainer.fused_update \"all\", policy '{policy}': {reason}; its update runs on the framework path")
