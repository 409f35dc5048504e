"""training/pg_update_kernels.py's five launches for the policies of the one-launch TagGridWorld rollout
(csrc/kernels/pg_update_gridworld.hip, code object wd_kernels_pg_gw.hsaco; the returns entry is wd_kernels_update.hsaco's):

    HipPgGwValues_H<H>      values [T, E, n] of the recorded rows of ONE policy (n agents per replica)
    HipDiscountedReturns    the existing entry on `values` (n agents, w = 1, v_col = 0): returns and advantages [T, E, n]
    HipPgGwGradients_H<H>   forward, the objective's gradient, backward: one partial of the eight tensors per block
    HipPgGwReduce           partials -> flat gradient, per-tensor sums of squares, the four sums of the objective
    HipPgGwApply            clip, Adam, refill of the rollout's packed policy in pack_gridworld_policy's layout

A row is (t, replica, agent of the policy): rows = T * E * n, and the objective's means are over all of them.  The network
is the module's -- W0 [H][21], b0, W1 [H][H], b1, Wp [5][H], bp, Wv [1][H], bv, float32 -- flat in that order (`FlatPolicy`
of training/pg_update_kernels.py, as it is); the packed policy is NOT a prefix of it (W0's rows are 24 floats apart there)
and the Apply launch writes every float of it.  `admitted_gridworld_shape` says which policies this serves."""
import numpy as np
import torch

from warp_drive_amd.training.pg_update_kernels import (APPLY_THREADS, LD, LDS_LIMIT, REDUCE_BLOCKS, REDUCE_THREADS,
                                                       RETURNS_ENTRY, RETURNS_THREADS, SUMS, TENSORS, TILE,
                                                       VALUES_MAX_THREADS, _NULL, _pad4, net_floats)

HIDDEN = (32, 64)          # widths the code object has entries for
OBS = 21                   # observation floats of a TagGridWorld row at 5 agents (full observations)
ACTIONS = 5
IN_STRIDE = 24             # floats per row of W0 in LDS and in the packed policy (tag_gridworld_n5_common.h: GW5_IN_STRIDE)
BIAS_SLOTS = 8             # the value head's LDS copy starts behind eight bias slots: a 16-byte boundary
CODE_OBJECT = "wd_kernels_pg_gw.hsaco"


def gw_net_floats(H):
    return net_floats(H, OBS, ACTIONS)


def packed_body_floats(H):
    """pack_gridworld_policy's tensors: W0 [H][24], b0, W1, b1, Wp, bp"""
    return H * IN_STRIDE + H + H * H + H + ACTIONS * H + ACTIONS


def packed_floats(H):
    """... rounded up to whole 16-byte vectors (envs/tag_gridworld.py::gridworld_policy_floats)"""
    return _pad4(packed_body_floats(H))


def values_lds_bytes(H):
    return 4 * _pad4(packed_body_floats(H) - ACTIONS + BIAS_SLOTS + H + 1)


def gradients_lds_bytes(H):
    return values_lds_bytes(H) + 4 * LD * (2 * H + OBS + (ACTIONS + 1) + SUMS)


def kernel_names(H):
    """the five launches, in order"""
    return [f"HipPgGwValues_H{H}", RETURNS_ENTRY, f"HipPgGwGradients_H{H}", "HipPgGwReduce", "HipPgGwApply"]


def all_kernel_names():
    """every entry of wd_kernels_pg_gw.hsaco"""
    return sorted({n for H in HIDDEN for n in kernel_names(H)} - {RETURNS_ENTRY})


def pack_from_flat(theta, H):
    """pack_gridworld_policy's block formed from a flat theta (a numpy float32 array of gw_net_floats(H)): what the Apply
    launch leaves in the packed tensor"""
    theta = np.asarray(theta, np.float32)
    assert theta.shape == (gw_net_floats(H),)
    out = np.zeros(packed_floats(H), np.float32)
    out[:H * IN_STRIDE].reshape(H, IN_STRIDE)[:, :OBS] = theta[:H * OBS].reshape(H, OBS)
    rest = theta[H * OBS:gw_net_floats(H) - H - 1]
    out[H * IN_STRIDE:H * IN_STRIDE + rest.size] = rest
    return out


def admitted_gridworld_shape(one_launch_rollout, gridworld_packing, n_policies, n_agents, head_sizes, fc_dims, obs_size,
                             dtype, normalize_return, normalize_advantage, neg_pos_env_ratio, world_size, algorithm):
    """(True, "") when these update kernels serve this policy, else (False, why).  Any number of policies, n >= 1 agents
    per policy."""
    if n_policies < 1:
        return False, f"{n_policies} policies"
    if n_agents < 1:
        return False, f"{n_agents} agents: the update kernels train at least one per replica"
    heads = [int(a) for a in head_sizes]
    if len(heads) != 1:
        return False, f"{len(heads)} action heads: the update kernels take one"
    if heads[0] != ACTIONS:
        return False, f"{heads[0]} actions: the gridworld update kernels take {ACTIONS}"
    dims = [int(d) for d in fc_dims]
    if len(dims) != 2:
        return False, f"{len(dims)} hidden layers: the update kernels take two"
    if dims[0] != dims[1]:
        return False, f"the hidden layers have unequal widths {dims}"
    if dims[0] not in HIDDEN:
        return False, f"hidden width {dims[0]}: the update kernels exist for {list(HIDDEN)}"
    if int(obs_size) != OBS:
        return False, f"observation size {obs_size}: the gridworld update kernels take {OBS}"
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
    if not gridworld_packing:
        return False, "the rollout's packed policy is not pack_gridworld_policy's layout"
    return True, ""


class PgGridworldUpdateKernels:
    """The five launches for one policy of (E, T, n, H): PgUpdateKernels' methods and geometry rules on rows = T * E * n."""

    def __init__(self, function_manager, E, T, n, H, device, compute_units=None):
        assert H in HIDDEN, H
        assert E >= 1 and T >= 1 and n >= 1, (E, T, n)
        self.E, self.T, self.n, self.H, self.O, self.A = int(E), int(T), int(n), int(H), OBS, ACTIONS
        self.device = torch.device(device)
        if compute_units is None:
            compute_units = torch.cuda.get_device_properties(self.device).multi_processor_count
        self.compute_units = int(compute_units)
        self.P = gw_net_floats(H)
        self.packed_floats = packed_floats(H)
        self.names = kernel_names(H)
        function_manager.initialize_functions(self.names)
        (self.fn_values, self.fn_returns, self.fn_gradients, self.fn_reduce,
         self.fn_apply) = (function_manager.get_function(name) for name in self.names)
        # ---- geometry
        self.rows = self.T * self.E * self.n
        block = VALUES_MAX_THREADS
        while block > 64 and -(-self.rows // block) < self.compute_units:
            block //= 2
        self.values_block = block
        self.values_grid = max(1, min(-(-self.rows // block), 8 * self.compute_units))
        self.values_lds = values_lds_bytes(H)
        self.returns_grid = -(-(self.E * self.n) // RETURNS_THREADS)
        self.tiles = -(-self.rows // TILE)
        self.gradients_grid = max(1, min(self.tiles, self.compute_units))
        self.gradients_lds = gradients_lds_bytes(H)
        self.apply_grid = -(-max(self.P, self.packed_floats) // APPLY_THREADS)   # one thread per float of the larger
        assert max(self.values_lds, self.gradients_lds) <= LDS_LIMIT
        # ---- what the launches hand to each other
        f32 = dict(dtype=torch.float32, device=self.device)
        self.values = torch.zeros((self.T, self.E, self.n), **f32)
        self.returns = torch.zeros((self.T, self.E, self.n), **f32)
        self.advantages = torch.zeros((self.T, self.E, self.n), **f32)
        self.partials = torch.zeros((self.gradients_grid, self.P + SUMS), **f32)
        self.grads = torch.zeros(self.P, **f32)
        self.sumsq = torch.zeros(TENSORS, **f32)
        self.sums = torch.zeros(SUMS, **f32)

    # ------------------------------------------------------------------------------------------------ the launches
    def _check_batch(self, t, tail, dtype=torch.float32, rows=None):
        rows = self.rows if rows is None else rows
        assert t.dtype == dtype and t.is_contiguous() and t.numel() == rows * tail, (tuple(t.shape), rows, tail)

    def compute_values(self, obs, theta, out=None, block=None, grid=None):
        """values [T, E, n] = v(obs); obs [T, E, n, 21]"""
        out = self.values if out is None else out
        self._check_batch(obs, OBS)
        assert obs.shape[-1] == OBS, tuple(obs.shape)
        assert theta.numel() == self.P and theta.dtype == torch.float32 and theta.is_contiguous()
        assert out.numel() == self.rows and out.dtype == torch.float32 and out.is_contiguous()
        block = self.values_block if block is None else int(block)
        assert block % 64 == 0 and 64 <= block <= VALUES_MAX_THREADS
        self.fn_values(obs, theta, np.int64(self.rows), out, block=(block, 1, 1),
                       grid=(self.values_grid if grid is None else int(grid), 1), shared=self.values_lds)
        return out

    def discounted_returns(self, rewards, done, gamma, values=None, returns=None, advantages=None):
        """(returns, returns - values) [T, E, n] from the existing HipDiscountedReturns: n agents, an output row of width 1
        whose column 0 is the value; done [T, E] is the replica's"""
        values = self.values if values is None else values
        returns = self.returns if returns is None else returns
        advantages = self.advantages if advantages is None else advantages
        self._check_batch(rewards, 1)
        self._check_batch(done, 1, torch.int32, rows=self.T * self.E)
        for t in (values, returns, advantages):
            assert t.numel() == self.rows and t.dtype == torch.float32 and t.is_contiguous()
        self.fn_returns(rewards, done, values, np.int32(1), np.int32(0), np.float32(gamma), np.int32(self.T), np.int32(self.E),
                        np.int32(self.n), returns, advantages, block=(RETURNS_THREADS, 1, 1), grid=(self.returns_grid, 1),
                        shared=0)
        return returns, advantages

    def gradients(self, obs, actions, theta, ent_coeff, vf_coeff, advantages=None, returns=None, partials=None):
        """per-block partials [blocks, P + 4]: the gradient of
        mean(-logp(a) adv) + vf_coeff mean((v - ret)^2) - ent_coeff mean(entropy) over the T * E * n rows, then the block's
        four sums; the grid is the number of rows of `partials`"""
        advantages = self.advantages if advantages is None else advantages
        returns = self.returns if returns is None else returns
        partials = self.partials if partials is None else partials
        self._check_batch(obs, OBS)
        assert obs.shape[-1] == OBS, tuple(obs.shape)
        self._check_batch(actions, 1, torch.int32)
        assert advantages.numel() == returns.numel() == self.rows and theta.numel() == self.P
        assert advantages.dtype == returns.dtype == theta.dtype == torch.float32
        assert advantages.is_contiguous() and returns.is_contiguous() and theta.is_contiguous()
        assert partials.dim() == 2 and partials.shape[1] == self.P + SUMS and partials.is_contiguous()
        assert partials.dtype == torch.float32
        self.fn_gradients(obs, actions, advantages, returns, theta, np.int64(self.rows), np.float32(1.0 / self.rows),
                          np.float32(ent_coeff), np.float32(vf_coeff), partials, block=(TILE, 1, 1),
                          grid=(int(partials.shape[0]), 1), shared=self.gradients_lds)
        return partials

    def reduce(self, partials=None, grads=None, sumsq=None, sums=None):
        """flat gradient [P], sums of squares per tensor [8], the four sums"""
        partials = self.partials if partials is None else partials
        grads, sumsq, sums = (self.grads if grads is None else grads, self.sumsq if sumsq is None else sumsq,
                              self.sums if sums is None else sums)
        assert partials.shape[1] == self.P + SUMS and partials.is_contiguous() and partials.dtype == torch.float32
        assert grads.numel() == self.P and sumsq.numel() == TENSORS and sums.numel() == SUMS
        self.fn_reduce(partials, np.int32(partials.shape[0]), np.int32(self.H), grads, sumsq, sums,
                       block=(REDUCE_THREADS, 1, 1), grid=(REDUCE_BLOCKS, 1), shared=0)
        return grads, sumsq, sums

    def apply(self, theta, exp_avg, exp_avg_sq, step, lr, max_norm=None, packed=None, grads=None, sumsq=None,
              betas=(0.9, 0.999), eps=1e-8):
        """clip (max_norm None or <= 0: off), Adam step number `step` (1 for the first), and every float of the packed
        policy (pack_gridworld_policy's layout).  step_size = lr / (1 - beta1^step) and sqrt(1 - beta2^step) are Python
        floats, as in torch.optim.Adam."""
        grads, sumsq = self.grads if grads is None else grads, self.sumsq if sumsq is None else sumsq
        for t in (theta, exp_avg, exp_avg_sq, grads):
            assert t.numel() == self.P and t.dtype == torch.float32 and t.is_contiguous()
        assert step >= 1 and sumsq.numel() == TENSORS
        if packed is not None:
            assert packed.numel() == self.packed_floats and packed.dtype == torch.float32 and packed.is_contiguous()
        beta1, beta2 = betas
        bc1, bc2 = 1 - beta1 ** float(step), 1 - beta2 ** float(step)
        self.fn_apply(theta, exp_avg, exp_avg_sq, grads, sumsq, _NULL if packed is None else packed, np.int32(self.H),
                      np.float32(max_norm if max_norm else 0.0), np.float32(lr / bc1), np.float32(bc2 ** 0.5),
                      np.float32(1 - beta1), np.float32(beta2), np.float32(1 - beta2), np.float32(eps),
                      block=(APPLY_THREADS, 1, 1), grid=(self.apply_grid, 1), shared=0)

    # ------------------------------------------------------------------------------------------------ reading back
    def gradient_norm(self, sumsq=None):
        """the 2-norm of the whole gradient before clipping, from the reduce launch (reads the device)"""
        return float(torch.sqrt((self.sumsq if sumsq is None else sumsq).double().sum()))

    def metrics(self, rewards, actions, ent_coeff, vf_coeff, ppo):
        """the metric dict of losses.A2C.compute_loss_and_metrics_from_logits from what the launches left behind (reads
        the device; call after `reduce`); rewards [T, E, n], actions [T, E, n, 1]"""
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

