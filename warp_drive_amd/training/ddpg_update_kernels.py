"""TrainerDDPG's update as four launches (csrc/kernels/ddpg_update.hip, code object wd_kernels_ddpg.hsaco):

    HipDdpgTargets_H<H>_O<O>    next values of the T - 1 rows that have a next row, from the two target networks
    HipDdpgGradients_H<H>_O<O>  n-step returns, then the critic's and the actor's gradient as one partial per block
    HipDdpgReduce               partials -> flat gradients, per-tensor sums of squares, the two losses
    HipDdpgApply                clip, Adam, soft update of the targets, refill of the rollout's packed actor

`trainer.fused_update: true` selects it (opt-in; training/trainer_ddpg.py).  `admitted_shape` says which trainers it
serves; `DdpgUpdateKernels` holds the launch wrappers, their geometry fixed from E, T, n_step and H; `FlatNetworks` makes
the parameters of the actor and the critic (and of their targets) views of one flat float32 buffer each, in the kernels'
layout, so the kernels update the modules in place and the modules remain the source of truth.

Layout of one network (two hidden layers of H units on I inputs, one output), the order of its parameters:
W0 [H][I], b0 [H], W1 [H][H], b1 [H], Wo [H], bo [1]; a flat buffer holds the actor (I = O), then the critic (I = O + 1)."""
import logging

import numpy as np
import torch

HIDDEN = (32, 64)          # widths the code object has entries for
OBS_SIZES = (2, 3)
TILE = 128                 # rows per tile = threads per block of HipDdpgGradients (its __launch_bounds__)
LD = TILE + 4              # row stride of the arrays it stages in LDS
TARGETS_MAX_THREADS = 256  # __launch_bounds__ of HipDdpgTargets
REDUCE_THREADS = 1024      # block size HipDdpgReduce is written for
REDUCE_BLOCKS = 13         # twelve parameter tensors + the losses
APPLY_THREADS = 256
LDS_LIMIT = 160 * 1024
TENSORS_PER_NETWORK = 6
_NULL = np.uint64(0)


def net_floats(H, I):
    return H * I + H + H * H + H + H + 1


def _pad4(n):
    return (n + 3) & ~3


def total_floats(H, O):
    """floats of (actor, critic)"""
    return net_floats(H, O) + net_floats(H, O + 1)


def tensor_slices(H, O):
    """(offset, shape) of the twelve parameter tensors inside the flat buffer, actor first"""
    out, at = [], 0
    for I in (O, O + 1):
        for shape in ((H, I), (H,), (H, H), (H,), (1, H), (1,)):
            out.append((at, shape))
            at += int(np.prod(shape))
    assert at == total_floats(H, O)
    return out


def targets_lds_bytes(H, O):
    return 4 * (_pad4(net_floats(H, O)) + _pad4(net_floats(H, O + 1)))


def gradients_lds_bytes(H, O):
    return targets_lds_bytes(H, O) + 4 * (2 * H * LD + 4 * LD + 2 * TILE)


def kernel_names(H, O):
    return [f"HipDdpgTargets_H{H}_O{O}", f"HipDdpgGradients_H{H}_O{O}", "HipDdpgReduce", "HipDdpgApply"]


def all_kernel_names():
    return sorted({n for H in HIDDEN for O in OBS_SIZES for n in kernel_names(H, O)})


def admitted_shape(n_policies, n_agents, obs_size, action_dims, actor_fc_dims, critic_fc_dims, normalize_return):
    """(True, "") when the update kernels serve this trainer, else (False, why).  `normalize_advantage` touches a logged
    metric only and is not asked about."""
    if n_policies != 1:
        return False, f"{n_policies} policies: the update kernels train one"
    if n_agents != 1:
        return False, f"{n_agents} agents: the update kernels train one"
    if action_dims != 1:
        return False, f"{action_dims} action dimensions: the update kernels take one"
    actor, critic = [int(d) for d in actor_fc_dims], [int(d) for d in critic_fc_dims]
    for name, dims in (("actor", actor), ("critic", critic)):
        if len(dims) != 2:
            return False, f"the {name} has {len(dims)} hidden layers: the update kernels take two"
        if dims[0] != dims[1]:
            return False, f"the {name}'s hidden layers have unequal widths {dims}"
    if actor != critic:
        return False, f"the actor's width {actor[0]} is not the critic's {critic[0]}"
    if actor[0] not in HIDDEN:
        return False, f"hidden width {actor[0]}: the update kernels exist for {list(HIDDEN)}"
    if int(obs_size) not in OBS_SIZES:
        return False, f"observation size {obs_size}: the update kernels exist for {list(OBS_SIZES)}"
    if normalize_return:
        return False, "normalize_return: the returns are normalised by the framework path only"
    return True, ""


def _layers(net):
    return [net.fc["0"][0], net.fc["1"][0], net.action_head if hasattr(net, "action_head") else net.q_head]


class FlatNetworks:
    """`flat` [PA + PC] float32 holding (actor, critic); every parameter of the two modules becomes a view of it (same
    values), so a kernel that writes `flat` has updated the modules, and `load_state_dict` / `copy_` on the modules write
    `flat`."""

    def __init__(self, actor, critic):
        params = [p for net in (actor, critic) for layer in _layers(net) for p in (layer.weight, layer.bias)]
        H, O = int(params[0].shape[0]), int(params[0].shape[1])
        slices = tensor_slices(H, O)
        assert [tuple(p.shape) for p in params] == [s for _, s in slices], "not the layout of the update kernels"
        self.H, self.O = H, O
        self.flat = torch.empty(total_floats(H, O), dtype=torch.float32, device=params[0].device)
        with torch.no_grad():
            for p, (at, shape) in zip(params, slices):
                view = self.flat[at:at + p.numel()].view(shape)
                view.copy_(p.detach().float())
                p.data = view
        self.params = params

    def bound(self):
        """every parameter still is the view it was made (nobody has re-assigned `.data`)"""
        return all(p.data_ptr() == self.flat.data_ptr() + 4 * at for p, (at, _) in zip(self.params, tensor_slices(self.H, self.O)))


class DdpgUpdateKernels:
    """The four launches for one (E, T, n_step, H, O).  Blocks and grids are fixed here: the gradient kernel's block is its
    tile (TILE threads) and its grid one block per tile up to one per compute unit (the rest are grid-stride trips); the
    next-value kernel takes the largest block of 64 / 128 / 256 threads that still gives every compute unit one."""

    def __init__(self, function_manager, E, T, n_step, H, O, device, compute_units=None):
        assert H in HIDDEN and O in OBS_SIZES, (H, O)
        assert n_step >= 1 and T >= max(n_step, 2), (T, n_step)
        self.E, self.T, self.n_step, self.H, self.O = int(E), int(T), int(n_step), int(H), int(O)
        self.V = self.T - self.n_step + 1
        self.device = torch.device(device)
        if compute_units is None:
            compute_units = torch.cuda.get_device_properties(self.device).multi_processor_count
        self.compute_units = int(compute_units)
        self.PT = total_floats(H, O)
        self.PA = net_floats(H, O)
        self.names = kernel_names(H, O)
        function_manager.initialize_functions(self.names)
        self.fn_targets, self.fn_gradients, self.fn_reduce, self.fn_apply = (function_manager.get_function(n) for n in self.names)
        # ---- geometry
        rows1 = (self.T - 1) * self.E
        block = TARGETS_MAX_THREADS
        while block > 64 and -(-rows1 // block) < self.compute_units:
            block //= 2
        self.targets_block = block
        self.targets_grid = max(1, min(-(-rows1 // block), 8 * self.compute_units))
        self.targets_lds = targets_lds_bytes(H, O)
        self.rows = self.V * self.E
        self.tiles = -(-self.rows // TILE)
        self.gradients_grid = max(1, min(self.tiles, self.compute_units))
        self.gradients_lds = gradients_lds_bytes(H, O)
        self.apply_grid = -(-self.PT // APPLY_THREADS)
        assert max(self.targets_lds, self.gradients_lds) <= LDS_LIMIT
        # ---- what the launches hand to each other
        f32 = dict(dtype=torch.float32, device=self.device)
        self.next_values = torch.zeros((self.T - 1, self.E), **f32)
        self.returns = torch.zeros((self.V, self.E), **f32)
        self.partials = torch.zeros((self.gradients_grid, self.PT + 2), **f32)
        self.grads = torch.zeros(self.PT, **f32)
        self.sumsq = torch.zeros(2 * TENSORS_PER_NETWORK, **f32)
        self.losses = torch.zeros(2, **f32)

    # ------------------------------------------------------------------------------------------------ the launches
    def _check_batch(self, t, rows, tail, dtype=torch.float32):
        assert t.dtype == dtype and t.is_contiguous() and t.numel() == rows * self.E * tail, (tuple(t.shape), rows, tail)

    def targets(self, obs, target_flat, action_scale, action_bias, out=None, block=None, grid=None):
        """next_values [T - 1, E] = Q'(obs[t + 1], mu'(obs[t + 1])); obs [T, E, (1,) O]"""
        out = self.next_values if out is None else out
        self._check_batch(obs, self.T, self.O)
        assert target_flat.numel() == self.PT and out.numel() == (self.T - 1) * self.E
        block = self.targets_block if block is None else int(block)
        assert block % 64 == 0 and 64 <= block <= TARGETS_MAX_THREADS
        self.fn_targets(obs, target_flat, np.int32(self.T), np.int32(self.E), np.float32(action_scale),
                        np.float32(action_bias), out, block=(block, 1, 1),
                        grid=(self.targets_grid if grid is None else int(grid), 1), shared=self.targets_lds)
        return out

    def gradients(self, obs, actions, rewards, done, next_values, theta, gamma, action_scale, action_bias,
                  returns_out=None, partials=None):
        """per-block partials [blocks, PT + 2] (gradient of the actor, of the critic, sum of squared errors, sum of
        Q(obs, mu(obs))) and the n-step returns [V, E]; the grid is the number of rows of `partials`"""
        returns_out = self.returns if returns_out is None else returns_out
        partials = self.partials if partials is None else partials
        self._check_batch(obs, self.T, self.O)
        self._check_batch(actions, self.T, 1)
        self._check_batch(rewards, self.T, 1)
        self._check_batch(done, self.T, 1, torch.int32)
        assert next_values.numel() == (self.T - 1) * self.E and next_values.dtype == torch.float32
        assert theta.numel() == self.PT and returns_out.numel() == self.rows
        assert partials.dim() == 2 and partials.shape[1] == self.PT + 2 and partials.is_contiguous()
        self.fn_gradients(obs, actions, rewards, done, next_values, theta, np.int32(self.T), np.int32(self.E),
                          np.int32(self.n_step), np.float32(gamma), np.float32(action_scale), np.float32(action_bias),
                          returns_out, partials, block=(TILE, 1, 1), grid=(int(partials.shape[0]), 1),
                          shared=self.gradients_lds)
        return partials, returns_out

    def reduce(self, partials=None, grads=None, sumsq=None, losses=None):
        """flat gradients [PT], sums of squares per tensor [12], (critic loss, actor loss)"""
        partials = self.partials if partials is None else partials
        grads, sumsq, losses = (self.grads if grads is None else grads, self.sumsq if sumsq is None else sumsq,
                                self.losses if losses is None else losses)
        assert partials.shape[1] == self.PT + 2 and partials.is_contiguous()
        assert grads.numel() == self.PT and sumsq.numel() == 2 * TENSORS_PER_NETWORK and losses.numel() == 2
        self.fn_reduce(partials, np.int32(partials.shape[0]), np.int32(self.H), np.int32(self.O), np.int64(self.rows),
                       grads, sumsq, losses, block=(REDUCE_THREADS, 1, 1), grid=(REDUCE_BLOCKS, 1), shared=0)
        return grads, sumsq, losses

    def apply(self, theta, target, exp_avg, exp_avg_sq, step, actor_lr, critic_lr, tau, max_norm=None, packed=None,
              grads=None, sumsq=None, betas=(0.9, 0.999), eps=1e-8):
        """clip (max_norm None or <= 0: off), Adam step number `step` (1 for the first), soft update, packed actor.
        step_size = lr / (1 - beta1^step) and sqrt(1 - beta2^step) are Python floats, as in torch.optim.Adam."""
        grads, sumsq = self.grads if grads is None else grads, self.sumsq if sumsq is None else sumsq
        for t in (theta, target, exp_avg, exp_avg_sq, grads):
            assert t.numel() == self.PT and t.dtype == torch.float32 and t.is_contiguous()
        assert step >= 1
        if packed is not None:
            OP = (self.O + 1) // 2 * 2
            assert packed.numel() == self.PA + self.H * (OP - self.O) and packed.dtype == torch.float32
        beta1, beta2 = betas
        bc1, bc2 = 1 - beta1 ** float(step), 1 - beta2 ** float(step)
        self.fn_apply(theta, target, exp_avg, exp_avg_sq, grads, sumsq, _NULL if packed is None else packed,
                      np.int32(self.H), np.int32(self.O), np.float32(max_norm if max_norm else 0.0),
                      np.float32(actor_lr / bc1), np.float32(critic_lr / bc1), np.float32(bc2 ** 0.5),
                      np.float32(1 - beta1), np.float32(beta2), np.float32(1 - beta2), np.float32(eps),
                      np.float32(tau), np.float32(1.0 - tau), block=(APPLY_THREADS, 1, 1), grid=(self.apply_grid, 1),
                      shared=0)

    def gradient_norms(self, sumsq=None):
        """(actor, critic): the sum of the 2-norms of the network's six gradient tensors -- the logged "Gradient norm"
        (reads the device)"""
        norms = torch.sqrt(self.sumsq if sumsq is None else sumsq).cpu().numpy().astype(np.float64)
        return float(norms[:TENSORS_PER_NETWORK].sum()), float(norms[TENSORS_PER_NETWORK:].sum())


def log_refusal(reason):
    logging.info(f"trainer.fused_update: {reason}; the update runs on the framework path")
