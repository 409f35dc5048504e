"""training/pg_update_kernels.py's five launches for the in-kernel policy of a CUSTOM environment: the entries the macro
WD_PG_UPDATE_ENTRIES(Name, F) of include/wd_env_update.h defines in the environment's own code object (the returns entry
is wd_kernels_update.hsaco's):

    Hip<Name>PgValues_H<H>      values [T, E, n] of the recorded rows (n agents per replica)
    HipDiscountedReturns        the existing entry on `values` (n agents, w = 1, v_col = 0): returns and advantages [T, E, n]
    Hip<Name>PgGradients_H<H>   forward, the objective's gradient, backward: one partial of the eight tensors per block
    Hip<Name>PgReduce           partials -> flat gradient, per-tensor sums of squares, the four sums of the objective
    Hip<Name>PgApply            clip, Adam, refill of the rollout's packed policy (pack_rollout_policy: a prefix of the flat
                                parameters)

A row is (t, replica, agent): rows = T * E * n, and the objective's means are over all of them.  The observation size F
(1 .. 32) is fixed when the environment's source is compiled; the action count A (1 .. 8) is a launch argument.  The
network is the module's -- W0 [H][F], b0, W1 [H][H], b1, Wp [A][H], bp, Wv [1][H], bv, float32 -- flat in that order
(`FlatPolicy` of training/pg_update_kernels.py, as it is).  `admitted_custom_shape` says which policies this serves;
warp_drive_amd/utils/custom_tick.py::FusedUpdateMixin asks it for an env class and builds the launches."""
import numpy as np
import torch

from warp_drive_amd.training.pg_update_kernels import (HIDDEN, LD, LDS_LIMIT, MAX_ACTIONS, RETURNS_ENTRY, SUMS,
                                                       _admitted_tail, _pad4, _PgUpdateLaunches, packed_floats)

MAX_OBS = 32               # WD_UPD_MAX_OBS of include/wd_env_update.h
MAX_BLOCKS_PER_CU = 2      # blocks of the gradient launch per compute unit, where two are resident (default_blocks_per_cu)


def values_lds_bytes(H, F):
    """wd_pg_values_lds_floats: W0 with rows of pad4(F) floats, eight head rows and eight bias slots whatever A is"""
    return 4 * _pad4(H * _pad4(F) + H + H * H + H + MAX_ACTIONS * H + MAX_ACTIONS + H + 1)


def gradients_lds_bytes(H, F):
    """wd_pg_gradients_lds_floats: ... and the staged tile"""
    return values_lds_bytes(H, F) + 4 * LD * (2 * H + F + (MAX_ACTIONS + 1) + SUMS)


def default_blocks_per_cu(H, F):
    """blocks of the gradient launch per compute unit: two where the LDS of a compute unit holds two of them (every
    width-32 shape), else one (every width-64 shape).  docs/rounds/r39.md: at width 32 every window of two blocks lay below
    every window of one at 4 M and at 400 k rows; at width 64, where a second block is not resident but queued, two lost
    at both."""
    return max(1, min(MAX_BLOCKS_PER_CU, LDS_LIMIT // gradients_lds_bytes(H, F)))


def kernel_names(prefix, H):
    """the five launches, in order; `prefix`: "Hip<Name>Pg" """
    return [f"{prefix}Values_H{H}", RETURNS_ENTRY, f"{prefix}Gradients_H{H}", f"{prefix}Reduce", f"{prefix}Apply"]


def all_kernel_names(prefix):
    """the six entries WD_PG_UPDATE_ENTRIES defines"""
    return sorted({n for H in HIDDEN for n in kernel_names(prefix, H)} - {RETURNS_ENTRY})


def admitted_custom_shape(one_launch_rollout, rollout_packing, n_policies, n_agents, head_sizes, fc_dims, obs_size, dtype,
                          normalize_return, normalize_advantage, neg_pos_env_ratio, world_size, algorithm):
    """(True, "") when the kit's update kernels serve this policy, else (False, why).  One policy, n >= 1 agents;
    `rollout_packing`: the rollout's packed policy is pack_rollout_policy's layout."""
    if n_policies != 1:
        return False, f"{n_policies} policies: the update kernels of wd_env_update.h train one"
    if n_agents < 1:
        return False, f"{n_agents} agents: the update kernels train at least one per replica"
    heads = [int(a) for a in head_sizes]
    if len(heads) != 1:
        return False, f"{len(heads)} action heads: the update kernels take one"
    if not 1 <= heads[0] <= MAX_ACTIONS:
        return False, f"{heads[0]} actions: the update kernels take 1 to {MAX_ACTIONS}"
    ok, why = _admitted_tail(fc_dims, obs_size, range(1, MAX_OBS + 1), f"the update kernels of wd_env_update.h take 1 to {MAX_OBS}",
                             dtype, normalize_return, normalize_advantage, neg_pos_env_ratio, world_size, algorithm,
                             one_launch_rollout)
    if not ok:
        return ok, why
    if not rollout_packing:
        return False, "the rollout's packed policy is not pack_rollout_policy's layout"
    H, F = int(fc_dims[0]), int(obs_size)
    if max(values_lds_bytes(H, F), gradients_lds_bytes(H, F)) > LDS_LIMIT:
        return False, f"{gradients_lds_bytes(H, F)} bytes of LDS: over the {LDS_LIMIT} of a compute unit"
    return True, ""


class PgCustomUpdateKernels(_PgUpdateLaunches):
    """The five launches for the policy of (E, T, n, H, F, A) on the entries `entry_prefix`Values_H<H> ...: rows =
    T * E * n; the Values and Gradients entries take A, Reduce and Apply take (H, A).  blocks_per_cu: the gradient
    launch's grid is one block per tile up to this many per compute unit (None: default_blocks_per_cu)."""

    def __init__(self, function_manager, entry_prefix, E, T, n, H, F, A, device, compute_units=None, blocks_per_cu=None):
        assert H in HIDDEN and 1 <= F <= MAX_OBS and 1 <= A <= MAX_ACTIONS, (H, F, A)
        self._setup(function_manager, kernel_names(entry_prefix, H), (T, E, n), H, F, A, values_lds_bytes(H, F),
                    gradients_lds_bytes(H, F), packed_floats(H, F, A), device, compute_units)
        self.blocks_per_cu = default_blocks_per_cu(H, F) if blocks_per_cu is None else int(blocks_per_cu)
        assert self.blocks_per_cu >= 1
        self.gradients_grid = max(1, min(self.tiles, self.blocks_per_cu * self.compute_units))
        self.partials = torch.zeros((self.gradients_grid, self.P + SUMS), dtype=torch.float32, device=self.device)

    def _shape_args(self, per_row):
        return (np.int32(self.A),) if per_row else (np.int32(self.H), np.int32(self.A))

