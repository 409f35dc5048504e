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

from warp_drive_amd.training.pg_update_kernels import (LD, RETURNS_ENTRY, SUMS, _admitted_tail, _pad4, _PgUpdateLaunches,
                                                       net_floats)

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
    ok, why = _admitted_tail(fc_dims, obs_size, (OBS,), f"the gridworld update kernels take {OBS}", dtype, normalize_return,
                             normalize_advantage, neg_pos_env_ratio, world_size, algorithm, one_launch_rollout)
    if not ok:
        return ok, why
    if not gridworld_packing:
        return False, "the rollout's packed policy is not pack_gridworld_policy's layout"
    return True, ""


class PgGridworldUpdateKernels(_PgUpdateLaunches):
    """The five launches for one policy of (E, T, n, H): rows = T * E * n; the Values and Gradients entries take no shape
    argument, Reduce and Apply take H."""

    def __init__(self, function_manager, E, T, n, H, device, compute_units=None):
        assert H in HIDDEN, H
        self._setup(function_manager, kernel_names(H), (T, E, n), H, OBS, ACTIONS, values_lds_bytes(H), gradients_lds_bytes(H),
                    packed_floats(H), device, compute_units)

    def _shape_args(self, per_row):
        return () if per_row else (np.int32(self.H),)
