"""warp_drive_amd/utils/launch_checks.py on the host alone (no GPU, no kernel built): every way a tensor can be wrong is
refused with the class the caller names, a missing batch gives four nulls, the float counts equal numbers written out
here and the old public names equal them, the env modules still import without torch, and `UnsupportedRolloutShape` is one
class whichever module it is taken from."""
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from warp_drive_amd.utils import launch_checks as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERRORS = (AssertionError, lc.UnsupportedRolloutShape, ValueError)


def _tensor(shape, dtype, cuda=True, contiguous=True):
    n = int(np.prod(shape))
    return types.SimpleNamespace(is_cuda=cuda, is_contiguous=lambda: contiguous, dtype=dtype, shape=tuple(shape),
                                 numel=lambda: n)


# --------------------------------------------------------------------------------------------------- the float counts
# elements of W0 [H][I], b0 [H], W1 [H][H], b1 [H], Wp [A][H], bp [A], added up by hand: {H: {O: [A = 1, 2, 3, 5, 8]}}
ACTIONS = (1, 2, 3, 5, 8)
POLICY_FLOATS = {32: {2: [1185, 1218, 1251, 1317, 1416], 3: [1217, 1250, 1283, 1349, 1448],
                      4: [1249, 1282, 1315, 1381, 1480], 6: [1313, 1346, 1379, 1445, 1544]},
                 64: {2: [4417, 4482, 4547, 4677, 4872], 3: [4481, 4546, 4611, 4741, 4936],
                      4: [4545, 4610, 4675, 4805, 5000], 6: [4673, 4738, 4803, 4933, 5128]}}
# W0 [H][OP], b0 [H], W1 [H][H], b1 [H], Wa [H], ba [1], OP = O rounded up to even: {H: {O: floats}}
ACTOR_FLOATS = {32: {2: 1185, 3: 1249, 4: 1249, 6: 1313}, 64: {2: 4417, 3: 4545, 4: 4545, 6: 4673}}
GRIDWORLD_FLOATS = {32: (2021, 2024), 64: (6085, 6088)}   # rows of 24 floats, 5 actions: (as counted, in whole float4)


def test_float_counts_equal_the_numbers_written_out():
    for H, by_obs in POLICY_FLOATS.items():
        for O, counts in by_obs.items():
            assert [lc.rp_policy_floats(O, H, A) for A in ACTIONS] == counts, (H, O)
            assert lc.rp_actor_floats(H, O) == ACTOR_FLOATS[H][O], (H, O)
    assert [lc.rp_pad4(n) for n in (0, 1, 3, 4, 5, 1282, 1315, 5000)] == [0, 4, 4, 4, 8, 1284, 1316, 5000]
    for H, (counted, padded) in GRIDWORLD_FLOATS.items():
        assert lc.rp_policy_floats(24, H, 5) == counted and lc.rp_pad4(counted) == padded


def test_the_old_public_names_give_the_same_counts():
    from warp_drive_amd.envs.cartpole import CUDAClassicControlCartPoleEnv
    from warp_drive_amd.envs.classic_control import rollout_actor_floats
    from warp_drive_amd.envs.tag_gridworld import gridworld_policy_floats
    from warp_drive_amd.utils import custom_tick

    for H in (32, 64):
        assert gridworld_policy_floats(H) == lc.rp_pad4(lc.rp_policy_floats(24, H, 5)) == GRIDWORLD_FLOATS[H][1]
        for O in (2, 3, 4, 6):
            assert rollout_actor_floats(O, H) == ACTOR_FLOATS[H][O]
            for A, n in zip(ACTIONS, POLICY_FLOATS[H][O]):
                assert custom_tick.rollout_policy_floats(O, H, A) == n
        for A, n in zip(ACTIONS, POLICY_FLOATS[H][4]):   # Cartpole: four inputs; the policy part of the pooled entries' LDS
            assert CUDAClassicControlCartPoleEnv.pool_rollout_lds_bytes(H, A, 0, False) == 4 * ((n + 3) // 4 * 4)
            assert CUDAClassicControlCartPoleEnv.pool_rollout_lds_bytes(H, A, 7, True) == 4 * ((n + 3) // 4 * 4) + 112
    assert CUDAClassicControlCartPoleEnv.pool_rollout_lds_bytes(0, 2, 7, True) == 112


# ------------------------------------------------------------------------------------------------ the packed tensor
@pytest.mark.parametrize("error", ERRORS)
def test_packed_tensor_check(error):
    n = 1282
    lc.check_packed(_tensor((n,), torch.float32), n, error)
    lc.check_packed(_tensor((2, n // 2), torch.float32), n, error)   # (elements count, not the shape)
    bad = [_tensor((n,), torch.float32, cuda=False), _tensor((n,), torch.float32, contiguous=False),
           _tensor((n,), torch.float64), _tensor((n,), torch.float16), _tensor((n,), torch.int32),
           _tensor((n + 1,), torch.float32), _tensor((n - 1,), torch.float32), None, "weights"]
    for t in bad:
        with pytest.raises(error) as caught:
            lc.check_packed(t, n, error, "the packed actor", "observation 3, width 32")
        assert type(caught.value) is error
        assert str(caught.value) == ("the packed actor must be a contiguous float32 CUDA tensor of 1282 elements "
                                     "(observation 3, width 32)")


# ------------------------------------------------------------------------------------------------ the record tensors
@pytest.mark.parametrize("error", ERRORS)
def test_record_tensor_check(error):
    T, E = 9, 70
    lc.check_record(_tensor((T, E, 1, 4), torch.float32), "obs", "float32", T, (E, 1, 4), error)
    lc.check_record(_tensor((T + 3, E, 1, 4), torch.float32), "obs", "float32", T, (E, 1, 4), error)   # more rows are fine
    lc.check_record(_tensor((T, E), torch.int32), "done", "int32", T, (E,), error)
    for shape in ((T, E), (T, E, 1), (T, 7, 10)):    # an element count per row
        lc.check_record(_tensor(shape, torch.float32), "trace", "float32", T, E, error)
    lc.check_record(_tensor((T,), torch.float32), "trace", "float32", T, 1, error)   # [T] is T rows of one element ...
    with pytest.raises(error):                                                        # ... unless two dimensions are asked
        lc.check_record(_tensor((T,), torch.float32), "trace", "float32", T, 1, error, min_dims=2)
    exact = [_tensor((T, E, 1, 4), torch.float32, cuda=False), _tensor((T, E, 1, 4), torch.float32, contiguous=False),
             _tensor((T, E, 1, 4), torch.float64), _tensor((T, E, 1, 4), torch.int32), _tensor((T - 1, E, 1, 4), torch.float32),
             _tensor((T, E, 1, 5), torch.float32), _tensor((T, E, 4), torch.float32), _tensor((T, E + 1, 1, 4), torch.float32),
             _tensor((), torch.float32), None, 3]
    for t in exact:
        with pytest.raises(error) as caught:
            lc.check_record(t, "obs", "float32", T, (E, 1, 4), error)
        assert type(caught.value) is error
        if error is AssertionError:   # what the asserts showed: the name and what was given
            assert caught.value.args[0] == ("obs", tuple(getattr(t, "shape", ())), getattr(t, "dtype", None))
        else:
            assert str(caught.value) == "obs must be a contiguous float32 CUDA tensor [>= 9, 70, 1, 4]"
    counted = [_tensor((T, E), torch.float32, cuda=False), _tensor((T, E), torch.float32, contiguous=False),
               _tensor((T, E), torch.float64), _tensor((T - 1, E), torch.float32), _tensor((T, E + 1), torch.float32),
               _tensor((T, E, 2), torch.float32), None]
    for t in counted:
        with pytest.raises(error) as caught:
            lc.check_record(t, "mean_trace", "float32", T, E, error)
        if error is not AssertionError:
            assert str(caught.value) == "mean_trace must be a contiguous float32 CUDA tensor [>= 9, 70]"
    with pytest.raises(lc.UnsupportedRolloutShape, match="^said by the caller$"):
        lc.check_record(None, "obs", "float32", T, (E,), lc.UnsupportedRolloutShape, "said by the caller")


def _batch(T, E, N, F, actions=torch.int32):
    return {"obs": _tensor((T, E, N, F), torch.float32), "actions": _tensor((T, E, N, 1), actions),
            "rewards": _tensor((T, E, N), torch.float32), "done": _tensor((T, E), torch.int32)}


def test_no_batch_gives_four_nulls():
    for error in ERRORS:
        nulls = lc.batch_arguments(None, 9, 70, 1, 4, error=error)
        assert len(nulls) == 4 and all(type(a) is np.uint64 and a == 0 for a in nulls)
    assert type(lc.NULL) is np.uint64 and lc.NULL == 0


@pytest.mark.parametrize("error", ERRORS)
def test_batch_arguments(error):
    T, E, N, F = 9, 70, 5, 21
    batch = _batch(T + 1, E, N, F)
    assert lc.batch_arguments(batch, T, E, N, F, error=error) == [batch["obs"], batch["actions"], batch["rewards"], batch["done"]]
    box = _batch(T, E, 1, 3, actions=torch.float32)
    assert lc.batch_arguments(box, T, E, 1, 3, actions="float32", error=error)[1] is box["actions"]
    with pytest.raises(error):   # the discrete entries record int32 actions
        lc.batch_arguments(box, T, E, 1, 3, error=error)
    wrong = {"obs": [(T, E, N, F + 1), (T, E, N), (T, E + 1, N, F)], "actions": [(T, E, N), (T, E, N, 2)],
             "rewards": [(T, E, N, 1), (T, E, N + 1)], "done": [(T, E, 1), (T, E - 1)]}
    for key, good in batch.items():
        bad = [_tensor(good.shape, good.dtype, cuda=False), _tensor(good.shape, good.dtype, contiguous=False),
               _tensor(good.shape, torch.float64), _tensor((T - 1,) + good.shape[1:], good.dtype), None]
        bad += [_tensor(shape, good.dtype) for shape in wrong[key]]
        for t in bad:
            with pytest.raises(error) as caught:
                lc.batch_arguments(dict(batch, **{key: t}), T, E, N, F, error=error, who="Env (Kernel): ")
            assert type(caught.value) is error
            if error is AssertionError:
                assert caught.value.args[0][0] == key
            else:
                assert str(caught.value).startswith(f"Env (Kernel): batch[{key!r}] must be a contiguous torch.")
                assert f"[>= {T}, " in str(caught.value)
        with pytest.raises(error):   # a missing tensor, and a batch that is no mapping
            lc.batch_arguments({k: v for k, v in batch.items() if k != key}, T, E, N, F, error=error)
    with pytest.raises(error):
        lc.batch_arguments([batch["obs"]], T, E, N, F, error=error)


@pytest.mark.parametrize("error", ERRORS)
def test_evaluation_outputs(error):
    E = 70
    out = {"reward_sum": _tensor((E + 3,), torch.float32), "steps": _tensor((E,), torch.int32), "done": _tensor((E, 1), torch.int32)}
    assert lc.evaluation_outputs(out, E, error) == [out["reward_sum"], out["steps"], out["done"]]
    with pytest.raises(error):   # five rewards per replica
        lc.evaluation_outputs(out, E, error, reward_elements=5 * E)
    lc.evaluation_outputs(dict(out, reward_sum=_tensor((E, 5), torch.float32)), E, error, reward_elements=5 * E)
    for key, good in out.items():
        other = torch.float64 if good.dtype == torch.float32 else torch.int64
        swapped = torch.int32 if good.dtype == torch.float32 else torch.float32
        for t in (_tensor((E,), good.dtype, cuda=False), _tensor((E,), good.dtype, contiguous=False), _tensor((E,), other),
                  _tensor((E,), swapped), _tensor((E - 1,), good.dtype), None):
            with pytest.raises(error) as caught:
                lc.evaluation_outputs(dict(out, **{key: t}), E, error)
            assert type(caught.value) is error
            if error is not AssertionError:
                assert str(caught.value) == (f"outputs[{key!r}] must be a contiguous {good.dtype} CUDA tensor of at least "
                                             f"{E} elements")


# ------------------------------------------------------------------------------------------------------ the unpackers
def test_unpackers_refuse_what_has_another_form():
    packed = _tensor((10,), torch.float32)
    assert lc.unpack_policy((packed, np.int64(32))) == (packed, 32) and type(lc.unpack_policy((packed, 32.0))[1]) is int
    assert lc.unpack_policy((packed, "64"), count=lambda: np.int32(3)) == (packed, 64, 3)
    for policy in (packed, (packed,), (packed, 32, 1), (packed, "x"), (packed, None), None):
        with pytest.raises(lc.UnsupportedRolloutShape, match=r"^Env: policy = \(packed weights, hidden width\), not "):
            lc.unpack_policy(policy, who="Env: ")

    def no_count():
        return types.SimpleNamespace().n   # a Box space has no `n`

    for count in (no_count, lambda: "x", lambda: None):
        with pytest.raises(lc.UnsupportedRolloutShape, match=r"^policy = \(packed weights, hidden width\), not "):
            lc.unpack_policy((packed, 32), count=count)
    assert lc.unpack_policy_pair(((packed, packed), "32")) == (packed, packed, 32)
    for policy in (packed, (packed, 32), ((packed,), 32), ((packed, packed, packed), 32), ((packed, packed), "x"), None):
        with pytest.raises(lc.UnsupportedRolloutShape, match=r"^policy = \(\(packed tagger policy, packed runner policy\)"):
            lc.unpack_policy_pair(policy)
    got = lc.unpack_actor((packed, np.int32(64), 2, np.float32(0.5)))
    assert got == (packed, 64, 2.0, 0.5) and [type(v) for v in got[1:]] == [int, float, float]
    for actor in (packed, (packed, 32), (packed, 32, 1.0), (packed, "x", 1.0, 0.0), (packed, 32, "s", 0.0), (packed, 32, 1.0, None)):
        with pytest.raises(lc.UnsupportedRolloutShape, match=r"^actor = \(packed weights, hidden width, action_scale, action_bias\)"):
            lc.unpack_actor(actor)
    assert lc.unpack_ou((1, np.float32(0.25), "0.5")) == (1.0, 0.25, 0.5)
    for ou in (None, 3.0, (1, 2), (1, 2, 3, 4), (1, 2, "x"), (1, None, 3)):
        with pytest.raises(lc.UnsupportedRolloutShape, match=r"^ou = \(damping, stddev, scale\), not "):
            lc.unpack_ou(ou)


# ----------------------------------------------------------------------------------------------------- the shared base
def test_cartpole_takes_the_shared_device_side_without_the_classic_control_switches():
    from warp_drive_amd.envs.cartpole import CUDAClassicControlCartPoleEnv as Cartpole
    from warp_drive_amd.envs.classic_control import _CUDAClassicControlEnv

    base = lc.SingleAgentDeviceEnv
    for name in ("step_launch", "step", "get_reset_pool_dictionary", "has_live_policy_evaluate", "evaluate_launch"):
        assert getattr(Cartpole, name) is getattr(_CUDAClassicControlEnv, name) is getattr(base, name), name
    for name in ("TICK_POOL_RESET", "ROLLOUT_POLICY_OPT_IN", "ROLLOUT_POOL_RESET"):
        assert not hasattr(base, name), name
    assert _CUDAClassicControlEnv.TICK_POOL_RESET is True and _CUDAClassicControlEnv.ROLLOUT_POLICY_OPT_IN is True
    assert not getattr(Cartpole, "TICK_POOL_RESET", False)
    assert isinstance(vars(Cartpole)["ROLLOUT_POLICY_OPT_IN"], property) and isinstance(vars(Cartpole)["ROLLOUT_POOL_RESET"], property)
    assert Cartpole.TICK_HEADS == _CUDAClassicControlEnv.TICK_HEADS == 1 and Cartpole.ticks_per_launch == 1
    plain, pooled = Cartpole(episode_length=5, seed=1), Cartpole(episode_length=5, seed=1, reset_pool_size=3)
    assert (plain.ROLLOUT_POLICY_OPT_IN, plain.ROLLOUT_POOL_RESET) == (False, False)
    assert (pooled.ROLLOUT_POLICY_OPT_IN, pooled.ROLLOUT_POOL_RESET) == (True, True)
    assert plain.cuda_data_manager is None and plain._obs_size() == 4   # a constant: no data-manager query
    assert np.asarray(pooled.get_reset_pool_dictionary()["state_reset_pool"]["data"]).shape == (3, 1, 4)
    plain.cuda_step = types.SimpleNamespace(name="HipClassicControlCartPoleEnvStep")
    assert [plain._entry(s) for s in ("Tick", "Rollout_H32", "Evaluate_H64")] == [
        "HipClassicControlCartPoleEnvTick", "HipClassicControlCartPoleEnvRollout_H32", "HipClassicControlCartPoleEnvEvaluate_H64"]


# -------------------------------------------------------------------------------------------------------- import weight
MODULES = ["warp_drive_amd.utils.launch_checks", "warp_drive_amd.utils.custom_tick", "warp_drive_amd.envs.cartpole",
           "warp_drive_amd.envs.classic_control", "warp_drive_amd.envs.tag_gridworld", "warp_drive_amd.envs.tag_continuous"]


@pytest.mark.parametrize("module", MODULES)
def test_module_imports_without_torch_and_without_the_rollout_engine(module):
    code = (f"import sys; sys.path.insert(0, {ROOT!r}); import {module}; "
            "print('torch' in sys.modules, 'warp_drive_amd.rollout' in sys.modules)")
    out = subprocess.run([sys.executable, "-c", code], check=True, capture_output=True, text=True).stdout
    assert out.split() == ["False", "False"], (module, out)


def test_one_exception_class_whichever_module_it_is_taken_from():
    from warp_drive_amd import rollout
    from warp_drive_amd.utils import custom_tick

    assert rollout.UnsupportedRolloutShape is lc.UnsupportedRolloutShape is custom_tick.UnsupportedRolloutShape
    assert issubclass(lc.UnsupportedRolloutShape, RuntimeError) and lc.UnsupportedRolloutShape.__doc__


def test_formulas_and_tensor_predicates_stand_in_the_shared_module_only():
    """over warp_drive_amd/envs and warp_drive_amd/utils: the square term of the float counts, the contiguity test and the
    import of the exception from the rollout engine occur in launch_checks.py or nowhere"""
    patterns = {r"H \* H|width \* width": True, r"\.is_contiguous\(\)": True,
                r"from warp_drive_amd\.rollout import UnsupportedRolloutShape": False}
    for folder in ("envs", "utils"):
        here = os.path.join(ROOT, "warp_drive_amd", folder)
        for name in sorted(f for f in os.listdir(here) if f.endswith(".py")):
            text = open(os.path.join(here, name)).read()
            for pattern, in_shared in patterns.items():
                found = re.search(pattern, text) is not None
                assert found == (in_shared and name == "launch_checks.py"), (folder, name, pattern)
