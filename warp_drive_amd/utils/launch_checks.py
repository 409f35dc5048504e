"""What the envs' launch builders (`tick_launch`, `evaluate_launch`, `evaluate_actor_launch`, the custom-environment kit)
share: the refusal they raise, the float counts of the packed networks, the unpacking of `policy` / `actor` / `ou`, the
checks of the packed and of the record tensors, and the device side that Cartpole and the four other classic-control envs
have in common.  A leaf module: numpy at import, torch only inside the checks that compare a dtype, so the env modules
stay importable without torch.

Every check takes the exception class to raise.  A builder's class per condition is part of its contract:
`UnsupportedRolloutShape` is a capability answer the trainers catch (they keep the per-tick path), `AssertionError` is a
caller's bug and propagates.  For a record tensor an `AssertionError` carries (name, shape, dtype), what the `assert`s
these checks replace showed; a refusal carries a sentence.
"""
import numpy as np

from warp_drive_amd.utils.constants import Constants
from warp_drive_amd.utils.data_feed import DataFeed
from warp_drive_amd.utils.spaces import Box

NULL = np.uint64(0)   # a null pointer argument
MAX_ACTIONS = 8       # actions the in-kernel policies hold in registers


class UnsupportedRolloutShape(RuntimeError):
    """an env's tick entry was asked for a variant (live in-kernel policy, presampled actions, ...) that does not exist
    for this env shape -- a capability answer, raised explicitly (never an `assert`: it must survive `python -O` and must
    not be confused with an assertion that caught a bug)"""


def tick_tag():
    """the stream tag of the fused tick's draws"""
    from warp_drive_amd.managers.function_manager import _stream_tag

    return _stream_tag("tick")


# ------------------------------------------------------------------------------------------------------ float counts
# restated from csrc/kernels/rollout_policy.h (tests/test_launch_checks_host.py holds them to written-out numbers)
def rp_pad4(n):
    """rp_pad4: (n + 3) & ~3, whole 16-byte vectors"""
    return (int(n) + 3) // 4 * 4


def rp_policy_floats(I, H, A):
    """rp_policy_floats(I, H, A) = I * H + H + H * H + H + A * H + A: W0 [H][I], b0 [H], W1 [H][H], b1 [H], Wp [A][H],
    bp [A]; I = floats per row of W0 (the observation size, or TagGridWorld's padded 24)"""
    I, H, A = int(I), int(H), int(A)
    return I * H + H + H * H + H + A * H + A


def rp_actor_floats(H, O):
    """rp_actor_floats(H, O) = rp_actor_op(O) * H + H + H * H + H + H + 1: W0 [H][OP], b0 [H], W1 [H][H], b1 [H], Wa [H],
    ba [1]; OP = rp_actor_op(O) = (O + 1) & ~1, the observation size rounded up to even"""
    H, OP = int(H), (int(O) + 1) // 2 * 2
    return OP * H + H + H * H + H + H + 1


# --------------------------------------------------------------------------------------------------------- unpackers
def unpack_policy(policy, count=None, who=""):
    """policy = (packed weights, hidden width) -> packed, width; with `count` (a callable that gives the action count)
    -> packed, width, count"""
    try:
        packed, width = policy
        return (packed, int(width)) if count is None else (packed, int(width), int(count()))
    except (TypeError, ValueError, AttributeError) as err:
        raise UnsupportedRolloutShape(f"{who}policy = (packed weights, hidden width), not {policy!r}") from err


def unpack_policy_pair(policy):
    """((packed tagger policy, packed runner policy), hidden width) -> tagger, runner, width"""
    try:
        (tagger, runner), width = policy
        return tagger, runner, int(width)
    except (TypeError, ValueError) as err:
        raise UnsupportedRolloutShape("policy = ((packed tagger policy, packed runner policy), hidden width), "
                                      f"not {policy!r}") from err


def unpack_actor(actor):
    """actor = (packed weights, hidden width, action_scale, action_bias), the numbers as int / float"""
    try:
        packed, width, action_scale, action_bias = actor
        return packed, int(width), float(action_scale), float(action_bias)
    except (TypeError, ValueError) as err:
        raise UnsupportedRolloutShape("actor = (packed weights, hidden width, action_scale, action_bias), "
                                      f"not {actor!r}") from err


def unpack_ou(ou):
    """ou = (damping, stddev, scale) as floats"""
    try:
        damping, stddev, scale = (float(v) for v in ou)
        return damping, stddev, scale
    except (TypeError, ValueError) as err:
        raise UnsupportedRolloutShape(f"ou = (damping, stddev, scale), not {ou!r}") from err


# ------------------------------------------------------------------------------------------------------ tensor checks
def on_device(t):
    """is `t` a contiguous CUDA tensor?  (False for whatever is no tensor at all)"""
    return bool(getattr(t, "is_cuda", False) and t.is_contiguous())


def _refuse(error, name, t, sentence):
    """a record tensor `t` called `name` failed its check"""
    if error is AssertionError:
        raise AssertionError((name, tuple(getattr(t, "shape", ())), getattr(t, "dtype", None)))
    raise error(sentence)


def check_packed(t, n, error, what="the packed policy", detail=""):
    """`t` is a contiguous float32 CUDA tensor of `n` elements (the kernel reads it as float32 whatever it is), else
    `error`; `what` and `detail` say whose weights and for which sizes"""
    import torch

    if not (on_device(t) and t.dtype == torch.float32 and t.numel() == n):
        raise error(f"{what} must be a contiguous float32 CUDA tensor of {n} elements ({detail})")


def check_record(t, name, dtype, rows, tail, error, sentence=None, min_dims=1):
    """`t` is a contiguous CUDA tensor of torch's `dtype` (by name) with at least `rows` leading rows and behind them the
    exact shape `tail` (a tuple) or `tail` elements per row (an int), else `error` (with `sentence`, or one made here)"""
    import torch

    exact = isinstance(tail, tuple)
    ok = (on_device(t) and t.dtype == getattr(torch, dtype) and len(t.shape) >= min_dims and t.shape[0] >= rows
          and (tuple(t.shape[1:]) == tail if exact else int(np.prod(t.shape[1:])) == tail))
    if not ok:
        _refuse(error, name, t, sentence or f"{name} must be a contiguous {dtype} CUDA tensor "
                                           f"[>= {rows}, {', '.join(map(str, tail)) if exact else tail}]")


def batch_arguments(batch, rows, E, N, F, actions="int32", error=AssertionError, who=""):
    """the four `*_batch` arguments of a tick / rollout entry: four nulls without batch tensors, else [obs [T, E, N, F]
    float32, actions [T, E, N, 1] of dtype `actions`, rewards [T, E, N] float32, done [T, E] int32], T >= `rows`, each
    checked (`error`)"""
    if batch is None:
        return [NULL, NULL, NULL, NULL]
    want = {"obs": ((E, N, F), "float32"), "actions": ((E, N, 1), actions), "rewards": ((E, N), "float32"),
            "done": ((E,), "int32")}
    for key, (shape, dtype) in want.items():
        t = batch.get(key) if hasattr(batch, "get") else None
        got = None if t is None else (tuple(getattr(t, "shape", ())), getattr(t, "dtype", None))
        check_record(t, key, dtype, rows, shape, error,
                     f"{who}batch[{key!r}] must be a contiguous torch.{dtype} CUDA tensor "
                     f"[>= {rows}, {', '.join(map(str, shape))}], not {got}")
    return [batch["obs"], batch["actions"], batch["rewards"], batch["done"]]


def evaluation_outputs(outputs, E, error, reward_elements=None):
    """[reward_sum, steps, done] of an evaluation's `outputs`: contiguous CUDA tensors, float32 of at least
    `reward_elements` (default E) elements, int32 of at least E, int32 of at least E; else `error`"""
    import torch

    for key, dtype, n in (("reward_sum", torch.float32, E if reward_elements is None else reward_elements),
                          ("steps", torch.int32, E), ("done", torch.int32, E)):
        t = outputs[key]
        if not (on_device(t) and t.dtype == dtype and t.numel() >= n):
            _refuse(error, key, t, f"outputs[{key!r}] must be a contiguous {dtype} CUDA tensor of at least {n} elements")
    return [outputs["reward_sum"], outputs["steps"], outputs["done"]]


# ------------------------------------------------------------------------------------------- the shared device side
class SingleAgentDeviceEnv:
    """The device side that Cartpole and the four other classic-control envs share: one thread per replica, the reset
    pool of `state`, the step, and the one-launch evaluation with the policy inside the kernel.  Entries are named after
    the step's: Hip<X>EnvStep -> ...Tick, ...Rollout_H<width>, ...Evaluate_H<width>.  A class gives `_step_args()` (the
    step's argument names), STATE_DIM and, where the widths exist, ROLLOUT_POLICY_WIDTHS; what a trainer decides by
    (TICK_POOL_RESET, ROLLOUT_POLICY_OPT_IN, ROLLOUT_POOL_RESET) is each class's own."""
    TICK_HEADS = 1          # action heads the fused tick kernel samples (RolloutEngine)
    ticks_per_launch = 1    # > 1: fixed-policy rollout, T ticks fused per launch
    _PACKED_DETAIL = "observation {O}, width {width}, {n_act} actions"

    def _obs_size(self):
        """floats of an observation row"""
        return int(self.cuda_data_manager.get_shape(Constants.OBSERVATIONS)[-1])

    def _entry(self, suffix):
        return self.cuda_step.name.replace("Step", suffix)

    def _n_envs(self):
        return int(self.cuda_data_manager.meta_info("n_envs"))

    def _checked_policy(self, packed, width, n_act, error):
        """floats of the packed policy of this env, `packed` checked against them"""
        O = self._obs_size()
        n_w = rp_policy_floats(O, width, n_act)
        check_packed(packed, n_w, error, detail=self._PACKED_DETAIL.format(O=O, width=width, n_act=n_act))
        return n_w

    def get_reset_pool_dictionary(self):
        pool = DataFeed()
        if self.reset_pool_size >= 2:
            states = np.stack([np.atleast_2d(self._draw_initial_state(fixed=False))
                               for _ in range(self.reset_pool_size)], axis=0)
            assert states.ndim == 3 and states.shape[2] == self.STATE_DIM
            pool.add_pool_for_reset(name="state_reset_pool", data=states, reset_target="state")
        return pool

    def step_launch(self):
        block = (256, 1, 1)
        grid = (max(1, min(4096, (self._n_envs() + 255) // 256)), 1)
        return self.cuda_step, self.cuda_step_function_feed(self._step_args()), block, grid, 0

    def step(self, actions=None):
        self.timestep += 1
        if self.env_backend != "hip":
            raise Exception(f"{type(self).__name__} expects env_backend = 'hip'")
        fn, args, block, grid, shared = self.step_launch()
        fn(*args, block=block, grid=grid, shared=shared)

    def has_live_policy_evaluate(self, width, n_actions):
        """does an evaluation kernel exist that runs one episode of every replica with the policy network inside it
        (...Evaluate_H<width>, Trainer.evaluate_episodes)?  The same widths and action counts as the rollout entries;
        the Box envs have none."""
        if isinstance(self.action_space[0], Box) or int(width) not in getattr(self, "ROLLOUT_POLICY_WIDTHS", ()) \
                or not 1 <= int(n_actions) <= MAX_ACTIONS:
            return False
        return bool(self.cuda_function_manager.has_function(self._entry(f"Evaluate_H{int(width)}")))

    def evaluate_launch(self, sampler, policy, use_argmax, outputs, action_trace=None, ticks=None, n_actions=None):
        """One episode of every replica in ONE launch (...Evaluate_H<width>): from the state, observation and timestep
        the arrays hold, at most `ticks` (default: episode_length) ticks of policy network -> action (use_argmax: the
        first maximum of the probabilities; else the counting draw of the fused tick) -> step, up to the first done.
        policy = (packed float32 CUDA tensor, hidden width) as in `tick_launch`; `n_actions` defaults to the env's action
        count.  outputs = {"reward_sum": float32, "steps": int32, "done": int32}, CUDA tensors of at least n_envs
        elements; `action_trace` (optional) int32 [>= ticks, n_envs]: row k = tick k's actions.  The launch writes those,
        and in sampled mode the sampler's epoch words; the env's arrays are read only.
        Returns (function, arguments, block, grid, shared bytes)."""
        fm = self.cuda_function_manager
        packed, width, n_act = unpack_policy(policy, lambda: self.action_space[0].n if n_actions is None else n_actions)
        if not self.has_live_policy_evaluate(width, n_act):
            raise UnsupportedRolloutShape(f"{type(self).__name__} has no in-kernel evaluation of width {width} with "
                                          f"{n_act} actions")
        E = self._n_envs()
        n_w = self._checked_policy(packed, width, n_act, UnsupportedRolloutShape)
        T = int(self.episode_length if ticks is None else ticks)
        out_args = evaluation_outputs(outputs, E, AssertionError)
        if action_trace is not None:
            check_record(action_trace, "action_trace", "int32", T, E, AssertionError)
        name = self._entry(f"Evaluate_H{width}")
        fm.initialize_functions([name])
        _, args, block, grid, _ = self.step_launch()
        args = list(args) + [sampler.rng_state, np.int32(n_act), tick_tag(), np.int32(T), packed, np.int32(width),
                             np.int32(1 if use_argmax else 0)] + out_args + \
            [NULL if action_trace is None else action_trace]
        return fm.get_function(name), args, block, grid, 4 * n_w
