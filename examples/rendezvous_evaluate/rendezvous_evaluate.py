"""RendezvousEvaluate: the Rendezvous example whose WHOLE TRAINING AND EVALUATION CYCLE runs as kernels -- the one-launch
rollout with the policy inside it (examples/rendezvous_policy/), the A2C / PPO update as five launches
(examples/rendezvous_update/) AND `Trainer.evaluate_episodes` as ONE launch, greedy or sampled
(docs/custom_environments.md, "Evaluation in one launch").

The env is examples/rendezvous/rendezvous.py's, unchanged: same host step, same arrays, same step arguments.  The device
source next to this file, rendezvous_evaluate.hip, is self-contained: the step written once as a `__device__` function, its
Step, Tick and Rollout_H32 / _H64 wrappers, the WD_PG_UPDATE_ENTRIES line, and the two entries
HipRendezvousEvaluateEvaluate_H32 / _H64 written from one template with include/wd_env_evaluate.h.  `FusedEvaluateMixin`
packs their arguments; the class names them (EVALUATE_KERNEL):

    registrar = EnvironmentRegistrar()
    registrar.add(env_backend=["cpu", "hip"], cuda_env_src_path=SOURCE)(RendezvousEvaluate)
    wrapper = EnvWrapper(env_name="RendezvousEvaluate", env_config={...}, num_envs=E, env_backend="hip",
                         env_registrar=registrar)
    config["trainer"]["fused_rollout_policy"] = "all"      # and a [32, 32] or [64, 64] fully connected model
    config["trainer"]["fused_update"] = "all"              # A2C / PPO, float32, no normalisations
    trainer = Trainer(env_wrapper=wrapper, config=config, ...)
    trainer.train(...)
    reward_sum, steps = trainer.evaluate_episodes(use_argmax=True)
    # trainer.rollout_path == "one launch", trainer.update_path == {policy: "kernels"},
    # trainer.evaluation_path == "one launch"

Without `fused_rollout_policy: "all"` the evaluation runs per tick, as RendezvousUpdate's does; so does a shape the
entries do not serve (an env with a reset pool, a block over an entry's launch bound, a width other than 32 / 64).
"""
import importlib.util
import os
import sys

from warp_drive_amd.utils.custom_tick import FusedEvaluateMixin, FusedUpdateMixin

_HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(_HERE, "rendezvous_evaluate.hip")


def _parent_module():
    """examples/rendezvous/rendezvous.py, imported by path (the examples are not a package)"""
    name = "rendezvous_example"
    if name not in sys.modules:
        path = os.path.join(os.path.dirname(_HERE), "rendezvous", "rendezvous.py")
        spec = importlib.util.spec_from_file_location(name, path)
        module = importlib.util.module_from_spec(spec)
        sys.modules[name] = module
        spec.loader.exec_module(module)
    return sys.modules[name]


_rendezvous = _parent_module()


class RendezvousEvaluate(FusedEvaluateMixin, FusedUpdateMixin, _rendezvous.Rendezvous):
    name = "RendezvousEvaluate"

    TICK_KERNEL = "HipRendezvousEvaluateTick"
    TICK_STEP_ARGS = _rendezvous._STEP_ARGS  # the Tick, Rollout and Evaluate entries' leading parameters are the Step entry's
    ROLLOUT_KERNEL = "HipRendezvousEvaluateRollout_H{width}"
    ROLLOUT_MAX_THREADS = {32: 1024, 64: 512}  # the entries' __launch_bounds__ in rendezvous_evaluate.hip
    UPDATE_KERNEL_PREFIX = "HipRendezvousEvaluatePg"  # WD_PG_UPDATE_ENTRIES(RendezvousEvaluate, 5)
    UPDATE_OBS_SIZE = 5
    EVALUATE_KERNEL = "HipRendezvousEvaluateEvaluate_H{width}"
    EVALUATE_MAX_THREADS = {32: 1024, 64: 512}  # the Evaluate entries' __launch_bounds__
