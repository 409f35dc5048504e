"""RendezvousPolicy: the Rendezvous example with a ONE-LAUNCH ROLLOUT that evaluates the policy network inside the kernel
(docs/custom_environments.md, "A policy inside the kernel").

The env is examples/rendezvous/rendezvous.py's, unchanged: same host step, same arrays, same step arguments.  The device
source next to this file, rendezvous_policy.hip, writes the step once as a `__device__` function and wraps it four times:
`HipRendezvousPolicyStep` (the plain step), `HipRendezvousPolicyTick` (include/wd_env_tick.h: draw, step and restart in
one launch) and `HipRendezvousPolicyRollout_H32` / `_H64` (include/wd_env_rollout.h: a policy of two hidden layers of 32 /
64 units is evaluated on every agent's observation row, the action drawn, the step run, the batch rows recorded and
finished replicas restarted, for a whole training batch of ticks in one launch).  `FusedRolloutMixin` packs those entries'
arguments.  `Trainer` takes the one launch when the config asks for it:

    registrar = EnvironmentRegistrar()
    registrar.add(env_backend=["cpu", "hip"], cuda_env_src_path=SOURCE)(RendezvousPolicy)
    wrapper = EnvWrapper(env_name="RendezvousPolicy", env_config={...}, num_envs=E, env_backend="hip",
                         env_registrar=registrar)
    config["trainer"]["fused_rollout_policy"] = "all"      # and a [32, 32] or [64, 64] fully connected model
    trainer = Trainer(env_wrapper=wrapper, config=config, ...)   # trainer.rollout_path == "one launch"

Without that key the class is driven per tick on its Tick entry, as RendezvousFused is.  The _H64 entry is bound to 512
threads (ROLLOUT_MAX_THREADS): with more than 512 agents only the width-32 policy runs inside the kernel.
"""
import importlib.util
import os
import sys

from warp_drive_amd.utils.custom_tick import FusedRolloutMixin

_HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(_HERE, "rendezvous_policy.hip")


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


class RendezvousPolicy(FusedRolloutMixin, _rendezvous.Rendezvous):
    name = "RendezvousPolicy"

    TICK_KERNEL = "HipRendezvousPolicyTick"
    TICK_STEP_ARGS = _rendezvous._STEP_ARGS  # the Tick and Rollout entries' leading parameters are the Step entry's
    ROLLOUT_KERNEL = "HipRendezvousPolicyRollout_H{width}"
    ROLLOUT_MAX_THREADS = {32: 1024, 64: 512}  # the entries' __launch_bounds__ in rendezvous_policy.hip
