"""RendezvousUpdate: the Rendezvous example whose WHOLE TRAINING ITERATION runs as kernels -- the one-launch rollout with
the policy inside it (examples/rendezvous_policy/) AND the A2C / PPO update as five launches
(docs/custom_environments.md, "The update as kernels").

The env is examples/rendezvous/rendezvous.py's, unchanged: same host step, same arrays, same step arguments.  The device
source next to this file, rendezvous_update.hip, is self-contained: the step written once as a `__device__` function, its
Step, Tick and Rollout_H32 / _H64 wrappers (include/wd_env_tick.h, include/wd_env_rollout.h), and ONE more line,

    WD_PG_UPDATE_ENTRIES(RendezvousUpdate, 5)        // include/wd_env_update.h; 5 = observation floats of a row

which defines HipRendezvousUpdatePgValues_H32 / _H64, ...PgGradients_H32 / _H64, ...PgReduce and ...PgApply.
`FusedUpdateMixin` packs those entries' arguments; the class names them (UPDATE_KERNEL_PREFIX) and the observation size
they were compiled for (UPDATE_OBS_SIZE).  `Trainer` takes both paths when the config asks for both:

    registrar = EnvironmentRegistrar()
    registrar.add(env_backend=["cpu", "hip"], cuda_env_src_path=SOURCE)(RendezvousUpdate)
    wrapper = EnvWrapper(env_name="RendezvousUpdate", env_config={...}, num_envs=E, env_backend="hip",
                         env_registrar=registrar)
    config["trainer"]["fused_rollout_policy"] = "all"      # and a [32, 32] or [64, 64] fully connected model
    config["trainer"]["fused_update"] = "all"              # A2C / PPO, float32, no normalisations
    trainer = Trainer(env_wrapper=wrapper, config=config, ...)
    # trainer.rollout_path == "one launch", trainer.update_path == {policy: "kernels"}

Without `fused_update: "all"` the update runs in framework ops, as RendezvousPolicy's does; a shape the kernels do not
serve logs its reason once and stays there too.
"""
import importlib.util
import os
import sys

from warp_drive_amd.utils.custom_tick import FusedUpdateMixin

_HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(_HERE, "rendezvous_update.hip")


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


class RendezvousUpdate(FusedUpdateMixin, _rendezvous.Rendezvous):
    name = "RendezvousUpdate"

    TICK_KERNEL = "HipRendezvousUpdateTick"
    TICK_STEP_ARGS = _rendezvous._STEP_ARGS  # the Tick and Rollout entries' leading parameters are the Step entry's
    ROLLOUT_KERNEL = "HipRendezvousUpdateRollout_H{width}"
    ROLLOUT_MAX_THREADS = {32: 1024, 64: 512}  # the entries' __launch_bounds__ in rendezvous_update.hip
    UPDATE_KERNEL_PREFIX = "HipRendezvousUpdatePg"  # WD_PG_UPDATE_ENTRIES(RendezvousUpdate, 5)
    UPDATE_OBS_SIZE = 5
