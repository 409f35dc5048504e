"""RendezvousFused: the Rendezvous example with a FUSED TICK (docs/custom_environments.md, "A fused tick").

The env is examples/rendezvous/rendezvous.py's, unchanged: same host step, same arrays, same step arguments.  What is
new is the device source next to this file: rendezvous_fused.hip writes the step once as a `__device__` function and
wraps it twice -- `HipRendezvousFusedStep` (the plain step) and `HipRendezvousFusedTick`, built with
include/wd_env_tick.h: the action draw, the step and the restart of finished replicas in one launch, for as many ticks
as its last argument says.  `FusedTickMixin` packs that entry's arguments, and `RolloutEngine` / `Trainer` then drive the
env with one launch per tick, and a `run(n)` with one launch for n ticks:

    registrar = EnvironmentRegistrar()
    registrar.add(env_backend=["cpu", "hip"], cuda_env_src_path=SOURCE)(RendezvousFused)
    wrapper = EnvWrapper(env_name="RendezvousFused", env_config={...}, num_envs=E, env_backend="hip",
                         env_registrar=registrar)
    engine = RolloutEngine(wrapper, sampler)      # engine.fused, engine.entry_names == ["HipRendezvousFusedTick"]
"""
import importlib.util
import os
import sys

from warp_drive_amd.utils.custom_tick import FusedTickMixin

_HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(_HERE, "rendezvous_fused.hip")


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


class RendezvousFused(FusedTickMixin, _rendezvous.Rendezvous):
    name = "RendezvousFused"

    TICK_KERNEL = "HipRendezvousFusedTick"
    TICK_STEP_ARGS = _rendezvous._STEP_ARGS  # the Tick entry's leading parameters are the Step entry's
