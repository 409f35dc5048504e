"""The worked custom environment of examples/rendezvous/, loaded for the tests (it lives outside the package, so it is
imported by path), with a registrar that holds its device source."""
import importlib.util
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXAMPLE_DIR = os.path.join(ROOT, "examples", "rendezvous")
SOURCE = os.path.join(EXAMPLE_DIR, "rendezvous_step.hip")


def example_module():
    name = "rendezvous_example"
    if name not in sys.modules:
        spec = importlib.util.spec_from_file_location(name, os.path.join(EXAMPLE_DIR, "rendezvous.py"))
        module = importlib.util.module_from_spec(spec)
        sys.modules[name] = module
        spec.loader.exec_module(module)
    return sys.modules[name]


def host_run(config, num_envs, ticks, seed):
    """`num_envs` host replicas driven by the action stream the consistency checker draws from `seed` (its generator,
    its order: every replica of a tick, every agent of a replica), restarted when they finish, for `ticks` ticks.
    Returns (largest spread per tick and replica [ticks, num_envs], replicas that finished before the time limit,
    replicas that finished at it)."""
    import numpy as np

    from warp_drive_amd.env_cpu_gpu_consistency_checker import generate_random_actions

    envs = [example_module().Rendezvous(**config) for _ in range(num_envs)]
    for env in envs:
        env.reset()
    rng = np.random.RandomState(seed)
    maxima, early, timed = np.zeros((ticks, num_envs), dtype=np.int64), 0, 0
    for t in range(ticks):
        actions = generate_random_actions(envs[0], num_envs, rng)
        for e, env in enumerate(envs):
            done = env.step(actions[e])[2]["__all__"]
            maxima[t, e] = env.last_max_spread
            if done:
                early += env.timestep < env.episode_length
                timed += env.timestep == env.episode_length
                env.reset()
    return maxima, int(early), int(timed)


def spread_limit_for(config, num_envs, ticks, seed, percentile=10):
    """the spread limit of a checked run, chosen from the host env alone: the `percentile`-th percentile (rounded
    down) of the per-tick largest spread over a dry run of the same action stream with the limit off"""
    import numpy as np

    maxima, _, _ = host_run(dict(config, spread_limit=-1), num_envs, ticks, seed)
    return int(np.floor(np.percentile(maxima, percentile)))


def registrar_for(cls=None, source=SOURCE):
    """a fresh registrar with `cls` (default: the example's class) registered for both backends with its source"""
    from warp_drive_amd.utils.env_registrar import EnvironmentRegistrar

    registrar = EnvironmentRegistrar()
    registrar.add(env_backend=["cpu", "hip"], cuda_env_src_path=source)(cls or example_module().Rendezvous)
    return registrar
