"""EvaluateProbe: a test-only custom environment for the one-launch evaluation of include/wd_env_evaluate.h with an EVEN
observation size (F = 2) and an action count chosen at run time.  The env is tests/custom_envs/policy_probe.py's --
observation (counter / L, agent parity), reward action + 1 (the reward sums show which actions the in-kernel policy handed
to the step), done at the time limit only -- on a source of its own that adds the Evaluate_H32 / _H64 entries."""
import os

from tests.custom_envs.policy_probe import PolicyProbe
from warp_drive_amd.utils.custom_tick import FusedEvaluateMixin

SOURCE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "evaluate_probe.hip")


class EvaluateProbe(FusedEvaluateMixin, PolicyProbe):
    name = "EvaluateProbe"
    TICK_KERNEL = "HipEvaluateProbeTick"
    ROLLOUT_KERNEL = "HipEvaluateProbeRollout_H{width}"
    EVALUATE_KERNEL = "HipEvaluateProbeEvaluate_H{width}"  # launch bounds: the Rollout entries' (ROLLOUT_MAX_THREADS)
