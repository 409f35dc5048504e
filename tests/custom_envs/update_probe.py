"""UpdateProbe: the test-only device sources of the update kit (include/wd_env_update.h) at observation sizes the worked
example does not have.  No environment class: a unit is the macro's six entries, loaded as a function manager's custom
code object and launched through training/pg_update_custom_kernels.py::PgCustomUpdateKernels.

    UpdateProbeF1    update_probe_f1.hip     F = 1    no whole float4 in a row of W0, three pad columns
    UpdateProbe      update_probe.hip        F = 7    one float4 and a tail of three
    UpdateProbeF32   update_probe_f32.hip    F = 32   the largest: compiled only, never launched

(one source per size: no single first-use compile dominates a test)"""
import os

_HERE = os.path.dirname(os.path.abspath(__file__))

# unit name -> (device source, F, entry prefix)
UNITS = {"UpdateProbeF1": (os.path.join(_HERE, "update_probe_f1.hip"), 1, "HipUpdateProbeF1Pg"),
         "UpdateProbe": (os.path.join(_HERE, "update_probe.hip"), 7, "HipUpdateProbePg"),
         "UpdateProbeF32": (os.path.join(_HERE, "update_probe_f32.hip"), 32, "HipUpdateProbeF32Pg")}
RUN = {1: "UpdateProbeF1", 7: "UpdateProbe"}   # observation size -> the unit the GPU test launches
# the LDS sizes the sources assert, in floats: {(H, F): (values, gradients)}
LDS_FLOATS = {(32, 1): (1516, 11812), (64, 1): (5068, 23812), (32, 7): (1644, 12732), (64, 7): (5324, 24860),
              (32, 32): (2412, 16800), (64, 32): (6860, 29696)}
