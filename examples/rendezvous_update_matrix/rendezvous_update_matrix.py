"""RendezvousUpdateMatrix: RendezvousUpdate (examples/rendezvous_update/) whose update launches its gradients ON THE
FLOAT32 MATRIX CORES (docs/custom_environments.md, "The update as kernels").

The device source next to this file includes rendezvous_update.hip as it is and adds ONE line,

    WD_PG_UPDATE_MX_ENTRIES(RendezvousUpdate, 5)     // include/wd_env_update_matrix.h; the arguments of WD_PG_UPDATE_ENTRIES

which defines HipRendezvousUpdatePgGradientsMx_H32 / _H64 next to the six update entries.  `FusedUpdateMixin` finds them by
UPDATE_KERNEL_PREFIX; `Trainer` launches them when the config asks:

    config["trainer"]["fused_rollout_policy"] = "all"
    config["trainer"]["fused_update"] = "all"
    config["trainer"]["fused_update_gradients"] = "matrix"
    # trainer.update_path == {policy: "kernels"}, trainer.update_gradients_path == {policy: "matrix"}

Without the last key the gradient launch is the "lanes" entry, as RendezvousUpdate's; an env whose code object lacks the
Mx entries (RendezvousUpdate itself) logs one line under that key and keeps its "lanes" entries.
"""
import importlib.util
import os
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(_HERE, "rendezvous_update_matrix.hip")


def _parent_module():
    """examples/rendezvous_update/rendezvous_update.py, imported by path (the examples are not a package)"""
    name = "rendezvous_update_example"
    if name not in sys.modules:
        path = os.path.join(os.path.dirname(_HERE), "rendezvous_update", "rendezvous_update.py")
        spec = importlib.util.spec_from_file_location(name, path)
        module = importlib.util.module_from_spec(spec)
        sys.modules[name] = module
        spec.loader.exec_module(module)
    return sys.modules[name]


class RendezvousUpdateMatrix(_parent_module().RendezvousUpdate):
    name = "RendezvousUpdateMatrix"

    def initialize_step_function_context(self, cuda_data_manager, cuda_function_manager, cuda_step_function_feed,
                                         step_function_name):
        # the entries are the included source's: HipRendezvousUpdateStep, not Hip<this class's name>Step
        return super().initialize_step_function_context(cuda_data_manager, cuda_function_manager, cuda_step_function_feed,
                                                        "HipRendezvousUpdateStep")
