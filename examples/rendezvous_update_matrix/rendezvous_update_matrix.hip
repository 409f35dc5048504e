// RendezvousUpdateMatrix: RendezvousUpdate (examples/rendezvous_update/) -- the whole training iteration as kernels -- with
// the update's gradient launch ON THE FLOAT32 MATRIX CORES as well (include/wd_env_update_matrix.h;
// docs/custom_environments.md, "The update as kernels").  The step, the tick, the rollout and the update's six entries are
// that example's source, included as it is (so the entries keep its names, HipRendezvousUpdate...); this file adds ONE
// line, the kit's second macro with the same two arguments, which defines HipRendezvousUpdatePgGradientsMx_H32 / _H64.
#include "../rendezvous_update/rendezvous_update.hip"
#include "wd_env_update_matrix.h"

WD_PG_UPDATE_MX_ENTRIES(RendezvousUpdate, 5)
