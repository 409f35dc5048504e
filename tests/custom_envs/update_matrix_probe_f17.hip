// UpdateMatrixProbeF17: test-only device source for the matrix-core gradient launch of include/wd_env_update_matrix.h at
// F = 17: the MFMA dW0 at its smallest, with a pad row (F2 = 18) and fifteen lanes that supply zero.
// The kit's six entries and the two Mx entries, nothing else.  The LDS sizes as literals;
// tests/test_custom_env_update_matrix_build.py holds the host's formula to the same numbers.
#include "wd_env_update.h"
#include "wd_env_update_matrix.h"

static_assert(wd_pg_gradients_mx_lds_floats(32, 17) == 15180 && wd_pg_gradients_mx_lds_floats(64, 17) == 33836, "the LDS");
WD_PG_UPDATE_ENTRIES(UpdateMatrixProbeF17, 17)
WD_PG_UPDATE_MX_ENTRIES(UpdateMatrixProbeF17, 17)
