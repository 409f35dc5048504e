// UpdateMatrixProbeF32: test-only device source for the matrix-core gradient launch of include/wd_env_update_matrix.h at
// F = 32: the largest observation size: sixteen first-layer steps, the MFMA dW0 with every lane supplying an input.
// The kit's six entries and the two Mx entries, nothing else.  The LDS sizes as literals;
// tests/test_custom_env_update_matrix_build.py holds the host's formula to the same numbers.
#include "wd_env_update.h"
#include "wd_env_update_matrix.h"

static_assert(wd_pg_gradients_mx_lds_floats(32, 32) == 17644 && wd_pg_gradients_mx_lds_floats(64, 32) == 37196, "the LDS");
WD_PG_UPDATE_ENTRIES(UpdateMatrixProbeF32, 32)
WD_PG_UPDATE_MX_ENTRIES(UpdateMatrixProbeF32, 32)
