// UpdateMatrixProbeF1: test-only device source for the matrix-core gradient launch of include/wd_env_update_matrix.h at
// F = 1: ONE first-layer step whose upper lane half is all pad (F2 = 2); the vector dW0 with one input.
// The kit's six entries and the two Mx entries, nothing else.  The LDS sizes as literals;
// tests/test_custom_env_update_matrix_build.py holds the host's formula to the same numbers.
#include "wd_env_update.h"
#include "wd_env_update_matrix.h"

static_assert(wd_pg_gradients_mx_lds_floats(32, 1) == 12364 && wd_pg_gradients_mx_lds_floats(64, 1) == 29996, "the LDS");
WD_PG_UPDATE_ENTRIES(UpdateMatrixProbeF1, 1)
WD_PG_UPDATE_MX_ENTRIES(UpdateMatrixProbeF1, 1)
