// UpdateProbeF32: test-only device source for the update kit of include/wd_env_update.h at its LARGEST observation size
// (F = 32: eight float4s per row of W0, no tail, no pad column).  Compiled only -- the build test reads its registers,
// scratch and LDS from the code object -- never launched.
// The LDS sizes as literals; tests/test_custom_env_update_build.py holds the host's formulas to the same numbers.
#include "wd_env_update.h"

static_assert(wd_pg_values_lds_floats(32, 32) == 2412 && wd_pg_values_lds_floats(64, 32) == 6860, "the network in LDS");
static_assert(wd_pg_gradients_lds_floats(32, 32) == 16800 && wd_pg_gradients_lds_floats(64, 32) == 29696, "... and the tile");
static_assert(4 * wd_pg_gradients_lds_floats(64, 32) <= 160 * 1024, "the largest shape fits the LDS of a compute unit");

WD_PG_UPDATE_ENTRIES(UpdateProbeF32, 32)
