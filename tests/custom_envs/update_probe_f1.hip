// UpdateProbeF1: test-only device source for the update kit of include/wd_env_update.h at the smallest observation size
// (F = 1: no whole float4 in a row of W0, a tail of one, three pad columns).  No environment: the six entries alone.
// The LDS sizes as literals; tests/test_custom_env_update_build.py holds the host's formulas to the same numbers.
#include "wd_env_update.h"

static_assert(wd_pg_values_lds_floats(32, 1) == 1516 && wd_pg_values_lds_floats(64, 1) == 5068, "the network in LDS");
static_assert(wd_pg_gradients_lds_floats(32, 1) == 11812 && wd_pg_gradients_lds_floats(64, 1) == 23812, "... and the tile");

WD_PG_UPDATE_ENTRIES(UpdateProbeF1, 1)
