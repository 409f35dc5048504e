// UpdateProbe: test-only device source for the update kit of include/wd_env_update.h at an observation size that is no
// multiple of four (F = 7: one whole float4 and a tail of three per row of W0).  No environment: the six entries alone.
// The LDS sizes as literals; tests/test_custom_env_update_build.py holds the host's formulas to the same numbers.
#include "wd_env_update.h"

static_assert(wd_pg_values_lds_floats(32, 7) == 1644 && wd_pg_values_lds_floats(64, 7) == 5324, "the network in LDS");
static_assert(wd_pg_gradients_lds_floats(32, 7) == 12732 && wd_pg_gradients_lds_floats(64, 7) == 24860, "... and the tile");

WD_PG_UPDATE_ENTRIES(UpdateProbe, 7)
