// Host program of tests/test_obs_state_layout.py: reads lines "E O DW OW obs_dtype obs_encoding" from stdin and
// prints, for each, the observation-state record (libzombsole_amd/csrc/zs_obs_state.hpp) as one JSON line, with
// the dtype obs_state_record_dtype() lays the record out for.  "flag_viewer": the header's ZS_FLAG_VIEWER.
#include <stdio.h>

#include "zs_obs_state.hpp"

int main(void) {
    int E, O, DW, OW, dtype, enc;
    while (scanf("%d %d %d %d %d %d", &E, &O, &DW, &OW, &dtype, &enc) == 6) {
        const int rd = obs_state_record_dtype(dtype, enc);
        const ObsStateLayout L = obs_state_layout(E, O, DW, OW, dtype);
        printf("{\"hp_dirty\": %d, \"dead_dirty\": %d, \"pos\": %d, \"life\": %d, \"dead\": %d, \"obst_present\": %d, "
               "\"obst_hp\": %d, \"weapon\": %d, \"present\": %d, \"pad\": %d, \"rec_bytes\": %d, \"hp_bytes\": %d, "
               "\"record_dtype\": %d, \"flag_viewer\": %u}\n",
               L.hp_dirty, L.dead_dirty, L.pos, L.life, L.dead, L.obst_present, L.obst_hp, L.weapon, L.present, L.pad,
               L.rec_bytes, L.hp_bytes, rd, ZS_FLAG_VIEWER);
    }
    return 0;
}
