// Host program of tests/test_step_plan.py: reads lines of integers from stdin and prints one JSON line for each.
//   P N W H E A DW ncand nps nzs minimum_zombies lanes_per_env obs_bytes, then the zs_launch fields in the
//     header's order (22 integers): the step plan (libzombsole_amd/csrc/zs_step_plan.hpp) of the pair
//   I fused ne E DW rw_cap cand_cap lists_cap A ncand obs_bytes: the step launch's LDS image of these arguments,
//     tick_layout(...).bytes and reset_lds_bytes(...), and the fused launch's (the larger of the two)
#include <stdio.h>
#include <string.h>

#include "zs_step_plan.hpp"

int main(void) {
    const int n_launch = 22;
    static_assert(sizeof(zs_launch) == (22 + 10) * sizeof(int32_t), "zs_launch: 22 switches and 10 reserved words");
    char mode[4];
    while (scanf("%3s", mode) == 1) {
        int v[12];
        const int nv = mode[0] == 'I' ? 10 : 12;
        for (int i = 0; i < nv; i++)
            if (scanf("%d", &v[i]) != 1) return 2;
        if (mode[0] == 'I') {
            const int tick = tick_layout(v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[9]).bytes;
            const int reset = reset_lds_bytes(v[2], v[3], v[8], v[6], v[9]);
            printf("{\"tick\": %d, \"reset\": %d, \"bytes\": %d}\n", tick, reset, v[0] && reset > tick ? reset : tick);
            continue;
        }
        zs_launch ov;
        memset(&ov, 0, sizeof(ov));
        int32_t* f = (int32_t*)&ov;
        for (int i = 0; i < n_launch; i++) {
            int x;
            if (scanf("%d", &x) != 1) return 2;
            f[i] = x;
        }
        const StepShape s = {v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], v[9], v[10], v[11]};
        const StepPlan p = step_plan(s, ov);
        if (p.error) {
            printf("{\"error\": \"%s\", \"defer_respawn\": %d}\n", p.error, p.defer_respawn);
            continue;
        }
        printf("{\"G\": %d, \"fused\": %d, \"tick_waves\": %d, \"lds\": %d, \"resident\": %d, \"want\": %d, \"rw_cap\": %d, "
               "\"rw_step\": %d, \"cand_cap\": %d, \"lists_cap\": %d, \"rlists_cap\": %d, \"reset_lds\": %d, \"side_stream\": %d, "
               "\"n_reset\": %d, \"reset_grid_list\": %d, \"reset_grid_mask\": %d, \"respawn_grid\": %d, \"defer_respawn\": %d}\n",
               p.G, p.fused, p.tick_waves, p.lds, p.resident, p.want, p.rw_cap, p.rw_step, p.cand_cap, p.lists_cap, p.rlists_cap,
               p.reset_lds, p.side_stream, p.n_reset, p.reset_grid_list, p.reset_grid_mask, p.respawn_grid, p.defer_respawn);
    }
    return 0;
}
