// Host program of tests/test_obs_plan.py: reads rows of integers from stdin, one (shape, overrides) pair
// per line, and prints the observation plan (libzombsole_amd/csrc/zs_obs_plan.hpp) of each as a JSON line.
//   row: refuse N W H O OW DW E A scope enc obs_w dtype reward_mode opad_n rank_order defer_respawn
//        then the zs_launch fields in the header's order (22 integers)
// refuse = 1: lds_ok refuses every request for more dynamic LDS.
#include <stdio.h>
#include <string.h>

#include "zs_obs_plan.hpp"

static bool lds_always(int, int, int, int, void*) { return true; }
static bool lds_never(int, int, int, int, void*) { return false; }

static void print_kernel(const char* name, const ObsKernel& k, int n_envs) {
    printf("\"%s\": {\"kind\": %d, \"name\": \"%s\", \"encoders\": \"%s\", \"nobs\": %d, \"patched\": %d, \"grid\": %u, "
           "\"block\": %d, \"lds\": %d, \"stat\": %d, \"us\": %d, \"win\": %d, \"hp_cap\": %d, \"img_bytes\": %d, "
           "\"envs_per_wg\": %d}",
           name, k.kind, obs_kernel_name(k.kind), obs_encoders_name(k), k.nobs, k.patched, obs_grid(k, n_envs), k.block,
           k.lds, k.stat, k.us, k.L.win, k.L.hp_cap, k.L.bytes, k.envs_per_wg);
}

int main(void) {
    const int n_launch = 22;
    static_assert(sizeof(zs_launch) == (22 + 10) * sizeof(int32_t), "zs_launch: 22 switches and 10 reserved words");
    for (;;) {
        int refuse, v[16];
        if (scanf("%d", &refuse) != 1) break;
        for (int i = 0; i < 16; i++)
            if (scanf("%d", &v[i]) != 1) return 2;
        zs_launch ov;
        memset(&ov, 0, sizeof(ov));
        int32_t* f = (int32_t*)&ov;
        for (int i = 0; i < n_launch; i++) {
            int x;
            if (scanf("%d", &x) != 1) return 2;
            f[i] = x;
        }
        const ObsShape s = {v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], v[9], v[10], v[11], v[12], v[13], v[14], v[15]};
        const ObsPlan p = obs_plan(s, ov, refuse ? lds_never : lds_always, nullptr);
        if (p.error) {
            printf("{\"error\": \"%s\"}\n", p.error);
            continue;
        }
        printf("{");
        print_kernel("full", p.full, s.N);
        printf(", ");
        print_kernel("masked", p.masked, s.N);
        printf(", \"obs_stat\": %d, \"fobs\": %d, \"step_img_bytes\": %d, \"step_win\": %d, \"step_hp_cap\": %d}\n", p.obs_stat, p.fobs,
               p.step_img.bytes, p.step_img.win, p.step_img.hp_cap);
    }
    return 0;
}
