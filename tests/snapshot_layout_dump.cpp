// Host program of tests/test_snapshot_layout.py: the snapshot record and fingerprint of
// libzombsole_amd/csrc/zs_snapshot.hpp, compiled with the host compiler.  One JSON line per input line:
//   "L E O DW OW A"  ->  the record's section offsets, "pad", "rec_bytes", and the header's constants
//   "F num_envs obs_dtype lanes_per_env W H rules reward_mode max_episode_steps initial_zombies minimum_zombies
//      nA nP nO nObj nPS nZS  obstacle_xy[2 nO] obstacle_kind[nO] player_spawn_xy[2 nPS] zombie_spawn_xy[2 nZS]
//      objective_xy[2 nObj] agent_weapons[nA] bot_types[nP]"  ->  {"fp_lo", "fp_hi"}: snapshot_fingerprint()
#include <stdio.h>

#include <vector>

#include "zs_snapshot.hpp"

static std::vector<int32_t> ints(int n) {
    std::vector<int32_t> v(n > 0 ? n : 0);
    for (auto& x : v)
        if (scanf("%d", &x) != 1) x = 0;
    return v;
}

int main(void) {
    static const char* names[SNAP_NSEC] = {"ring", "dead", "obst_hp", "obst_present", "obst_nonpos", "pos", "life", "serial", "scal",
                                           "hp_dirty", "dead_dirty", "rngst", "prev_life", "weapon", "present", "order", "listed"};
    char kind;
    while (scanf(" %c", &kind) == 1) {
        if (kind == 'L') {
            int E, O, DW, OW, A;
            if (scanf("%d %d %d %d %d", &E, &O, &DW, &OW, &A) != 5) return 1;
            const SnapshotLayout L = snapshot_layout(E, O, DW, OW, A);
            printf("{");
            for (int s = 0; s < SNAP_NSEC; s++) printf("\"%s\": %d, ", names[s], L.off[s]);
            printf("\"pad\": %d, \"rec_bytes\": %d, \"nscal\": %d, \"ring_words\": %d, \"nsec\": %d}\n", L.off[SNAP_NSEC],
                   L.rec_bytes, ZS_SNAP_NSCAL, ZS_SNAP_RING, SNAP_NSEC);
        } else if (kind == 'F') {
            const std::vector<int32_t> h = ints(16);
            const int nA = h[10], nP = h[11], nO = h[12], nObj = h[13], nPS = h[14], nZS = h[15];
            const std::vector<int32_t> oxy = ints(2 * nO), okind = ints(nO), ps = ints(2 * nPS), zs = ints(2 * nZS),
                                       obj = ints(2 * nObj), aw = ints(nA), bt = ints(nP);
            const std::vector<uint8_t> kinds(okind.begin(), okind.end());
            zs_config c = {};
            c.num_envs = h[0];
            c.obs_dtype = h[1];
            c.lanes_per_env = h[2];
            c.map.width = h[3];
            c.map.height = h[4];
            c.rules = h[5];
            c.reward_mode = h[6];
            c.max_episode_steps = h[7];
            c.initial_zombies = h[8];
            c.minimum_zombies = h[9];
            c.num_agents = nA;
            c.num_bots = nP;
            c.map.n_obstacles = nO;
            c.map.n_objectives = nObj;
            c.map.n_player_spawns = nPS;
            c.map.n_zombie_spawns = nZS;
            c.map.obstacle_xy = oxy.data();
            c.map.obstacle_kind = kinds.data();
            c.map.player_spawn_xy = ps.data();
            c.map.zombie_spawn_xy = zs.data();
            c.map.objective_xy = obj.data();
            c.agent_weapons = aw.data();
            c.bot_types = bt.data();
            const uint64_t fp = snapshot_fingerprint(&c);
            printf("{\"fp_lo\": %u, \"fp_hi\": %u}\n", (unsigned)(uint32_t)fp, (unsigned)(uint32_t)(fp >> 32));
        } else {
            return 1;
        }
    }
    return 0;
}
