// entity_obs_host.cpp — csrc/zs_entity_obs.hpp's rule functions on the host (tests/test_entity_obs_model.py builds this
// with AddressSanitizer and UBSan and runs it as a program): the rows of hand-built and recorded states, encoded with
// the rank rule the kernel uses (a slot's rank in its class = the count of smaller keys), for the test to compare
// with libzombsole_amd/entity_obs.py's encode.
//
// Input (a text file of integers, argv[1]): the number of cases, then per case
//   W H A P E O nobj kz kp, E x {present x y life weapon}, O x {x y present}, nobj x {x y}
// Output: per case one line of A * ROW int16 words.
#include <cstdio>
#include <cstring>
#include <vector>

#include "zs_entity_obs.hpp"

struct Ent {
    int present, x, y, life, weapon;
};
struct Obst {
    int x, y, present;
};

static bool rd(FILE* f, int* v) { return fscanf(f, "%d", v) == 1; }

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return 2;
    int ncases = 0;
    if (!rd(f, &ncases)) return 2;
    for (int c = 0; c < ncases; c++) {
        int W, H, A, P, E, O, nobj, kz, kp;
        if (!(rd(f, &W) && rd(f, &H) && rd(f, &A) && rd(f, &P) && rd(f, &E) && rd(f, &O) && rd(f, &nobj) && rd(f, &kz) && rd(f, &kp)))
            return 2;
        if (!ent_k_ok(kz, kp) || E < A + P || A < 1 || W < 1 || H < 1) return 3;
        std::vector<Ent> ent(E);
        std::vector<Obst> ob(O);
        std::vector<int> objx(nobj), objy(nobj);
        for (auto& e : ent)
            if (!(rd(f, &e.present) && rd(f, &e.x) && rd(f, &e.y) && rd(f, &e.life) && rd(f, &e.weapon))) return 2;
        for (auto& o : ob)
            if (!(rd(f, &o.x) && rd(f, &o.y) && rd(f, &o.present))) return 2;
        for (int i = 0; i < nobj; i++)
            if (!(rd(f, &objx[i]) && rd(f, &objy[i]))) return 2;
        const EntLayout L = ent_layout(kz, kp);
        const int rowq = L.row_words / 4, np = A + P;
        std::vector<uint64_t> out((size_t)A * rowq, 0x5a5a5a5a5a5a5a5aull);  // every word must be written
        int nz = 0, npl = 0;
        for (int s = 0; s < E; s++) (s >= np ? nz : npl) += ent[s].present != 0;
        auto blocked = [&](int cx, int cy) {
            for (const auto& o : ob)
                if (o.x == cx && o.y == cy && o.present) return true;
            return false;
        };
        for (int a = 0; a < A; a++) {
            uint64_t* r = out.data() + (size_t)a * rowq;
            if (!ent[a].present) {
                for (int i = 0; i < rowq; i++) r[i] = 0;
                continue;
            }
            const int ax = ent[a].x, ay = ent[a].y, r2 = ent_weapon_r2(ent[a].weapon);
            std::vector<int32_t> sd(E);
            for (int s = 0; s < E; s++)
                sd[s] = ent[s].present && s != a ? ent_d2(ent[s].x - ax, ent[s].y - ay) : ZS_ENT_ABSENT;
            for (int s = 0; s < E; s++) {
                if (sd[s] == ZS_ENT_ABSENT) continue;
                const bool player = s < np;
                const int lo = player ? 0 : np, hi = player ? np : E, K = player ? kp : kz;
                int rank = 0;
                for (int t = lo; t < hi; t++) rank += ent_key_less(sd[t], t, sd[s], s) ? 1 : 0;
                if (rank < K)
                    r[((player ? L.players : L.zombies) >> 2) + rank] =
                        ent_slot_row(ent[s].x - ax, ent[s].y - ay, ent[s].life, player, s < A, ent[s].weapon, r2);
            }
            for (int i = nz; i < kz; i++) r[(L.zombies >> 2) + i] = 0;
            for (int i = npl - 1; i < kp; i++) r[(L.players >> 2) + i] = 0;
            uint64_t key = ~0ull;
            for (int i = 0; i < nobj; i++) {
                const uint64_t k2 = ent_obj_key(ent_d2(objx[i] - ax, objy[i] - ay), i);
                key = k2 < key ? k2 : key;
            }
            r[L.self >> 2] = ent_pack4(1, ax, ay, ent_sat16(ent[a].life));
            r[(L.self >> 2) + 1] = ent_pack4(ent[a].weapon, r2, ent_sat16(nz), ent_sat16(npl - 1));
            uint64_t o = 0;
            if (nobj > 0) {
                const int i = (int)(uint32_t)key;
                o = ent_pack4(objx[i] - ax, objy[i] - ay, ZS_ENT_VALID | ((key >> 32) == 0 ? ZS_ENT_ON_OBJECTIVE : 0), ent_sat16(nobj));
            }
            r[L.objective >> 2] = o;
            int n[4];
            for (int k = 0; k < 4; k++) n[k] = ent_ray(ax, ay, k, W, H, blocked);
            r[L.rays >> 2] = ent_pack4(n[0], n[1], n[2], n[3]);
        }
        for (size_t i = 0; i < out.size(); i++) {
            int16_t w[4];
            std::memcpy(w, &out[i], 8);
            printf("%s%d %d %d %d", i ? " " : "", w[0], w[1], w[2], w[3]);
        }
        printf("\n");
    }
    fclose(f);
    return 0;
}
