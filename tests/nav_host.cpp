// nav_host.cpp — csrc/zs_nav.hpp's rule functions on the host (tests/test_nav_plan.py builds this plain and with
// AddressSanitizer and UBSan and runs it as a program): the bit-row level loop over row bitmaps, word by word as the
// kernel's lanes run it, for the test to compare with libzombsole_amd/nav.py; and nav_plan() for a table of shapes.
//
//   nav_host cases FILE   FILE: the number of cases, then per case
//                           W H A P E O nobj fields max_dist, E x {present x y}, O x {x y present}, nobj x {x y}
//                         output per case: one line of A * F * 8 int16 words, then per field one line of H * W uint16
//   nav_host plan W H A [W H A ...]
//                         output per triple: ok ww nw nq env_bytes envs_per_wg block lds_bytes
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "zs_nav.hpp"

struct Ent {
    int present, x, y;
};
struct Obst {
    int x, y, present;
};

static bool rd(FILE* f, int* v) { return fscanf(f, "%d", v) == 1; }

// one field of one env: the distances of every cell, by the level loop
static std::vector<uint16_t> run_field(int W, int H, int bit, int max_dist, int A, int P, const std::vector<Ent>& ent,
                                       const std::vector<Obst>& ob, const std::vector<int>& objx, const std::vector<int>& objy) {
    const int ww = nav_ww(W), nw = H * ww;
    std::vector<uint32_t> fre(nw), vis(nw, 0), fr[2] = {std::vector<uint32_t>(nw, 0), std::vector<uint32_t>(nw, 0)};
    for (int i = 0; i < nw; i++) fre[i] = nav_row_mask(i % ww, W);
    for (const auto& o : ob)
        if (o.present) fre[nav_word(o.x, o.y, ww)] &= ~nav_bit(o.x);
    auto source = [&](int x, int y) {
        if (x < 0 || x >= W || y < 0 || y >= H) return;
        if (nav_source_ok(fre[nav_word(x, y, ww)], x)) fr[0][nav_word(x, y, ww)] |= nav_bit(x);
    };
    if (bit == 0)
        for (size_t i = 0; i < objx.size(); i++) source(objx[i], objy[i]);
    else
        for (size_t s = A + P; s < ent.size(); s++)
            if (ent[s].present) source(ent[s].x, ent[s].y);
    std::vector<uint16_t> dist((size_t)W * H, ZS_NAV_UNREACHED);
    auto record = [&](int i, uint32_t m, int level) {
        for (; m; m &= m - 1) dist[(size_t)(i / ww) * W + 32 * (i % ww) + __builtin_ctz(m)] = (uint16_t)level;
    };
    for (int i = 0; i < nw; i++) {
        vis[i] = fr[0][i];
        record(i, fr[0][i], 0);
    }
    const int cap = nav_trip_cap(max_dist, W, H);
    int cur = 0;
    for (int level = 1; level <= cap; level++) {
        uint32_t grew = 0;
        const std::vector<uint32_t>& f = fr[cur];
        std::vector<uint32_t>& nx = fr[cur ^ 1];
        for (int i = 0; i < nw; i++) {
            const int r = i / ww, w = i % ww;
            const uint32_t m = nav_step_word(f[i], w > 0 ? f[i - 1] : 0u, w + 1 < ww ? f[i + 1] : 0u, r > 0 ? f[i - ww] : 0u,
                                             r + 1 < H ? f[i + ww] : 0u) & fre[i] & ~vis[i];
            nx[i] = m;
            vis[i] |= m;
            grew |= m;
            record(i, m, level);
        }
        if (!grew) break;
        cur ^= 1;
    }
    return dist;
}

static int run_cases(const char* path) {
    FILE* f = fopen(path, "r");
    if (!f) return 2;
    int ncases = 0;
    if (!rd(f, &ncases)) return 2;
    for (int c = 0; c < ncases; c++) {
        int W, H, A, P, E, O, nobj, fields, max_dist;
        if (!(rd(f, &W) && rd(f, &H) && rd(f, &A) && rd(f, &P) && rd(f, &E) && rd(f, &O) && rd(f, &nobj) && rd(f, &fields) &&
              rd(f, &max_dist)))
            return 2;
        if (!nav_fields_ok(fields) || !nav_max_dist_ok(max_dist) || E < A + P || A < 1 || W < 1 || H < 1) return 3;
        std::vector<Ent> ent(E);
        std::vector<Obst> ob(O);
        std::vector<int> objx(nobj), objy(nobj);
        for (auto& e : ent)
            if (!(rd(f, &e.present) && rd(f, &e.x) && rd(f, &e.y))) return 2;
        for (auto& o : ob)
            if (!(rd(f, &o.x) && rd(f, &o.y) && rd(f, &o.present))) return 2;
        for (int i = 0; i < nobj; i++)
            if (!(rd(f, &objx[i]) && rd(f, &objy[i]))) return 2;
        const int F = nav_nfields(fields);
        std::vector<std::vector<uint16_t>> dist;
        for (int i = 0; i < F; i++) dist.push_back(run_field(W, H, nav_field_bit(fields, i), max_dist, A, P, ent, ob, objx, objy));
        std::vector<uint64_t> out((size_t)A * F * 2, 0x5a5a5a5a5a5a5a5aull);  // every word must be written
        for (int a = 0; a < A; a++)
            for (int i = 0; i < F; i++) {
                auto at = [&](int x, int y) {
                    if (x < 0 || x >= W || y < 0 || y >= H) return -1;
                    const uint16_t v = dist[i][(size_t)y * W + x];
                    return v == ZS_NAV_UNREACHED ? -1 : (int)v;
                };
                int d[4];
                for (int k = 0; k < 4; k++) d[k] = at(ent[a].x + nav_dir_dx(k), ent[a].y + nav_dir_dy(k));
                nav_row(ent[a].present != 0, ent[a].present ? at(ent[a].x, ent[a].y) : 0, d, &out[((size_t)a * F + i) * 2]);
            }
        for (size_t i = 0; i < out.size(); i++) {
            int16_t w[4];
            std::memcpy(w, &out[i], 8);
            printf("%s%d %d %d %d", i ? " " : "", w[0], w[1], w[2], w[3]);
        }
        printf("\n");
        for (int i = 0; i < F; i++) {
            for (size_t j = 0; j < dist[i].size(); j++) printf("%s%u", j ? " " : "", (unsigned)dist[i][j]);
            printf("\n");
        }
    }
    fclose(f);
    return 0;
}

int main(int argc, char** argv) {
    if (argc >= 3 && !strcmp(argv[1], "cases")) return run_cases(argv[2]);
    if (argc >= 5 && !strcmp(argv[1], "plan")) {
        for (int i = 2; i + 2 < argc; i += 3) {
            const NavPlan p = nav_plan(atoi(argv[i]), atoi(argv[i + 1]), atoi(argv[i + 2]));
            printf("%d %d %d %d %d %d %d %d\n", p.ok, p.ww, p.nw, p.nq, p.env_bytes, p.envs_per_wg, p.block, p.lds_bytes);
        }
        return 0;
    }
    return 2;
}
