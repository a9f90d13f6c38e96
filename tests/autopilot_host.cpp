// autopilot_host.cpp — csrc/zs_autopilot.hpp's rule functions on the host (tests/test_autopilot_plan.py builds this with
// AddressSanitizer and UBSan and runs it as a program): the triples of recorded states, decided with the key and the
// rule functions the kernel uses, for the test to compare with the fixtures' triples.
//
// Input (a text file of integers, argv[1]): the number of cases, then per case
//   W H A P E O, E x {present x y weapon rank}, O x {x y present}, A x {policy code}
// Output: per case one line of A triples; a row of code 0 is not written and prints as -9 -9 -9.
#include <cstdio>
#include <vector>

#include "zs_autopilot.hpp"

struct Ent {
    int present, x, y, weapon, rank;
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
        int W, H, A, P, E, O;
        if (!(rd(f, &W) && rd(f, &H) && rd(f, &A) && rd(f, &P) && rd(f, &E) && rd(f, &O))) return 2;
        if (E < A + P || A < 1 || W < 1 || H < 1 || O < 0) return 3;
        std::vector<Ent> ent(E);
        std::vector<Obst> ob(O);
        std::vector<int> code(A);
        for (auto& e : ent)
            if (!(rd(f, &e.present) && rd(f, &e.x) && rd(f, &e.y) && rd(f, &e.weapon) && rd(f, &e.rank))) return 2;
        for (auto& o : ob)
            if (!(rd(f, &o.x) && rd(f, &o.y) && rd(f, &o.present))) return 2;
        for (auto& k : code)
            if (!rd(f, &k)) return 2;
        const int np = A + P;
        for (int a = 0; a < A; a++) {
            PilotTriple t = pilot_triple(-9, -9, -9);
            if (code[a] != ZS_PILOT_NONE) {
                const int ax = ent[a].x, ay = ent[a].y;
                uint64_t key = ZS_PILOT_NO_KEY;
                int z = -1;
                for (int s = np; s < E; s++) {
                    if (!ent[s].present) continue;
                    const uint64_t k2 = pilot_key(pilot_d2(ent[s].x - ax, ent[s].y - ay), (uint32_t)ent[s].rank);
                    if (k2 < key) {
                        key = k2;
                        z = s;
                    }
                }
                bool chase, bad;
                t = pilot_simple(code[a], ent[a].present != 0, key, pilot_weapon_r2(ent[a].weapon), &chase, &bad);
                if (chase) {
                    const int k = pilot_best_dir(ax, ay, ent[z].x, ent[z].y);
                    const int bx = ax + pilot_adj_dx(k), by = ay + pilot_adj_dy(k);
                    int cell = PILOT_CELL_FREE;
                    if (bx >= 0 && bx < W && by >= 0 && by < H) {
                        for (const auto& o : ob)
                            if (o.x == bx && o.y == by && o.present) cell = PILOT_CELL_OTHER;
                        for (int s = 0; s < E && cell == PILOT_CELL_FREE; s++)
                            if (ent[s].present && ent[s].x == bx && ent[s].y == by) cell = s < np ? PILOT_CELL_PLAYER : PILOT_CELL_OTHER;
                    }
                    t = pilot_chase(k, cell);
                }
            }
            printf("%s%d %d %d", a ? " " : "", t.kind, t.dx, t.dy);
        }
        printf("\n");
    }
    fclose(f);
    return 0;
}
