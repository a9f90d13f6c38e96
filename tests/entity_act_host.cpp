// entity_act_host.cpp — csrc/zs_entity_act.hpp's rule functions on the host (tests/test_entity_act_model.py builds this
// with AddressSanitizer and UBSan and runs it as a program): the table of hand-built and generated states, put together
// the way the kernels do (a slot's rank in its class = the count of smaller keys; the fixed entries from the
// predicates of the agent's surroundings), for the test to compare with libzombsole_amd/entity_act.py.
//
// Input (a text file of integers, argv[1]): the number of cases, then per case
//   W H A P E O kz kp Q, E x {present x y life weapon}, O x {x y present}, Q x {kind dx dy}
// Output: per case and agent one line: NID x {kind dx dy bit} (decode and mask of every id), NID ids (encode of every
// id's decoded triple), Q ids (encode of the case's query triples).
#include <cstdio>
#include <vector>

#include "zs_entity_act.hpp"

struct Ent {
    int present, x, y, life, weapon;
};
struct Obst {
    int x, y, present;
};

static bool rd(FILE* f, int* v) { return fscanf(f, "%d", v) == 1; }

struct World {
    int W, H, A, P, kz, kp;
    std::vector<Ent> ent;
    std::vector<Obst> ob;
    int np() const { return A + P; }
    int E() const { return (int)ent.size(); }
    int32_t d2(int a, int s) const {
        return ent[s].present && s != a ? ent_d2(ent[s].x - ent[a].x, ent[s].y - ent[a].y) : ZS_ENT_ABSENT;
    }
    // the rank of present slot s != a in its class, seen from agent a
    int rank(int a, int s) const {
        const bool player = s < np();
        int r = 0;
        for (int t = player ? 0 : np(); t < (player ? np() : E()); t++) r += ent_key_less(d2(a, t), t, d2(a, s), s) ? 1 : 0;
        return r;
    }
    // the slot of rank j in the class, -1 when the class has fewer
    int slot_of(int a, bool player, int j) const {
        for (int s = player ? 0 : np(); s < (player ? np() : E()); s++)
            if (d2(a, s) != ZS_ENT_ABSENT && rank(a, s) == j) return s;
        return -1;
    }
    EactNear near(int a) const {
        EactNear w = {0, 0, 0, 0, false, false, false};
        const int r2 = ent_weapon_r2(ent[a].weapon);
        for (int k = 0; k < 4; k++) {
            const int cx = ent[a].x + ent_dir_dx(k), cy = ent[a].y + ent_dir_dy(k);
            if (cx < 0 || cx >= W || cy < 0 || cy >= H) w.out |= 1u << k;
            for (const auto& o : ob)
                if (o.present && o.x == cx && o.y == cy) w.obst |= 1u << k;
            for (int s = 0; s < E(); s++)
                if (s != a && ent[s].present && ent[s].x == cx && ent[s].y == cy) {
                    w.thing |= 1u << k;
                    if (s < np()) w.player |= 1u << k;
                }
        }
        for (int s = 0; s < E(); s++) {
            const int32_t dd = d2(a, s);
            if (dd == ZS_ENT_ABSENT) continue;
            if (s >= np()) {
                w.zombie_in_range = w.zombie_in_range || dd <= r2;
            } else {
                w.other_player = true;
                w.other_in_heal = w.other_in_heal || dd <= ZS_ENT_HEAL_R2;
            }
        }
        return w;
    }
    EactTriple decode(int a, int id, int* bit) const {
        *bit = 0;
        int k;
        const int cls = eact_class(id, kz, kp, &k);
        if (!ent[a].present || cls == EACT_BAD) return eact_triple(ZS_ACT_IDLE, 0, 0);
        if (cls != EACT_ZOMBIE_ROW && cls != EACT_PLAYER_ROW) {
            *bit = eact_fixed_mask(id, near(a));
            return eact_fixed_triple(id);
        }
        const bool player = cls == EACT_PLAYER_ROW;
        const int s = slot_of(a, player, k);
        if (s < 0) return eact_triple(ZS_ACT_IDLE, 0, 0);
        *bit = eact_row_mask(player, d2(a, s), ent_weapon_r2(ent[a].weapon));
        return eact_row_triple(player, ent[s].x - ent[a].x, ent[s].y - ent[a].y);
    }
    int encode(int a, const EactTriple& t) const {
        if (!ent[a].present) return eact_absent_id(t);
        int id = eact_fixed_match(t);
        if (id >= 0) return id;
        int nz = 0, others = 0;
        for (int s = 0; s < E(); s++) {
            if (d2(a, s) == ZS_ENT_ABSENT) continue;
            const bool player = s < np();
            (player ? others : nz)++;
            if (!eact_row_match(t, player, ent[s].x - ent[a].x, ent[s].y - ent[a].y)) continue;
            const int r = rank(a, s);
            if (r >= (player ? kp : kz)) continue;
            const int mine = player ? eact_player_id(kz, r) : eact_zombie_id(r);
            if (id < 0 || mine < id) id = mine;
        }
        if (id < 0 && eact_same(t, eact_triple(ZS_ACT_IDLE, 0, 0))) id = eact_idle_id(nz, others, kz, kp);
        return id;
    }
};

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return 2;
    int ncases = 0;
    if (!rd(f, &ncases)) return 2;
    for (int c = 0; c < ncases; c++) {
        World w;
        int E, O, Q;
        if (!(rd(f, &w.W) && rd(f, &w.H) && rd(f, &w.A) && rd(f, &w.P) && rd(f, &E) && rd(f, &O) && rd(f, &w.kz) && rd(f, &w.kp) &&
              rd(f, &Q)))
            return 2;
        if (!ent_k_ok(w.kz, w.kp) || E < w.A + w.P || w.A < 1 || w.W < 1 || w.H < 1 || O < 0 || Q < 0) return 3;
        w.ent.resize(E);
        w.ob.resize(O);
        std::vector<EactTriple> q(Q);
        for (auto& e : w.ent)
            if (!(rd(f, &e.present) && rd(f, &e.x) && rd(f, &e.y) && rd(f, &e.life) && rd(f, &e.weapon))) return 2;
        for (auto& o : w.ob)
            if (!(rd(f, &o.x) && rd(f, &o.y) && rd(f, &o.present))) return 2;
        for (auto& t : q)
            if (!(rd(f, &t.kind) && rd(f, &t.dx) && rd(f, &t.dy))) return 2;
        const int nid = eact_nid(w.kz, w.kp);
        for (int a = 0; a < w.A; a++) {
            std::vector<EactTriple> dec(nid);
            for (int id = 0; id < nid; id++) {
                int bit;
                dec[id] = w.decode(a, id, &bit);
                printf("%d %d %d %d ", dec[id].kind, dec[id].dx, dec[id].dy, bit);
            }
            for (int id = 0; id < nid; id++) printf("%d ", w.encode(a, dec[id]));
            for (const auto& t : q) printf("%d ", w.encode(a, t));
            printf("\n");
        }
    }
    fclose(f);
    return 0;
}
