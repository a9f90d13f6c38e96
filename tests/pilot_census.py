"""What the autopilot fixtures (tests/golden/pilot/pilot_*.json.gz) hold, counted from the files alone: the cases a wrong
k_autopilot would miss (libzombsole_amd/autopilot.py names the rules).  make_pilot_golden.py prints it;
test_autopilot_model.py requires every case of NEED.

The tie cases: a zombie on a diagonal of the agent (|dx| == |dy|) makes two adjacent cells equidistant to it, and
adjacent_positions order resolves (0,1) over (1,0), (0,-1) over (-1,0) and, the other way round the compass, (0,1) over
(-1,0) and (0,-1) over (1,0).

The slot case: two zombies at the minimal d2 whose dict-order ranks are opposite to their slot numbers and whose best
cells differ, so a kernel breaking the tie by slot walks the wrong way.  A fixture holds no slot numbers; the engine
gives zombies their slots in spawn order, which is the order of the records' `zid` idents, so the case is counted among
zombies present since the episode's reset call (a respawned zombie may take a freed slot)."""
import collections
import glob
import os

import golden_util as G
from libzombsole_amd import autopilot as AP
from libzombsole_amd import entity_obs as EO
from libzombsole_amd.maps import load_map

ZOMBIE, PLAYER, AGENT = 5, 6, 7
POLICY_NAMES = ("terminator", "sniper", "troll")
NEED = ["surface_single", "surface_multi", "in_range", "free_cell", "cell_outside", "cell_agent", "cell_bot",
        "cell_obstacle_alive", "cell_obstacle_destroyed", "dir_0", "dir_1", "dir_2", "dir_3", "tie_01_over_10",
        "tie_0m1_over_m10", "tie_01_over_m10", "tie_0m1_over_10", "slot_order_tie", "no_zombies", "absent_agent",
        "three_weapon_ranges", "terminal_call", "poked_call"]
TIES = {(0, 2): "tie_01_over_10", (1, 3): "tie_0m1_over_m10", (0, 3): "tie_01_over_m10", (1, 2): "tie_0m1_over_10"}


def pilot_fixture_names():
    """The fixtures lie in tests/golden/pilot/, beside the top-level ones that every replay test takes up
    (golden_util.fixture_names): golden_driver's own action streams cannot retake a policy-driven step or a poke."""
    return sorted("pilot/" + os.path.basename(p)[:-len(".json.gz")] for p in glob.glob(os.path.join(G.GOLDEN, "pilot", "pilot_*.json.gz")))


def static_of(fx):
    return EO.Static.of_map(G.map_path(fx["kwargs"]["map_name"]))


def n_agents(fx):
    return len(fx["kwargs"]["agent_ids"]) if fx["surface"] == "multi" else 1


def best_dir(p, z):
    d = [(z[0] - p[0] - dx) ** 2 + (z[1] - p[1] - dy) ** 2 for dx, dy in AP.ADJACENT]
    k = d.index(min(d))
    return k, [j for j in range(4) if d[j] == d[k]]


def census(fx, got=None):
    got = collections.Counter() if got is None else got
    st_map = static_of(fx)
    kinds = [o[2] for o in load_map(G.map_path(fx["kwargs"]["map_name"])).obstacles]
    pokes = {(p[0], p[1]) for p in (fx.get("extras") or {}).get("poke_things", [])}
    for run in fx["runs"]:
        since_reset = set()
        for c, (rec, pl) in enumerate(zip(run["calls"], run["pilot"])):
            st = rec["state"]
            got["calls"] += 1
            got["surface_" + fx["surface"]] += 1
            got["terminal_call"] += int(rec["kind"] == "step" and (rec["done"] or rec["trunc"]))
            got["poked_call"] += int((run["seed"], c) in pokes)
            idents = [z[0] for z in rec["zid"]]
            if rec["kind"] == "reset":
                since_reset = set(idents)
            dyn = st["dyn"]
            at = {(t[1], t[2]): t for t in dyn}
            changed = {i: (lf, present) for i, lf, present in st["obst"]}
            zombies = [(k, t) for k, t in enumerate(dyn) if t[0] == ZOMBIE]
            zident = dict(zip([k for k, _ in zombies], idents))
            assert len(idents) == len(zombies)
            agents = {t[5]: t for t in dyn if t[0] == AGENT}
            for a, row in enumerate(pl["terminator"]):
                if a not in agents:
                    assert row == [0, 0, 0] and pl["sniper"][a] == [0, 0, 0] and pl["troll"][a] == [0, 0, 0]
                    got["absent_agent"] += 1
                    continue
                t = agents[a]
                p = (t[1], t[2])
                r2 = EO.weapon_r2(t[4])
                got["weapon_r2_%d" % r2] += 1
                if not zombies:
                    got["no_zombies"] += 1
                    continue
                dd = [((z[1] - p[0]) ** 2 + (z[2] - p[1]) ** 2, k) for k, z in zombies]
                dmin, kmin = min(dd)
                if dmin <= r2:
                    got["in_range"] += 1
                    continue
                z = dyn[kmin]
                k, tied = best_dir(p, (z[1], z[2]))
                got["dir_%d" % k] += 1
                if len(tied) == 2:
                    got[TIES[tuple(tied)]] += 1
                for d2, k2 in dd:
                    if d2 == dmin and k2 != kmin and zident[k2] < zident[kmin] and {zident[k2], zident[kmin]} <= since_reset:
                        if best_dir(p, (dyn[k2][1], dyn[k2][2]))[0] != k:
                            got["slot_order_tie"] += 1
                cell = (p[0] + AP.ADJACENT[k][0], p[1] + AP.ADJACENT[k][1])
                o = st_map.obstacle_at.get(cell)
                if not (0 <= cell[0] < st_map.W and 0 <= cell[1] < st_map.H):
                    got["cell_outside"] += 1
                elif o is not None and changed.get(o, (1, 1))[1]:
                    life = changed.get(o, (10 if kinds[o] == 1 else 200, 1))[0]
                    got["cell_obstacle_alive" if life > 0 else "cell_obstacle_destroyed"] += 1
                elif cell in at:
                    got["cell_agent" if at[cell][0] == AGENT else "cell_bot" if at[cell][0] == PLAYER else "cell_zombie"] += 1
                else:
                    got["free_cell"] += 1
    got["three_weapon_ranges"] = int(sum(1 for k in got if k.startswith("weapon_r2_") and got[k]) >= 3)
    return got


def missing(got):
    return [n for n in NEED if got[n] == 0]


class View(object):
    """A fixture record's canonical state with the fields autopilot.decide reads of an engine.StateView.  The zombies'
    slots follow the dict order (a fixture holds no slot numbers, and the rules read none)."""

    def __init__(self, state, fx, st_map):
        A = n_agents(fx)
        P = len(fx["kwargs"].get("player_names", []))
        Z = max(fx["kwargs"].get("initial_zombies", 0), fx["kwargs"].get("minimum_zombies", 0))
        self.A, self.P = A, P
        self.ent = [[0] * 8 for _ in range(A + P + Z)]
        self.order = []
        nz = 0
        for t in state["dyn"]:
            if t[0] == ZOMBIE:
                s = A + P + nz
                nz += 1
            else:
                s = t[5] if t[0] == AGENT else A + t[5]
            self.ent[s] = [t[0], 1, t[1], t[2], t[3], t[4], t[5], 0]
            self.order.append(s)
        self.n_order = len(self.order)
        self.obst_present = [1] * len(st_map.obstacles)
        for i, _life, present in state["obst"]:
            self.obst_present[i] = present


def host_text(cases):
    """tests/autopilot_host.cpp's input for [(view, static, codes)]."""
    out = [str(len(cases))]
    for v, m, codes in cases:
        rank = {s: k for k, s in enumerate(v.order[:v.n_order])}
        out.append("%d %d %d %d %d %d" % (m.W, m.H, v.A, v.P, len(v.ent), len(m.obstacles)))
        out.append(" ".join("%d %d %d %d %d" % (r[1], r[2], r[3], r[5], rank.get(s, 0xffff)) for s, r in enumerate(v.ent)))
        out.append(" ".join("%d %d %d" % (c[0], c[1], int(v.obst_present[i])) for i, c in enumerate(m.obstacles)))
        out.append(" ".join(str(int(c)) for c in codes))
    return "\n".join(out) + "\n"
