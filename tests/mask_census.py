"""What the mask fixtures (tests/golden/masks_*.json.gz) hold, counted from the files alone: the cases the action-mask
rules distinguish (mask_model.py names the rules).  make_mask_golden.py prints it; test_mask_model.py requires
every case of NEED and every bit of every id seen both 0 and 1."""
import collections

import golden_util as G
import mask_model as M

WEAPONS = {10: "knife", 11: "axe", 12: "gun", 13: "rifle", 14: "shotgun"}
NEED = (["surface_single", "surface_multi", "border_x0", "border_x1", "border_y0", "border_y1", "corner",
         "dest_obstacle_alive", "dest_obstacle_nonpos_tick1", "dest_obstacle_gone", "dest_body", "dest_objective",
         "dest_zombie", "dest_player", "dest_outside", "dest_free", "no_zombies", "lone_agent", "dead_beside_live",
         "terminal_call", "heal_closest_bot_in_range", "heal_closest_bot_out_of_range",
         "heal_closest_agent_in_range", "heal_closest_agent_out_of_range"] +
        ["attack_%s_%s" % (w, r) for w in WEAPONS.values() for r in ("in", "out")])


def mask_fixture_names():
    return [n for n in G.fixture_names() if n.startswith("masks_")]


def census(fx, got=None):
    got = collections.Counter() if got is None else got
    mp = M.MapInfo(G.map_path(fx["kwargs"]["map_name"]))
    multi = fx["surface"] == "multi"
    nd = 7 if multi else 6
    for run in fx["runs"]:
        for rec, mk in zip(run["calls"], run["masks"]):
            st = rec["state"]
            got["calls"] += 1
            got["surface_" + fx["surface"]] += 1
            term = rec["kind"] == "step" and (rec["done"] or rec["trunc"])
            got["terminal_call"] += int(term)
            obst, gone = M.obstacle_cells(st, mp)
            dyn = st["dyn"]
            at = {(t[1], t[2]): t for t in dyn}
            dead = {(c % mp.W, c // mp.W) for c in st["dead"]}
            zombies = [t for t in dyn if t[0] == M.ZOMBIE]
            agents = {t[5]: t for t in dyn if t[0] == M.AGENT}
            if agents and len(agents) < len(mk):
                got["dead_beside_live"] += 1
            for a, row in enumerate(mk):
                for k in range(nd):
                    got["bit_%d_%d" % (k, row[k])] += 1
                assert not any(row[nd:]), "entries past the table"
                if a not in agents:
                    assert not any(row), "an absent agent has no set bit"
                    got["agent_absent"] += 1
                    continue
                t = agents[a]
                p = (t[1], t[2])
                bx = [p[0] == 0, p[0] == mp.W - 1, p[1] == 0, p[1] == mp.H - 1]
                for name, b in zip(("border_x0", "border_x1", "border_y0", "border_y1"), bx):
                    got[name] += int(b)
                got["corner"] += int((bx[0] or bx[1]) and (bx[2] or bx[3]))
                for k, (dx, dy) in enumerate(M.MOVES):
                    q = (p[0] + dx, p[1] + dy)
                    if not (0 <= q[0] < mp.W and 0 <= q[1] < mp.H):
                        c = "dest_outside"
                    elif q in obst:
                        c = "dest_obstacle_alive" if obst[q] > 0 else "dest_obstacle_nonpos"
                        if obst[q] <= 0 and st["ctr"][0] == -1:  # World.t of a fresh world: tick 1 comes next
                            got["dest_obstacle_nonpos_tick1"] += 1
                    elif q in at:
                        c = "dest_zombie" if at[q][0] == M.ZOMBIE else "dest_player"
                    else:
                        c = "dest_free"
                        got["dest_obstacle_gone"] += int(q in gone)
                        got["dest_body"] += int(q in dead)
                        got["dest_objective"] += int(q in mp.objectives)
                    got[c] += 1
                if zombies:
                    got["attack_%s_%s" % (WEAPONS[t[4]], "in" if row[4] else "out")] += 1
                else:
                    got["no_zombies"] += 1
                if multi:
                    others = [o for o in dyn if o[0] in (M.PLAYER, M.AGENT) and o is not t]
                    if not others:
                        got["lone_agent"] += 1
                    else:
                        near = min(others, key=lambda o: M.d2(p, (o[1], o[2])))
                        ties = {o[0] for o in others if M.d2(p, (o[1], o[2])) == M.d2(p, (near[1], near[2]))}
                        if len(ties) == 1:
                            got["heal_closest_%s_%s" % ("bot" if near[0] == M.PLAYER else "agent",
                                                        "in_range" if row[6] else "out_of_range")] += 1
    return got


def missing(got):
    need = list(NEED) + ["bit_%d_%d" % (k, v) for k in range(7) for v in (0, 1)]
    return [n for n in need if got[n] == 0]
