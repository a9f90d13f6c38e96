"""The action and death logs on the CPU: the oracle's logs (zo_set_logs) pinned to the real reference through the
events fixtures, and the census of log_cases.py's rows.

The pin: every events_* fixture is replayed on the oracle with logs on.  From the oracle's state before the step,
its two logs and the obstacles present after the step, a formatter written here (independent of game.py) forms the
step's World.events (core.py:68-70): 'idle' or 'error with next_step: ...' for every actor in dict order that gave no
action (core.py:80-101), the outcome message of every executed action in execution order with positions and occupancy
followed through the moves (core.py:103-119, 140-202), 'died' for the obstacles in map order and then for the logged
things (core.py:121-138).  Every step's [family, name, message] list must equal the fixture's.
"""
import pytest

import golden_util as G
import log_cases as L
import step_plan_table as T
from libzombsole_amd import actions as A
from oracle.oracle import OracleEnv, OracleRaised

EVENT_FIXTURES = sorted(n for n in G.fixture_names() if n.startswith("events_"))
WEAPON_NAME = {1: "ZombieClaws", 10: "Knife", 11: "Axe", 12: "Gun", 13: "Rifle", 14: "Shotgun"}  # observation codes
RANGE2 = {1: 2, 10: 2, 11: 2, 12: 36, 13: 100, 14: 9}  # the largest d^2 within max_range 1.5, 1.5, 1.5, 6, 10, 3
FAMILY = {5: ("zombie", None), 6: ("player", None), 7: ("agent", "agent"), 1: ("box", "box"), 4: ("wall", "wall")}


def step_events(builder, bots, pre, post, n, rows, deaths, errors):
    """One step's events as [family, name, message] from the oracle's pre-step state, logs and post-step obstacles.
    errors: agent index -> the message of the error its next_step raised.  Returns (events, simulated effects)."""
    W, H = builder.map.size
    obst = [(int(x), int(y), int(k)) for x, y, k in builder.map.obstacles]

    def name(kind, extra):
        fam, nm = FAMILY[kind]
        return [fam, nm if nm else ("zombie" if kind == 5 else bots[extra])]

    gone = {o[0] for o in pre["obst"] if not o[2]}
    occ = {(x, y): name(k, 0) for i, (x, y, k) in enumerate(obst) if i not in gone}
    thing, weapon = {}, {}
    acted = {r[0] for r in rows}
    ev = []
    for kind, x, y, life, w, extra in pre["dyn"]:
        thing[(x, y)] = name(kind, extra)
        weapon[(x, y)] = w
        occ[(x, y)] = thing[(x, y)]
        if kind == 7 and extra in errors:
            ev.append(thing[(x, y)] + ["error with next_step: %s" % errors[extra]])
            if n < 0:
                return ev, []  # debug: the step stopped here
        elif (x, y) not in acted:
            ev.append(thing[(x, y)] + ["idle"])
    assert n >= 0, "a raised step without a raising agent in the world"
    pos = {c: c for c in thing}  # pre-step cell -> the cell now
    effects = []
    for cell, kind, act, tgt, _ in rows:
        me, (x, y) = thing[cell], pos[cell]
        assert FAMILY[kind][0] == me[0]
        ok = False
        if act == 1:
            dx, dy = tgt[1], tgt[2]
            if 0 <= dx < W and 0 <= dy < H:
                if (dx, dy) in occ:
                    msg = "hit %s with his head" % occ[(dx, dy)][1]
                elif (dx - x) ** 2 + (dy - y) ** 2 > 1:
                    msg = "tried to walk too fast, but physics forbade it"
                else:
                    del occ[(x, y)]
                    occ[(dx, dy)] = me
                    pos[cell] = (dx, dy)
                    msg, ok = "moved to " + str((dx, dy)), True
            else:
                msg = "Tried to move out of bounds to %s" % str((dx, dy))
        else:
            if tgt[0] == "obst":
                tx, ty, k = obst[tgt[1]]
                tname = name(k, 0)[1]
            else:
                (tx, ty), tname = pos[(tgt[1], tgt[2])], thing[(tgt[1], tgt[2])][1]
            d2 = (tx - x) ** 2 + (ty - y) ** 2
            if act == 2:
                wn = WEAPON_NAME[weapon[cell]]
                ok = d2 <= RANGE2[weapon[cell]]
                msg = ("injured %s with a %s" if ok else "tried to attack %s, but it is too far for a %s") % (tname, wn)
            else:
                ok = d2 <= 9  # HEALING_RANGE = 3
                msg = ("healed " + tname) if ok else "tried to heal %s, but it is too far away" % tname
        effects.append(ok)
        ev.append(me + [msg])
    gone_after = {o[0] for o in post["obst"] if not o[2]}
    for i, (x, y, k) in enumerate(obst):
        if i in gone_after and i not in gone:
            ev.append(name(k, 0) + ["died"])
    for kind, idx, x, y, life, cell in deaths:
        assert life <= 0 and pos[cell] == (x, y), ("a logged death's position", cell, (x, y), pos[cell])
        ev.append(thing[cell] + ["died"])
    return ev, effects


def replay_events(fx, run):
    """The number of events compared over one run of a fixture."""
    b = G.builder_for(fx)
    bots = fx["kwargs"].get("player_names", [])
    env = OracleEnv(b)
    for i, life in G.obstacle_pokes(fx):
        assert env.poke_obstacle(i, life) == 0
    env.seed(run["seed"])
    env.set_logs()
    compared, carry = 0, []
    for i, rec in enumerate(run["calls"]):
        where = (fx["name"], run["seed"], i)
        if rec["kind"] == "reset":
            env.reset()
            assert env.action_log()[0] == 0 and env.death_log() == [], where
            assert not carry, where
            continue
        acts = rec["act"] if fx["surface"] == "multi" else [rec["act"]]
        errors = {}
        if fx["stream"] not in ("discrete",):
            for a, act in enumerate(acts):
                try:
                    A.encode_action(act)
                except A.ActionError as err:
                    errors[a] = str(err.args[0])
        pre = env.state()
        try:
            env.step(G.action_triples(fx, rec, b.num_agents))
            raised = False
        except OracleRaised:
            raised = True
        n, rows, _ = env.action_log()
        assert raised == (n < 0) == ("raised" in rec), where
        ev, effects = step_events(b, bots, pre, env.state(), n, rows, env.death_log(), errors)
        if raised:  # World.step re-raised: the driver records that step's events with the next step's
            assert env.death_log() == [], where
            carry += ev
            continue
        assert effects == [r[4] for r in rows], (where, "the oracle's effect flags", effects, rows)
        assert [e[1:] for e in rec["events"]] == carry + ev, (where, rec["events"], carry + ev)
        compared += len(rec["events"])
        carry = []
    return compared


# fixture -> the events its recording holds (every one of them is compared)
EVENT_COUNTS = {"events_multi_bridge_a3_bad": 1613, "events_multi_bridge_a4_rich": 2931, "events_multi_fort_a8_z40": 2486,
                "events_single_boxed_bots_rich": 1792, "events_single_easyexit_debug_bad": 918,
                "events_multi_melee_far_moves": 133}


@pytest.mark.parametrize("name", EVENT_FIXTURES)
def test_oracle_logs_give_the_references_events(name):
    fx = G.load_fixture(name)
    compared = sum(replay_events(fx, run) for run in fx["runs"])
    assert compared == sum(len(rec.get("events", [])) for run in fx["runs"] for rec in run["calls"]) > 100
    if name in EVENT_COUNTS:
        assert compared == EVENT_COUNTS[name]


def test_the_event_fixtures_are_there():
    assert set(EVENT_COUNTS) <= set(EVENT_FIXTURES)


def test_the_far_move_fixture_holds_near_and_far_destinations():
    """Moves off the map to x < 0 and y >= H within a step or 25 of it, and to coordinates no 16-bit field holds
    (the engine's action log packs a destination as x | y << 16, offsets clamped to +-16384)."""
    import re
    fx = G.load_fixture("events_multi_melee_far_moves")
    H = 6
    dests = [tuple(int(v) for v in re.findall(r"-?\d+", ev[3])) for run in fx["runs"] for rec in run["calls"]
             for ev in rec.get("events", []) if ev[1] == "agent" and ev[3].startswith("Tried to move out of bounds")]
    assert len(dests) == 38
    assert any(-25 <= x < 0 and 0 <= y < H for x, y in dests) and any(H <= y <= H + 25 for x, y in dests)
    assert any(x > 32767 for x, y in dests) and any(x < -32768 for x, y in dests)
    assert any(y > 32767 for x, y in dests) and any(y < -32768 for x, y in dests)
    assert any(x > 2 ** 31 for x, y in dests)


def test_logs_off_by_default_and_silent_on_reset():
    """Without zo_set_logs a step keeps no log; with it, a reset leaves both logs empty."""
    row = L.ROWS[1]
    o = OracleEnv(row.make(1))
    o.seed(3)
    o.reset()
    o.step(row.actions([3], 1, o.A)[0])
    assert o.action_log() == (0, [], False) and o.death_log() == []
    o.set_logs()
    o.step(row.actions([3], 2, o.A)[0])
    assert o.action_log()[0] > 0
    o.reset()
    assert o.action_log() == (0, [], False) and o.death_log() == []


# -- the case table ----------------------------------------------------------------------------------------------
def test_rows_cover_all_21_and_the_raise_rows():
    import step_instantiations as S
    rows = [(r.G, r.kernel) for r in L.ROWS]
    assert len(rows) == 21 and set(rows) == set(S.all_instantiations())
    for r in L.ROWS:
        assert r.n == S.ENVS[r.G] and r.launch == S.Row(r.G, r.kernel, "c2", ()).launch
    for r in L.ALL_ROWS:
        assert r.make(1).cfg.flags & 4  # _abi.FLAG_DEATH_LOG
    raise_gs = {r.G for r in L.RAISE_ROWS}
    assert {1, 8, 64} <= raise_gs
    assert all(r.make(1).cfg.flags & 2 and r.stream == "bad" for r in L.RAISE_ROWS)  # _abi.FLAG_DEBUG
    assert any(1 in list(r.make(1).cfg.bot_types[:r.make(1).cfg.num_bots]) or "ham" in r.config for r in L.RAISE_ROWS)
    assert len({r.id for r in L.ALL_ROWS}) == len(L.ALL_ROWS)


def test_the_plan_resolves_every_row_to_its_instantiation():
    plans = T.plans([(r.builder(), dict(r.launch, par_exec=1)) for r in L.ALL_ROWS])
    for r, p in zip(L.ALL_ROWS, plans):
        assert "error" not in p, (r.id, p)
        assert (p["G"], bool(p["fused"]), p["tick_waves"]) == (r.G, r.fused, r.tick_waves), (r.id, p)
        assert ("k_respawn" if p["defer_respawn"] else "tick") == r.respawn, (r.id, p)


@pytest.fixture(scope="module")
def census():
    return {r.id: L.census(r) for r in L.ALL_ROWS}


def test_rows_of_every_lane_count_meet_every_class(census):
    """A condition on the inputs, met by the oracle alone: the rows of every G meet every class of log_cases.CLASSES
    NEED_EACH times or more between them, or the class is listed as unreachable at that G with its reason."""
    import step_instantiations as S
    for G_ in S.GS:
        rows = [r for r in L.ALL_ROWS if r.G == G_]
        for c in L.CLASSES:
            tot = sum(census[r.id][c] for r in rows)
            if c in L.UNREACHABLE.get(G_, {}):
                assert L.UNREACHABLE[G_][c] and tot == 0, (G_, c, tot)
            else:
                assert tot >= L.NEED_EACH, (G_, c, tot, {r.id: census[r.id][c] for r in rows})
    for r in L.ALL_ROWS:  # every row resets, logs actions and (but the lonely rows) removes things
        c = census[r.id]
        assert c["resets"] >= r.n and c["entries"] > 0, (r.id, c)
        assert c["removed"] > 0 or r.config == "lonely", (r.id, c)


def test_walk_model():
    """The cleanup's walk: a mover is met behind the K pre-step entries, in execution order."""
    cells = [(1, 1), (2, 1), (3, 1)]
    rows = [((3, 1), 5, 1, ("cell", 3, 2), True), ((2, 1), 5, 1, ("cell", 9, 9), False),
            ((1, 1), 7, 1, ("cell", 1, 2), True)]
    assert L.walk(cells, rows) == cells + [(3, 1), (1, 1)]
    assert [L.walk_index(cells, rows, c) for c in cells] == [4, 1, 3]
