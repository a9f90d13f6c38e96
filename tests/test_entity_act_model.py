"""The entity action table's rules on the CPU: libzombsole_amd/entity_act.py against the reference's own probes
(tests/golden/eact_*.json.gz, make_entity_act_golden.py) and against the committed mask fixtures' rows; hand-built
states that pin each rule; and csrc/zs_entity_act.hpp's rule functions, compiled into a stand-alone program under
AddressSanitizer and UBSan (tests/entity_act_host.cpp), on hand-built and generated worlds.  The C ABI exports the new
calls."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import entity_obs_cases as EC
import golden_util as G
import mask_census as C
from entity_obs_cases import View, ent
from libzombsole_amd import actions as ACT
from libzombsole_amd import entity_act as EA
from libzombsole_amd import entity_obs as EO

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
KNIFE, AXE, GUN, RIFLE, SHOTGUN = 10, 11, 12, 13, 14
OPEN = EO.Static(40, 40)
IDLE = [ACT.ACT_IDLE, 0, 0]


# ---- hand-built states -------------------------------------------------------------------------------------------------
def test_layout():
    assert EA.layout(4, 1) == {"nid": 20, "row_bytes": 24, "attack_dir": 7, "heal_dir": 11, "zombie_rows": 15,
                               "player_rows": 19, "end": 20}
    assert EA.layout(1, 0)["nid"] == 16 and EA.layout(1, 0)["row_bytes"] == 16
    assert EA.layout(16, 16)["nid"] == 47 and EA.layout(16, 16)["row_bytes"] == 48
    for kz, kp in ((0, 0), (17, 1), (4, -1), (4, 17)):
        with pytest.raises(ValueError):
            EA.layout(kz, kp)


def test_fixed_entries_and_rows():
    # A = 2, P = 1: agent 0 (knife) at (10, 10), agent 1 at (10, 11), a bot at (13, 10); zombies at (9, 10), (10, 13)
    # and (30, 30); a present obstacle at (11, 10), a removed one at (10, 9)
    st = EO.Static(40, 40, [(11, 10), (10, 9)], [])
    v = View(2, 1, [ent(1, 10, 10, 100, KNIFE), ent(1, 10, 11), ent(1, 13, 10), ent(1, 9, 10), ent(1, 10, 13), ent(1, 30, 30)],
             [1, 0])
    dec, m = EA.decode_all(v, st, 4, 2), EA.mask(v, st, 4, 2)
    assert dec.shape == (2, 21, 3) and m.shape == (2, 24) and not m[:, 21:].any()
    assert dec[0, :7].tolist() == ACT.DISCRETE_TRIPLES.tolist()
    assert dec[0, 7:11].tolist() == [[ACT.ACT_ATTACK, 0, 1], [ACT.ACT_ATTACK, -1, 0], [ACT.ACT_ATTACK, 0, -1], [ACT.ACT_ATTACK, 1, 0]]
    assert dec[0, 11:15].tolist() == [[ACT.ACT_HEAL, 0, 1], [ACT.ACT_HEAL, -1, 0], [ACT.ACT_HEAL, 0, -1], [ACT.ACT_HEAL, 1, 0]]
    # moves: an agent, a zombie, a free cell (the removed obstacle), a present obstacle
    assert m[0, :4].tolist() == [0, 0, 1, 0]
    assert m[0, 4:7].tolist() == [1, 1, 1]  # the adjacent zombie is within the knife's range; agent 1 within healing range
    assert m[0, 7:11].tolist() == [1, 1, 0, 1]  # friendly fire at the agent, the zombie, nothing, the obstacle
    assert m[0, 11:15].tolist() == [1, 0, 0, 1]  # the agent, not the zombie, nothing, the obstacle
    assert dec[0, 15:19].tolist() == [[ACT.ACT_ATTACK, -1, 0], [ACT.ACT_ATTACK, 0, 3], [ACT.ACT_ATTACK, 20, 20], IDLE]
    assert m[0, 15:19].tolist() == [1, 0, 0, 0]
    assert dec[0, 19:21].tolist() == [[ACT.ACT_HEAL, 0, 1], [ACT.ACT_HEAL, 3, 0]] and m[0, 19:21].tolist() == [1, 1]
    # encode: the smallest id; an adjacent zombie's row is the attack-dir entry; idle is the first row that is not valid
    assert EA.encode(v, st, 4, 2, dec[:, 15]).tolist() == [8, 15]
    assert EA.encode(v, st, 4, 2, dec[:, 16]).tolist() == [16, 16]
    assert EA.encode(v, st, 4, 2, [IDLE, IDLE]).tolist() == [18, 18]
    assert EA.encode(v, st, 4, 2, [[ACT.ACT_ATTACK, 5, 5], [ACT.ACT_MOVE, 2, 0]]).tolist() == [-1, -1]
    assert EA.decode(v, st, 4, 2, [21, -1]).tolist() == [IDLE, IDLE]


def test_absent_agent_and_map_edge():
    v = View(2, 0, [ent(0, 3, 3), ent(1, 0, 0, 100, RIFLE), ent(1, 0, 1)])
    st = EO.Static(5, 5)
    dec, m = EA.decode_all(v, st, 1, 1), EA.mask(v, st, 1, 1)
    assert not m[0].any() and (dec[0] == 0).all()
    assert EA.encode(v, st, 1, 1, [IDLE, IDLE]).tolist() == [0, 16] and EA.encode(v, st, 1, 1, [[1, 0, 1]] * 2).tolist() == [-1, 0]
    # the corner: -x and -y lie outside the map, +y holds the zombie; no other player (the absent agent is none)
    assert m[1, :4].tolist() == [0, 0, 0, 1] and m[1, 7:11].tolist() == [1, 0, 0, 0] and m[1, 11:15].tolist() == [0, 0, 0, 0]
    assert m[1, 6] == 1 and m[1, 15] == 1 and m[1, 16] == 0 and dec[1, 16].tolist() == IDLE


# ---- the reference's probes ------------------------------------------------------------------------------------------------
def eact_fixture_names():
    return [n for n in G.fixture_names() if n.startswith("eact_")]


def fixture_view(fx, state, mp):
    """A View of a fixture record's state: agents and bots take their slots, zombies are numbered in dict order."""
    kw = fx["kwargs"]
    A = len(kw["agent_ids"]) if fx["surface"] == "multi" else 1
    P = len(kw["player_names"])
    Z = max(kw["initial_zombies"], kw["minimum_zombies"])
    rows = [[0] * 6 for _ in range(A + P + Z)]
    z = A + P
    for kind, x, y, life, weapon, extra in state["dyn"]:
        if kind == EC.AGENT:
            s = extra
        elif kind == EC.PLAYER:
            s = A + extra
        else:
            s, z = z, z + 1
        rows[s] = [kind, 1, x, y, life, weapon]
    present = np.ones(len(mp.obstacles), dtype=np.int64)
    for i, _life, pr in state["obst"]:
        present[i] = pr
    return View(A, P, rows, present)


def test_there_are_fixtures_with_every_class():
    """Every weapon, a bot, a dead agent beside a live one, a lone agent, an obstacle re-spawned destroyed; probes of both
    kinds seen 0 and 1, at adjacent and at far offsets."""
    names = eact_fixture_names()
    assert len(names) == 5
    weapons, seen = set(), set()
    for n in names:
        fx = G.load_fixture(n)
        assert len(fx["runs"]) >= 2
        seen |= {"bot"} if fx["kwargs"]["player_names"] else set()
        seen |= {"poked"} if G.obstacle_pokes(fx) else set()
        for run in fx["runs"]:
            assert len(run["probes"]) == len(run["calls"])
            for rec, probes in zip(run["calls"], run["probes"]):
                agents = [t for t in rec["state"]["dyn"] if t[0] == EC.AGENT]
                weapons |= {t[4] for t in agents}
                live = sum(1 for p in probes if p)
                assert live == len(agents)
                seen |= {"dead_beside_live"} if 0 < live < len(probes) else set()
                seen |= {"lone"} if live == 1 and not any(t[0] == EC.PLAYER for t in rec["state"]["dyn"]) else set()
                for row in probes:
                    seen |= {(k, dx * dx + dy * dy == 1, ok) for k, dx, dy, ok in row}
    assert weapons == {KNIFE, AXE, GUN, RIFLE, SHOTGUN}
    assert {"bot", "poked", "dead_beside_live", "lone"} <= seen
    assert {(k, adj, ok) for k in (ACT.ACT_ATTACK, ACT.ACT_HEAL) for adj in (True, False) for ok in (0, 1)} <= seen


@pytest.mark.parametrize("name", eact_fixture_names())
@pytest.mark.parametrize("kz,kp", EC.KS)
def test_model_equals_the_references_probes(name, kz, kp):
    """Every call's state replayed: for every agent and id from 7 up, the model's mask bit is `ok` of the probe at the
    id's decoded triple.  A row the probes do not reach lies beyond distance 11, outside every range."""
    fx = G.load_fixture(name)
    mp = EO.Static.of_map(G.map_path(fx["kwargs"]["map_name"]))
    checked = live = 0
    for run in fx["runs"]:
        for i, (rec, probes) in enumerate(zip(run["calls"], run["probes"])):
            v = fixture_view(fx, rec["state"], mp)
            dec, m = EA.decode_all(v, mp, kz, kp), EA.mask(v, mp, kz, kp)
            for a, row in enumerate(probes):
                if not row:
                    assert not m[a].any() and not dec[a].any(), (name, run["seed"], i, a)
                    continue
                live += 1
                ok = {(k, dx, dy): o for k, dx, dy, o in row}
                for j in range(EA.ATTACK_DIR, EA.layout(kz, kp)["nid"]):
                    t = tuple(int(x) for x in dec[a, j])
                    if t == tuple(IDLE):
                        assert j >= EA.FIXED and m[a, j] == 0
                    elif t in ok:
                        assert m[a, j] == ok[t], (name, run["seed"], i, a, j, t)
                        checked += 1
                    else:
                        assert j >= EA.FIXED and t[1] ** 2 + t[2] ** 2 > 121 and m[a, j] == 0, (name, run["seed"], i, a, j, t)
                # every thing the reference could act on within distance 11 is named by the table when K admits it
                if (kz, kp) == (16, 16):
                    named = {tuple(int(x) for x in t) for t in dec[a]}
                    for (k, dx, dy), o in ok.items():
                        at = [t for t in rec["state"]["dyn"] if (t[1], t[2]) == (int(v.ent[a][2]) + dx, int(v.ent[a][3]) + dy)]
                        if o and at and (k == ACT.ACT_ATTACK) == (at[0][0] == EC.ZOMBIE):
                            assert (k, dx, dy) in named, (name, run["seed"], i, a, k, dx, dy)
    assert live >= 80 and checked >= 8 * live  # the eight adjacent entries of every live agent of every call, and the rows


@pytest.mark.parametrize("name", [n for n in C.mask_fixture_names() if "_multi_" in n])
def test_ids_0_to_6_are_the_mask_fixtures_rows(name):
    fx = G.load_fixture(name)
    mp = EO.Static.of_map(G.map_path(fx["kwargs"]["map_name"]))
    for run in fx["runs"]:
        for i, (rec, want) in enumerate(zip(run["calls"], run["masks"])):
            m = EA.mask(fixture_view(fx, rec["state"], mp), mp, 4, 1)
            assert m[:, :7].tolist() == [w[:7] for w in want], (name, run["seed"], i)


# ---- the header's rule functions, as a program ------------------------------------------------------------------------
QUERIES = [IDLE, [ACT.ACT_IDLE, 1, 0], [ACT.ACT_MOVE, 0, 1], [ACT.ACT_MOVE, 1, 1], [ACT.ACT_ATTACK, 1, 0], [ACT.ACT_ATTACK, 0, 0],
           [ACT.ACT_ATTACK, 2, 0], [ACT.ACT_ATTACK, -1, 2], [ACT.ACT_HEAL, 0, 0], [ACT.ACT_HEAL, 0, -1], [ACT.ACT_HEAL, 2, 0],
           [ACT.ACT_HEAL, 1, 1], [ACT.ACT_ATTACK_CLOSEST, 0, 0], [ACT.ACT_ATTACK_CLOSEST, 1, 0], [ACT.ACT_HEAL_CLOSEST, 0, 0],
           [ACT.ACT_CONFUSED, 0, 0], [ACT.ACT_ATTACK, 0, 40000]]


def host_text(cases):
    lines = [str(len(cases))]
    for v, st, kz, kp in cases:
        lines.append("%d %d %d %d %d %d %d %d %d" % (st.W, st.H, v.A, v.P, len(v.ent), len(st.obstacles), kz, kp, len(QUERIES)))
        lines += ["%d %d %d %d %d" % tuple(int(x) for x in e[1:6]) for e in v.ent]
        lines += ["%d %d %d" % (x, y, int(v.obst_present[i])) for i, (x, y) in enumerate(st.obstacles)]
        lines += ["%d %d %d" % tuple(q) for q in QUERIES]
    return "\n".join(lines) + "\n"


def generated_worlds():
    """Small crowded worlds: equidistant slots at every turn, classes that are empty or shorter than K, agents on the
    map's edge and in its corners, absent agents, obstacles present and removed."""
    rng = np.random.RandomState(20260)
    out = []
    for i in range(60):
        W, H = [(5, 4), (7, 3), (1, 9), (9, 7)][i % 4]
        A, P = [(1, 0), (2, 1), (4, 2), (3, 0)][(i // 4) % 4]
        Z = int(rng.randint(0, 9))
        cells = [(x, y) for x in range(W) for y in range(H)]
        rng.shuffle(cells)
        n_ob = min(int(rng.randint(0, 4)), max(0, len(cells) - (A + P + Z)))
        obstacles, cells = cells[:n_ob], cells[n_ob:]
        if i % 5 == 0 and (0, 0) in cells:  # agent 0 in a corner
            cells.append(cells.pop(cells.index((0, 0))))
        rows = []
        for s in range(A + P + Z):
            if cells and (rng.rand() < 0.8 or (s == 0 and i % 5 == 0)):
                x, y = cells.pop()
                rows.append(ent(1, x, y, int(rng.randint(-5, 120)), int(rng.choice([KNIFE, AXE, GUN, RIFLE, SHOTGUN]))))
            else:
                rows.append(ent(0, int(rng.randint(0, W)), int(rng.randint(0, H))))
        out.append((View(A, P, rows, [int(rng.rand() < 0.7) for _ in obstacles]), EO.Static(W, H, obstacles, [])))
    return out


def hand_built():
    st = EO.Static(40, 40, [(11, 10), (10, 9)], [])
    return [
        (View(2, 1, [ent(1, 10, 10, 100, KNIFE), ent(1, 10, 11), ent(1, 13, 10), ent(1, 9, 10), ent(1, 10, 13), ent(1, 30, 30)],
              [1, 0]), st),
        (View(2, 0, [ent(0, 3, 3), ent(1, 0, 0, 100, RIFLE), ent(1, 0, 1)]), EO.Static(5, 5)),
        (View(1, 0, [ent(1, 10, 10), ent(1, 12, 10, 7), ent(1, 10, 8, 9), ent(1, 8, 10, 5)]), OPEN),  # a three-way tie
        (View(1, 0, [ent(1, 10, 10), ent(0, 11, 10), ent(0, 12, 10)]), OPEN),  # no zombies
        (View(1, 1, [ent(1, 10, 10), ent(0, 11, 10), ent(1, 12, 10)]), OPEN),  # a lone agent
        (View(2, 1, [ent(1, 10, 10), ent(1, 13, 10, 50, GUN), ent(1, 9, 13, 60, AXE)]), OPEN),  # healing range 9 and 10
    ]


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    cxx = shutil.which("clang++") or shutil.which("g++") or shutil.which("c++")
    if cxx is None and os.path.exists("/opt/rocm/llvm/bin/clang++"):
        cxx = "/opt/rocm/llvm/bin/clang++"
    assert cxx, "a host C++ compiler"
    exe = str(tmp_path_factory.mktemp("entity_act") / "entity_act_host")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "libzombsole_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "entity_act_host.cpp")])
    return exe


def _run_host(exe, cases, tmp_path, name):
    path = tmp_path / (name + ".txt")
    path.write_text(host_text(cases))
    lines = subprocess.check_output([exe, str(path)], text=True).splitlines()
    assert len(lines) == sum(c[0].A for c in cases)
    it = iter(lines)
    return [[np.array(next(it).split(), dtype=np.int64) for _ in range(c[0].A)] for c in cases]


def _check_host(got, cases):
    for ci, (c, rows) in enumerate(zip(cases, got)):
        v, st, kz, kp = c
        nid = EA.layout(kz, kp)["nid"]
        dec, m = EA.decode_all(v, st, kz, kp), EA.mask(v, st, kz, kp)
        enc_own = np.stack([EA.encode(v, st, kz, kp, dec[:, j]) for j in range(nid)], axis=1)
        enc_q = np.stack([EA.encode(v, st, kz, kp, [q] * v.A) for q in QUERIES], axis=1)
        for a, r in enumerate(rows):
            assert len(r) == 5 * nid + len(QUERIES), (ci, a)
            table = r[:4 * nid].reshape(nid, 4)
            assert np.array_equal(table[:, :3], dec[a]), (ci, a, kz, kp, table[:, :3].tolist(), dec[a].tolist())
            assert np.array_equal(table[:, 3], m[a, :nid]), (ci, a, kz, kp, table[:, 3].tolist(), m[a].tolist())
            assert np.array_equal(r[4 * nid:5 * nid], enc_own[a]), (ci, a, kz, kp, r[4 * nid:5 * nid].tolist(), enc_own[a].tolist())
            assert np.array_equal(r[5 * nid:], enc_q[a]), (ci, a, kz, kp, r[5 * nid:].tolist(), enc_q[a].tolist())


def test_host_program_equals_the_model(host_program, tmp_path):
    worlds = hand_built() + generated_worlds()
    cases = [(v, st, kz, kp) for v, st in worlds for kz, kp in EC.KS]
    _check_host(_run_host(host_program, cases, tmp_path, "worlds"), cases)
    # the generated worlds hold what they were made for
    ties = short = edge = absent = 0
    for v, st in generated_worlds():
        for a in range(v.A):
            if not v.ent[a][1]:
                absent += 1
                continue
            ax, ay = int(v.ent[a][2]), int(v.ent[a][3])
            d = sorted((int(e[2]) - ax) ** 2 + (int(e[3]) - ay) ** 2 for e in v.ent[v.A + v.P:] if e[1])
            ties += any(x == y for x, y in zip(d, d[1:]))
            short += len(d) < 4
            edge += ax in (0, st.W - 1) or ay in (0, st.H - 1)
    assert min(ties, short, edge, absent) >= 10, (ties, short, edge, absent)


MUTANTS = {
    "heal_dir_takes_zombies": ("(w.obst | w.player)) >> k", "(w.obst | w.thing)) >> k"),
    "row_range_lt": ("return d2 <= (player ? ZS_ENT_HEAL_R2 : r2) ? 1 : 0;", "return d2 < (player ? ZS_ENT_HEAL_R2 : r2) ? 1 : 0;"),
    "idle_prefers_players": ("return nz < kz ? eact_zombie_id(nz) : others < kp ? eact_player_id(kz, others) : -1;",
                             "return others < kp ? eact_player_id(kz, others) : nz < kz ? eact_zombie_id(nz) : -1;"),
}


@pytest.mark.parametrize("name", sorted(MUTANTS))
def test_a_wrong_rule_is_caught(name, tmp_path):
    """The header with one rule changed, built as a program: its table differs from the model's on the hand-built states."""
    old, new = MUTANTS[name]
    text = open(os.path.join(ROOT, "libzombsole_amd", "csrc", "zs_entity_act.hpp")).read()
    assert text.count(old) == 1, (name, "the rule's text is in the source once")
    (tmp_path / "zs_entity_act.hpp").write_text(text.replace(old, new))
    (tmp_path / "entity_act_host.cpp").write_text(open(os.path.join(ROOT, "tests", "entity_act_host.cpp")).read())
    cxx = shutil.which("clang++") or shutil.which("g++") or shutil.which("c++") or "/opt/rocm/llvm/bin/clang++"
    exe = str(tmp_path / "mutant")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-I", str(tmp_path), "-I", os.path.join(ROOT, "libzombsole_amd", "csrc"),
                           "-o", exe, str(tmp_path / "entity_act_host.cpp")])
    cases = [(v, st, 4, 2) for v, st in hand_built()]
    with pytest.raises(AssertionError):
        _check_host(_run_host(exe, cases, tmp_path, name), cases)


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------
def test_the_calls_are_exported_and_bound():
    from libzombsole_amd import _abi, engine
    L = engine.load_library()
    for name, n in (("zs_entity_act_table", 4), ("zs_entity_act_decode", 7), ("zs_entity_act_mask", 6),
                    ("zs_entity_act_encode", 7), ("zs_entity_act_bind", 5)):
        assert name in _abi.ABI and len(_abi.ABI[name]) == n
        f = getattr(L, name)
        assert ctypes.cast(f, ctypes.c_void_p).value and list(f.argtypes) == list(_abi.ABI[name]) and f.restype is ctypes.c_int
    assert _abi.ENTITY_ACT_TABLE_KEYS[:7] == EA.LAYOUT_KEYS and _abi.ENTITY_ACT_TABLE_KEYS[7] is None
    # a null handle is refused by every call before anything else
    assert L.zs_entity_act_table(None, 4, 1, (ctypes.c_int32 * 8)()) == _abi.ZS_EINVAL
    assert L.zs_entity_act_decode(None, None, 4, 1, None, None, None) == _abi.ZS_EINVAL
    assert L.zs_entity_act_mask(None, None, 4, 1, None, None) == _abi.ZS_EINVAL
    assert L.zs_entity_act_encode(None, None, 4, 1, None, None, None) == _abi.ZS_EINVAL
    assert L.zs_entity_act_bind(None, None, None, 4, 1) == _abi.ZS_EINVAL
