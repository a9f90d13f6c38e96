"""The entity observation's rules on the CPU: hand-built states pin each rule of libzombsole_amd/entity_obs.py's encode,
and csrc/zs_entity_obs.hpp's rule functions, compiled into a stand-alone program under AddressSanitizer and UBSan
(tests/entity_obs_host.cpp), give the same rows on those states and on the oracle's states of every GPU row."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import entity_obs_cases as EC
from entity_obs_cases import View, ent
from libzombsole_amd import entity_obs as EO

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
KNIFE, AXE, GUN, RIFLE, SHOTGUN = 10, 11, 12, 13, 14
OPEN = EO.Static(40, 40)


def zrow(rows, a, i, kz=4, kp=1):
    o = EO.layout(kz, kp)["zombies"] + 4 * i
    return [int(v) for v in rows[a][o:o + 4]]


def prow(rows, a, i, kz=4, kp=1):
    o = EO.layout(kz, kp)["players"] + 4 * i
    return [int(v) for v in rows[a][o:o + 4]]


def block(rows, a, name, kz=4, kp=1):
    o = EO.layout(kz, kp)[name]
    return [int(v) for v in rows[a][o:o + 4]]


# ---- the hand-built states: name -> (view, static, kz, kp) ------------------------------------------------------------
def _cases():
    c = {}
    # A = 1, P = 0: slot 0 the agent at (10, 10), zombies from slot 1
    c["tie"] = (View(1, 0, [ent(1, 10, 10), ent(1, 12, 10, 7), ent(1, 10, 8, 9), ent(1, 8, 10, 5)]), OPEN, 4, 1)
    c["kz_plus_one"] = (View(1, 0, [ent(1, 10, 10)] + [ent(1, 10 + i, 10, 10 + i) for i in (5, 1, 4, 2, 3)]), OPEN, 4, 1)
    c["no_zombies"] = (View(1, 0, [ent(1, 10, 10), ent(0, 11, 10), ent(0, 12, 10)]), OPEN, 4, 1)
    c["absent_agent"] = (View(2, 0, [ent(0, 3, 3), ent(1, 10, 10), ent(1, 11, 10)]), OPEN, 4, 1)
    c["lone_agent"] = (View(1, 1, [ent(1, 10, 10), ent(0, 11, 10), ent(1, 12, 10)]), OPEN, 4, 2)
    for w, r2, far in ((KNIFE, 2, (2, 0)), (AXE, 2, (2, 0)), (GUN, 36, (6, 1)), (RIFLE, 100, (10, 1)), (SHOTGUN, 9, (3, 1))):
        edge = {2: (1, 1), 36: (6, 0), 100: (10, 0), 9: (3, 0)}[r2]
        assert edge[0] ** 2 + edge[1] ** 2 == r2 and far[0] ** 2 + far[1] ** 2 in (r2 + 1, r2 + 2)
        c["range_w%d" % w] = (View(1, 0, [ent(1, 20, 20, 100, w), ent(1, 20 + edge[0], 20 + edge[1]),
                                          ent(1, 20 - far[0], 20 - far[1])]), OPEN, 4, 1)
    # healing: d2 9 and 10; slot 1 an agent with a gun, slot 2 a bot
    c["heal"] = (View(2, 1, [ent(1, 10, 10), ent(1, 13, 10, 50, GUN), ent(1, 9, 13, 60, AXE)]), OPEN, 1, 2)
    # rays on a 12 x 30 map from (5, 5): +y capped (16 free cells of 24), -x the edge after 5, -y a present obstacle
    # at 2 (the encoder takes no obstacle life at all: a destroyed obstacle that is still present stops the ray as a
    # live one does, which the GPU rows with poked lives exercise), +x a cleaned-up obstacle passed and a live one at 4
    st = EO.Static(12, 30, [(5, 2), (7, 5), (10, 5)], [])
    c["rays"] = (View(1, 0, [ent(1, 5, 5), ent(1, 5, 7), ent(1, 6, 5)], [1, 0, 1]), st, 4, 1)
    st = EO.Static(20, 20, [], [(12, 10), (10, 8), (10, 12), (0, 0)])
    c["objective_tie"] = (View(1, 0, [ent(1, 10, 10)]), st, 1, 0)
    c["on_objective"] = (View(2, 0, [ent(1, 10, 8), ent(1, 1, 1)]), st, 1, 1)
    c["life_saturates"] = (View(1, 1, [ent(1, 10, 10, -40000), ent(1, 11, 10, 40000), ent(1, 12, 10, -32769)]), OPEN, 1, 1)
    c["no_objectives"] = (View(1, 0, [ent(1, 0, 0)]), EO.Static(1, 1), 1, 0)
    return c


CASES = _cases()


def test_tie_lower_slot_first():
    rows = EO.encode(*CASES["tie"])
    assert zrow(rows, 0, 0) == [2, 0, 7, 1 | 2] and zrow(rows, 0, 1) == [0, -2, 9, 1 | 2] and zrow(rows, 0, 2) == [-2, 0, 5, 1 | 2]
    assert zrow(rows, 0, 3) == [0, 0, 0, 0]


def test_kz_plus_one_is_cut():
    rows = EO.encode(*CASES["kz_plus_one"])
    assert [zrow(rows, 0, i)[0] for i in range(4)] == [1, 2, 3, 4]
    assert [zrow(rows, 0, i)[2] for i in range(4)] == [11, 12, 13, 14]
    assert zrow(rows, 0, 0)[3] == 1 | 2 | 4  # adjacent
    assert int(rows[0][6]) == 5  # all five are counted


def test_no_zombies_absent_and_lone_agents():
    rows = EO.encode(*CASES["no_zombies"])
    assert all(zrow(rows, 0, i) == [0, 0, 0, 0] for i in range(4)) and int(rows[0][6]) == 0
    assert [int(v) for v in rows[0][:8]] == [1, 10, 10, 100, RIFLE, 100, 0, 0]
    rows = EO.encode(*CASES["absent_agent"])
    assert not rows[0].any() and rows[1][0] == 1
    assert prow(rows, 1, 0) == [0, 0, 0, 0] and int(rows[1][7]) == 0  # the absent agent is no player row
    rows = EO.encode(*CASES["lone_agent"])
    assert prow(rows, 0, 0, 4, 2) == [0, 0, 0, 0] and prow(rows, 0, 1, 4, 2) == [0, 0, 0, 0] and int(rows[0][7]) == 0
    assert zrow(rows, 0, 0, 4, 2)[:2] == [2, 0]


@pytest.mark.parametrize("w,r2", [(KNIFE, 2), (AXE, 2), (GUN, 36), (RIFLE, 100), (SHOTGUN, 9)])
def test_weapon_range_edge(w, r2):
    rows = EO.encode(*CASES["range_w%d" % w])
    assert int(rows[0][4]) == w and int(rows[0][5]) == r2
    near, far = zrow(rows, 0, 0), zrow(rows, 0, 1)
    assert near[0] ** 2 + near[1] ** 2 == r2 and near[3] & 2
    assert far[0] ** 2 + far[1] ** 2 > r2 and not far[3] & 2 and far[3] & 1


def test_healing_range_and_player_flags():
    rows = EO.encode(*CASES["heal"])
    assert prow(rows, 0, 0, 1, 2) == [3, 0, 50, 1 | 2 | 4 | GUN << 8]  # d2 = 9, an agent
    assert prow(rows, 0, 1, 1, 2) == [-1, 3, 60, 1 | AXE << 8]  # d2 = 10, a bot
    assert int(rows[0][7]) == 2


def test_rays():
    rows = EO.encode(*CASES["rays"])
    assert block(rows, 0, "rays") == [16, 5, 2, 4]
    v, st, kz, kp = CASES["rays"]
    gone = View(1, 0, [tuple(e) for e in v.ent], [0, 0, 0])
    assert block(EO.encode(gone, st, kz, kp), 0, "rays") == [16, 5, 5, 6]  # -y now reaches the edge, +x too


def test_objectives():
    rows = EO.encode(*CASES["objective_tie"])
    assert block(rows, 0, "objective", 1, 0) == [2, 0, 1, 4]  # three at d2 = 4: the first of the map file
    rows = EO.encode(*CASES["on_objective"])
    assert block(rows, 0, "objective", 1, 1) == [0, 0, 1 | 2, 4] and block(rows, 1, "objective", 1, 1) == [-1, -1, 1, 4]
    rows = EO.encode(*CASES["no_objectives"])
    assert block(rows, 0, "objective", 1, 0) == [0, 0, 0, 0] and block(rows, 0, "rays", 1, 0) == [0, 0, 0, 0]


def test_lives_saturate():
    rows = EO.encode(*CASES["life_saturates"])
    assert int(rows[0][3]) == -32768 and prow(rows, 0, 0, 1, 1)[2] == 32767 and zrow(rows, 0, 0, 1, 1)[2] == -32768


# ---- the header's rule functions, as a program ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    cxx = shutil.which("clang++") or shutil.which("g++") or shutil.which("c++")
    if cxx is None and os.path.exists("/opt/rocm/llvm/bin/clang++"):
        cxx = "/opt/rocm/llvm/bin/clang++"
    assert cxx, "a host C++ compiler"
    exe = str(tmp_path_factory.mktemp("entity_obs") / "entity_obs_host")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "libzombsole_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "entity_obs_host.cpp")])
    return exe


def _run_host(exe, cases, tmp_path, name):
    path = tmp_path / (name + ".txt")
    path.write_text(EC.host_text(cases))
    out = subprocess.check_output([exe, str(path)], text=True).splitlines()
    assert len(out) == len(cases)
    return [np.array(line.split(), dtype=np.int64).astype(np.int16).reshape(c[0].A, -1) for line, c in zip(out, cases)]


def test_host_program_equals_encode_on_the_hand_built_states(host_program, tmp_path):
    names = sorted(CASES)
    cases = [CASES[n] for n in names] + [(CASES[n][0], CASES[n][1], kz, kp) for n in names for kz, kp in EC.KS]
    got = _run_host(host_program, cases, tmp_path, "hand")
    for i, (c, g) in enumerate(zip(cases, got)):
        want = EO.encode(*c)
        assert g.shape == want.shape and np.array_equal(g, want), (i, names[i % len(names)], c[2:], g.tolist(), want.tolist())


@pytest.mark.parametrize("row", EC.ROWS)
def test_host_program_equals_encode_on_the_oracle_states(host_program, tmp_path, row):
    """The oracle's states of a GPU row (13 envs, every fourth step and the last): the program's rows are encode's, at
    every K pair; the (4, 1) and (1, 0) rows are the (16, 16) rows' first ones."""
    states, _census = EC.oracle_trace(row, 13)
    b = EC.builder(row, 1)
    static = EO.Static.of_map(b.map)
    ts = sorted(set(range(0, len(states), 4)) | {len(states) - 1})
    envs = range(13) if row != "fort_e132" else range(3)
    views = [EC.oracle_view(b, states[t][k]) for t in ts for k in envs]
    cases = [(v, static, kz, kp) for v in views for kz, kp in EC.KS]
    got = _run_host(host_program, cases, tmp_path, row)
    full = None
    for c, g in zip(cases, got):
        want = EO.encode(*c)
        assert np.array_equal(g, want), (row, c[2:])
        if c[2:] == (16, 16):
            full = want
    for v in views[:5]:
        full = EO.encode(v, static, 16, 16)
        for kz, kp in EC.KS:
            assert np.array_equal(EC.slice_rows(full, kz, kp), EO.encode(v, static, kz, kp))


# ---- three wrong rules, as programs: each must change named hand-built cases and no other ------------------------------
MUTANTS = {
    "tie_by_higher_slot": ("zs_entity_obs.hpp", "return da < db || (da == db && sa < sb);", "return da < db || (da == db && sa > sb);",
                           {"tie"}),
    "range_lt": ("zs_entity_obs.hpp", "(d2 <= r2 ? ZS_ENT_IN_RANGE : 0)", "(d2 < r2 ? ZS_ENT_IN_RANGE : 0)",
                 {"range_w%d" % w for w in (KNIFE, AXE, GUN, RIFLE, SHOTGUN)}),
    "rays_stopped_by_entities": ("entity_obs_host.cpp", "if (o.x == cx && o.y == cy && o.present) return true;",
                                 "if (o.x == cx && o.y == cy && o.present) return true;\n"
                                 "            for (const auto& t : ent) if (t.present && t.x == cx && t.y == cy) return true;",
                                 {"rays", "tie", "kz_plus_one", "lone_agent", "heal", "life_saturates", "absent_agent"}
                                 | {"range_w%d" % w for w in (KNIFE, AXE, GUN, RIFLE, SHOTGUN)}),  # a thing on an axis
}


@pytest.mark.parametrize("name", sorted(MUTANTS))
def test_a_wrong_rule_changes_the_named_cases(name, tmp_path):
    """The header (or the program's obstacle test) with one rule changed, built as a program: its rows differ from
    encode's on exactly the hand-built cases that hold the rule's case."""
    fname, old, new, expect = MUTANTS[name]
    srcs = {"zs_entity_obs.hpp": os.path.join(ROOT, "libzombsole_amd", "csrc", "zs_entity_obs.hpp"),
            "entity_obs_host.cpp": os.path.join(ROOT, "tests", "entity_obs_host.cpp")}
    for f, path in srcs.items():
        text = open(path).read()
        if f == fname:
            assert text.count(old) == 1, (name, "the rule's text is in the source once")
            text = text.replace(old, new)
        (tmp_path / f).write_text(text)
    cxx = shutil.which("clang++") or shutil.which("g++") or shutil.which("c++") or "/opt/rocm/llvm/bin/clang++"
    exe = str(tmp_path / "mutant")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-I", str(tmp_path), "-I", os.path.join(ROOT, "libzombsole_amd", "csrc"),
                           "-o", exe, str(tmp_path / "entity_obs_host.cpp")])
    names = sorted(CASES)
    got = _run_host(exe, [CASES[n] for n in names], tmp_path, name)
    differ = {n for n, g in zip(names, got) if not np.array_equal(g, EO.encode(*CASES[n]))}
    assert differ == expect, (name, sorted(differ))
