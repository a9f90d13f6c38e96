"""csrc/zs_nav.hpp on the host: the rule functions, built by the host compiler into a stand-alone program
(tests/nav_host.cpp) that runs the bit-row level loop on the CPU, against libzombsole_amd/nav.py on every row of the
case table, plain and under AddressSanitizer and UBSan; nav_plan() for every bundled map, at the boundaries where 4, 2
and 1 envs share a workgroup, and at the first size that is refused; the header, the binding table and the build list."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import nav_cases as NC
from entity_obs_cases import View, ent
from libzombsole_amd import _abi
from libzombsole_amd import engine
from libzombsole_amd import nav as NV
from libzombsole_amd.entity_obs import Static
from libzombsole_amd.maps import available_maps, load_map

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
LIMIT = 65536


def _cxx():
    cxx = shutil.which("clang++") or shutil.which("g++") or shutil.which("c++")
    if cxx is None and os.path.exists("/opt/rocm/llvm/bin/clang++"):
        cxx = "/opt/rocm/llvm/bin/clang++"
    assert cxx, "a host C++ compiler"
    return cxx


def _build(tmp, name, extra):
    exe = str(tmp / name)
    subprocess.check_call([_cxx(), "-std=c++17", "-O1", "-g"] + extra + ["-I", os.path.join(ROOT, "libzombsole_amd", "csrc"),
                                                                       "-o", exe, os.path.join(ROOT, "tests", "nav_host.cpp")])
    return exe


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("nav_host")
    return {"plain": _build(tmp, "nav_host", []),
            "sanitized": _build(tmp, "nav_host_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])}


def env_bytes(W, H, A):
    """The issue's image: free, and visited and two frontiers per field, of H * ceil(W / 32) words; 5 A query cells
    (int32) and their distances (int16 per field); rounded up to 16."""
    return (4 * H * ((W + 31) // 32) * 7 + (4 + 2 * 2) * 5 * A + 15) // 16 * 16


def plan(exe, shapes):
    out = subprocess.check_output([exe, "plan"] + [str(v) for s in shapes for v in s], text=True).splitlines()
    keys = ("ok", "ww", "nw", "nq", "env_bytes", "envs_per_wg", "block", "lds_bytes")
    return [dict(zip(keys, (int(v) for v in line.split()))) for line in out]


def _hand_cases():
    st = Static(5, 4, [], [(2, 1)])
    v = View(6, 0, [ent(1, 0, 0), ent(1, 2, 1), ent(1, 2, 0), ent(1, 0, 2), ent(1, 4, 1), ent(0, 2, 3), ent(1, 4, 3)])
    st2 = Static(6, 1, [(0, 0), (3, 0)], [(0, 0), (1, 0)])
    v2 = View(1, 0, [ent(1, 2, 0), ent(1, 5, 0)], [1, 1])
    v3 = View(1, 0, [ent(1, 2, 0), ent(1, 5, 0)], [0, 0])
    return [(v, st, f, cap) for f in (1, 2, 3) for cap in (1, 2, NV.MAX_DIST)] + \
           [(x, st2, f, cap) for x in (v2, v3) for f in (1, 2, 3) for cap in (1, 2, NV.MAX_DIST)]


def _run(exe, cases, tmp_path, name):
    path = tmp_path / (name + ".txt")
    path.write_text(NC.host_text(cases))
    lines = subprocess.check_output([exe, "cases", str(path)], text=True).splitlines()
    got, i = [], 0
    for v, st, fields, _cap in cases:
        F = bin(fields).count("1")
        rows = np.array(lines[i].split(), dtype=np.int64).astype(np.int16).reshape(v.A, F, 8)
        frames = [np.array(lines[i + 1 + f].split(), dtype=np.int64).astype(np.uint16).reshape(st.H, st.W) for f in range(F)]
        got.append((rows, frames))
        i += 1 + F
    assert i == len(lines)
    return got


def _check(cases, got, what):
    for c, (rows, frames) in zip(cases, got):
        v, st, fields, cap = c
        assert np.array_equal(rows, NV.encode(v, st, fields, cap)), (what, fields, cap)
        for b, frame in zip(NV.field_bits(fields), frames):
            assert np.array_equal(frame, NV.field(v, st, b, cap)), (what, fields, cap, b)


@pytest.mark.parametrize("build", ["plain", "sanitized"])
def test_host_program_equals_the_model_on_the_hand_built_states(programs, tmp_path, build):
    cases = _hand_cases()
    _check(cases, _run(programs[build], cases, tmp_path, "hand"), "hand")


@pytest.mark.parametrize("build", ["plain", "sanitized"])
@pytest.mark.parametrize("row", sorted(NC.ROWS))
def test_host_program_equals_the_model_on_the_oracle_states(programs, tmp_path, row, build):
    """The oracle's states of a row (the reset, the middle and the last step; five envs): the program's rows and fields
    are the model's, for every field mask and every cap of the row."""
    views, _s, _c = NC.oracle_trace(row, 13)
    static = Static.of_map(NC.builder(row, 1).map)
    ts = sorted({0, len(views) // 2, len(views) - 1})
    cases = [(views[t][k], static, f, cap) for t in ts for k in (range(5) if row != "fort_e132" else range(2))
             for f in (1, 2, 3) for cap in NC.caps_of(row)]
    _check(cases, _run(programs[build], cases, tmp_path, row), row)


def test_plan_of_every_bundled_map(programs):
    shapes = [tuple(load_map(n).size) + (a,) for n in available_maps() for a in (1, 4, 32)]
    for s, p in zip(shapes, plan(programs["sanitized"], shapes)):
        W, H, A = s
        assert p["ok"] == 1 and p["ww"] == (W + 31) // 32 and p["nw"] == H * p["ww"] and p["nq"] == 5 * A
        assert p["env_bytes"] == env_bytes(W, H, A) and p["envs_per_wg"] == 4 and p["block"] == 256, s  # several times over
        assert p["lds_bytes"] == 4 * p["env_bytes"] <= LIMIT
    city = plan(programs["plain"], [(128, 128, 1)])[0]
    assert 4 * city["nw"] == 2048  # 2 KiB per array


def _boundary(epw):
    """The largest H at W = 32, A = 1 at which epw envs' images fit the limit."""
    H = 1
    while epw * env_bytes(32, H + 1, 1) <= LIMIT:
        H += 1
    return H


def first_refused():
    """(W, H): the first height at W = 32, A = 1 whose single-env image is past the limit."""
    return 32, _boundary(1) + 1


def test_plan_boundaries_and_the_first_refused_size(programs):
    h4, h2, h1 = _boundary(4), _boundary(2), _boundary(1)
    assert h4 < h2 < h1
    shapes = [(32, h4, 1), (32, h4 + 1, 1), (32, h2, 1), (32, h2 + 1, 1), (32, h1, 1), (32, h1 + 1, 1), (16000, 1000, 1),
              (1, 1, 1), (1, 1, 254), (33, h4 // 2 + 1, 1), (32, h4, 2)]
    got = plan(programs["sanitized"], shapes)
    assert [p["envs_per_wg"] for p in got[:6]] == [4, 2, 2, 1, 1, 0]
    assert [p["ok"] for p in got] == [1, 1, 1, 1, 1, 0, 0, 1, 1, 1, 1]
    assert got[10]["envs_per_wg"] == 2  # the queries of a second agent tip the boundary shape over
    assert first_refused() == (32, h1 + 1) and got[5] == dict.fromkeys(got[5], 0) | {"ww": 1}
    for s, p in zip(shapes, got):
        assert p["lds_bytes"] <= LIMIT and p["block"] == 64 * p["envs_per_wg"], s
        if p["ok"]:
            assert p["lds_bytes"] == p["envs_per_wg"] * env_bytes(*s) and p["envs_per_wg"] in (4, 2, 1)
            assert p["envs_per_wg"] == 4 or 2 * p["envs_per_wg"] * env_bytes(*s) > LIMIT  # as many envs as fit


def test_the_header_the_bindings_and_the_build_list():
    src = open(os.path.join(ROOT, "include", "zombsole_mi355x.h")).read()
    for s in ("zs_nav_plan", "zs_nav_obs", "zs_nav_field", "zs_nav_bind"):
        assert re.search(r"^int %s\(" % s, src, re.M) and s in engine.SYMBOLS and s in _abi.ABI
    for name, val in (("ZS_NAV_OBJECTIVE", NV.OBJECTIVE), ("ZS_NAV_ZOMBIES", NV.ZOMBIES), ("ZS_NAV_MAX_DIST", NV.MAX_DIST)):
        assert "#define %s %d" % (name, val) in src
    hpp = open(os.path.join(ROOT, "libzombsole_amd", "csrc", "zs_nav.hpp")).read()
    assert "#define ZS_NAV_ROW_WORDS %d" % NV.ROW_WORDS in hpp and "#define ZS_NAV_LDS_LIMIT %d" % LIMIT in hpp
    assert len(_abi.NAV_PLAN_KEYS) == 8
    import __graft_entry__ as ge
    assert ("k_nav.hip", [], "k_nav") in ge.UNITS
    L = engine.load_library()
    assert L.zs_nav_obs.argtypes is not None and hasattr(L, "zs_nav_bind")
