"""The scripted policies' host side on the CPU: the unit, the three symbols, the policy constants, and
csrc/zs_autopilot.hpp's rule functions compiled as a stand-alone program under AddressSanitizer and UBSan
(tests/autopilot_host.cpp), which prints the fixtures' triples."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

import golden_util as G
import pilot_census as PC
from libzombsole_amd import _abi
from libzombsole_amd import autopilot as AP
from libzombsole_amd import engine

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SYMBOLS = ("zs_autopilot", "zs_autopilot_bind")


def test_the_kernel_is_a_unit_of_its_own():
    import __graft_entry__ as ge
    assert ("k_autopilot.hip", [], "k_autopilot") in ge.UNITS
    assert os.path.isfile(os.path.join(ge.CSRC, "k_autopilot.hip"))


def test_the_header_the_binding_and_the_library_name_the_calls():
    src = open(os.path.join(ROOT, "include", "zombsole_mi355x.h")).read()
    L = engine.load_library()
    for s in SYMBOLS:
        assert re.search(r"^int %s\(" % s, src, re.M) and s in _abi.ABI and s in engine.SYMBOLS
        assert ctypes.cast(getattr(L, s), ctypes.c_void_p).value and getattr(L, s).argtypes is not None
    assert len(_abi.ABI["zs_autopilot"]) == 5 and len(_abi.ABI["zs_autopilot_bind"]) == 3
    out = subprocess.check_output(["nm", "-D", "--defined-only", engine.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(SYMBOLS) <= exported and any("k_autopilot" in s for s in exported)
    assert '"autopilot_bound"' in src  # zs_describe's new word


def test_the_policy_constants_agree():
    src = open(os.path.join(ROOT, "include", "zombsole_mi355x.h")).read()
    got = {n.lower(): int(v) for n, v in re.findall(r"^#define ZS_PILOT_(\w+) (\d+)$", src, re.M)}
    assert got == AP.POLICIES == {"none": 0, "terminator": 1, "sniper": 2, "troll": 3}
    assert (AP.NONE, AP.TERMINATOR, AP.SNIPER, AP.TROLL) == (0, 1, 2, 3)
    hpp = open(os.path.join(ROOT, "libzombsole_amd", "csrc", "zs_autopilot.hpp")).read()
    # adjacent_positions order, stated once for the device and once for numpy
    assert "return k == 2 ? 1 : k == 3 ? -1 : 0;" in hpp and "return k == 0 ? 1 : k == 1 ? -1 : 0;" in hpp
    assert AP.ADJACENT == ((0, 1), (0, -1), (1, 0), (-1, 0))


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    cxx = shutil.which("clang++") or shutil.which("g++") or shutil.which("c++")
    if cxx is None and os.path.exists("/opt/rocm/llvm/bin/clang++"):
        cxx = "/opt/rocm/llvm/bin/clang++"
    assert cxx, "a host C++ compiler"
    exe = str(tmp_path_factory.mktemp("autopilot") / "autopilot_host")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "libzombsole_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "autopilot_host.cpp")])
    return exe


@pytest.mark.parametrize("name", PC.pilot_fixture_names())
def test_the_rule_functions_print_the_fixtures_triples(host_program, tmp_path, name):
    fx = G.load_fixture(name)
    st_map = PC.static_of(fx)
    n = PC.n_agents(fx)
    cases, want = [], []
    for run in fx["runs"]:
        for c, (rec, pl) in enumerate(zip(run["calls"], run["pilot"])):
            view = PC.View(rec["state"], fx, st_map)
            for k, pname in enumerate(PC.POLICY_NAMES):
                cases.append((view, st_map, [k + 1] * n))
                want.append(pl[pname])
            codes = [(a + c) % 5 for a in range(n)]  # 0 (not written) and 4 (no policy: idle) among them
            cases.append((view, st_map, codes))
            want.append([[-9] * 3 if k == 0 else [0, 0, 0] if k == 4 else pl[PC.POLICY_NAMES[k - 1]][a]
                         for a, k in enumerate(codes)])
    path = tmp_path / (os.path.basename(name) + ".txt")
    path.write_text(PC.host_text(cases))
    out = subprocess.check_output([host_program, str(path)], text=True).splitlines()
    assert len(out) == len(cases)
    for i, (line, w) in enumerate(zip(out, want)):
        got = [int(v) for v in line.split()]
        assert got == [v for t in w for v in t], (name, i, got, w)
