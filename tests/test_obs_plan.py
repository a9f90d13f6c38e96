"""The observation plan (libzombsole_amd/csrc/zs_obs_plan.hpp) on the CPU: the header compiled with the host
compiler into tests/obs_plan_dump.cpp, every (shape, overrides) pair of obs_plan_table against the launch
parameters the engine used before the plan existed (obs_plan_expected.json)."""
import json
import os
import subprocess

import pytest

import obs_plan_table as T
from libzombsole_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL_KEYS = ("kind", "nobs", "patched", "grid", "block", "lds", "stat", "us")


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    """plan(pairs, refuse) -> one resolved row per (shape name, overrides) pair."""
    exe = tmp_path_factory.mktemp("obs_plan") / "obs_plan_dump"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "libzombsole_amd", "csrc"),
                           "-o", str(exe), os.path.join(ROOT, "tests", "obs_plan_dump.cpp")])

    def run(pairs, refuse=False):
        lines = []
        for shape, lo in pairs:
            mk, n = T.SHAPES[shape]
            ints = [int(refuse)] + T.shape_ints(mk(n), lo) + [int(lo.get(f, 0)) for f in _abi.LAUNCH_FIELDS]
            lines.append(" ".join(str(v) for v in ints))
        out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True)
        rows = [json.loads(l) for l in out.stdout.splitlines()]
        assert len(rows) == len(pairs)
        return rows
    return run


PAIRS = [(shape, lo) for shape in T.SHAPES for lo in T.overrides().values()]


def test_launch_fields_are_the_headers():
    """obs_plan_dump.cpp fills zs_launch as 22 consecutive int32 in _abi.LAUNCH_FIELDS' order (the order
    test_abi.py checks against the header)."""
    assert len(_abi.LAUNCH_FIELDS) == 22
    assert [f[0] for f in _abi.zs_launch._fields_[:22]] == _abi.LAUNCH_FIELDS


def test_rows_match_the_table(plan):
    rows = plan(PAIRS)
    bad = []
    for (shape, lo), got in zip(PAIRS, rows):
        exp = T.expected(shape, lo)
        for which in ("full", "masked"):
            if {k: got[which][k] for k in KERNEL_KEYS} != {k: exp[which][k] for k in KERNEL_KEYS}:
                bad.append((shape, lo, which, got[which], exp[which]))
        if (got["obs_stat"], got["fobs"], got["step_img_bytes"]) != (exp["obs_stat"], exp["fobs"], exp["step_img_bytes"]):
            bad.append((shape, lo, "step", got, exp))
    assert not bad, bad[:5]


@pytest.mark.parametrize("shape,lo,kernel", [("c2@65536", {}, "k_obs_ring"),
                                             ("c5@64", {}, "k_obs_ring"), ("c5@4097", {}, "k_obs_ring"),
                                             ("c5@65536", {}, "k_obs_ring"),
                                             ("c4@24", {}, "k_obs_pbring"), ("c4@16384", {}, "k_obs_pbring"),
                                             ("c4@24", {"obs_ring": -1}, "k_obs_gather"),
                                             ("c4@16384", {"obs_ring": -1}, "k_obs_gather")])
def test_default_picks(plan, shape, lo, kernel):
    """The kernels test_fullsize_parity.py asserts on the GPU at the bench's sizes."""
    row, = plan([(shape, lo)])
    assert row["full"]["name"] == kernel and not row["fobs"]
    assert T.expected_describe(shape, lo)[0] == kernel


def test_fallbacks_are_total(plan):
    """No kernel may have its dynamic-LDS limit raised: every pair still resolves, to kernels within the
    64 KiB every kernel may use."""
    for (shape, lo), row in zip(PAIRS, plan(PAIRS, refuse=True)):
        assert "error" not in row, (shape, lo)
        for which in ("full", "masked"):
            assert row[which]["name"] in T.KERNEL_NAMES and 0 < row[which]["lds"] <= 64 * 1024, (shape, lo, row)
