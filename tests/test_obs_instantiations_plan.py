"""The case table of obs_instantiations.py on the CPU: the observation plan (libzombsole_amd/csrc/zs_obs_plan.hpp,
compiled with the host compiler into tests/obs_plan_dump.cpp as test_obs_plan.py does) resolves every row's
(config, overrides) to exactly the instantiation the row claims, and the rows together with the justified
unreachable ones are the 57 device functions of k_obs_t.hip."""
import json
import os
import subprocess

import pytest

import obs_instantiations as I
import obs_plan_table as T
from libzombsole_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "libzombsole_amd", "csrc")


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    """plan(rows) -> the resolved plan of each row's (config, overrides)."""
    exe = tmp_path_factory.mktemp("obs_inst_plan") / "obs_plan_dump"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-o", str(exe),
                           os.path.join(ROOT, "tests", "obs_plan_dump.cpp")])

    def run(rows):
        lines = []
        for r in rows:
            ints = [0] + T.shape_ints(r.builder(), r.launch) + [int(r.launch.get(f, 0)) for f in _abi.LAUNCH_FIELDS]
            lines.append(" ".join(str(v) for v in ints))
        out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True)
        got = [json.loads(l) for l in out.stdout.splitlines()]
        assert len(got) == len(rows)
        return got
    return run


def test_rows_resolve_to_their_instantiation(plan):
    bad = []
    for r, p in zip(I.ROWS, plan(I.ROWS)):
        assert "error" not in p, r.id
        full, masked = p["full"], p["masked"]
        if (full["kind"], full["nobs"], full["patched"]) != (r.kind, r.nobs, r.patched):
            bad.append((r.id, "full", full))
        if (full["name"], full["encoders"]) != (r.obs_kernel, r.obs_encoders):
            bad.append((r.id, "names", full))
        if (masked["kind"], masked["nobs"], masked["name"]) != (r.masked_kind, r.masked_nobs, r.obs_kernel_masked):
            bad.append((r.id, "masked", masked))
        if (full["grid"], full["block"]) != (r.grid, r.block):  # one ring unit (ring_pair envs) per workgroup
            bad.append((r.id, "geometry", full, r.grid, r.block))
        if p["fobs"]:  # the step launch would write the observations and the kernel run only resets and observes
            bad.append((r.id, "fobs", p["fobs"]))
    assert not bad, bad


def test_rows_cover_all_57():
    every = I.all_instantiations()
    assert len(every) == len(set(every)) == 57
    rows = [(r.variant, r.dtype_name, r.nobs) for r in I.ROWS]
    assert len(rows) == len(set(rows))
    assert not set(rows) & set(I.UNREACHABLE)
    assert set(rows) | set(I.UNREACHABLE) == set(every)
    assert len(rows) + len(I.UNREACHABLE) == 57
    # masked launches: k_obs told each count, and k_obs_gather, at every dtype x count
    for kernel in ("k_obs", "k_obs_gather"):
        got = {(r.dtype_name, r.masked_nobs) for r in I.ROWS if r.obs_kernel_masked == kernel and r.masked_nobs}
        assert got == {(dt, n) for dt in I.DTYPES for n in (1, 2, 4)}, kernel


def test_unreachable_quote_the_plan():
    """Every unreachable entry quotes a condition that stands in obs_plan(), and the arithmetic next to the
    list holds: the ring of four int64 or int32 blocks is larger than the plan's limit before anything else
    is added, so no shape or override admits it."""
    with open(os.path.join(CSRC, "zs_obs_plan.hpp")) as f:
        src = f.read()
    for key, cond in I.UNREACHABLE.items():
        assert cond and cond in src, key
    assert "#define RING_SLOTS 8" in src

    def slot_bytes(ts, nblk):  # obs_stage_slot_bytes
        return ((nblk * 3 * 441 + 16 // ts) * (4 if ts == 8 else ts) + 15) // 16 * 16

    def pair(ts, nobs):  # ring_pair
        return 2 if (nobs * 1323 * ts) % 16 and not (2 * nobs * 1323 * ts) % 16 else 1

    size = {"i64": 8, "i32": 4, "i16": 2}
    for v in ("ring_patched", "ring_select"):
        for dt in I.DTYPES:
            for nobs in (1, 2, 4):
                ts, pr = size[dt], pair(size[dt], nobs)
                ring = (8 // pr) * slot_bytes(ts, nobs * pr)
                assert (ring > 160 * 1024) == ((v, dt, nobs) in I.UNREACHABLE), (v, dt, nobs, ring)


def test_unreachable_under_the_ring_overrides(plan):
    """What the ring's overrides reach where the ring does not fit: k_obs_patch (its rows are in the table)."""
    rows = [I.Row(v, dt, 4, "bridge64", 37) for (v, dt, _) in I.UNREACHABLE]
    for r, p in zip(rows, plan(rows)):
        assert p["full"]["name"] == "k_obs_patch", (r.id, p["full"])


def test_ring_pair_edges():
    """The rows the layout edges need: an odd env count wherever two envs make a ring unit."""
    for r in I.ROWS:
        assert 2 <= r.n <= 130
        if r.variant in ("ring_patched", "ring_select", "pbring") and (r.dtype_name, r.nobs) in I.UNIT_ENVS:
            assert r.n % 2 == 1 and r.envs_per_wg == 2, r.id
    assert {r.map_name for r in I.ROWS} == {"bridge64", "wall_hp"}
    for v in I.VARIANTS:  # every variant meets both maps
        assert {r.map_name for r in I.ROWS if r.variant == v} == {"bridge64", "wall_hp"}, v
