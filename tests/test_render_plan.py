"""The render feature's host side on the CPU: the record layouts of the flag combinations (unflagged numbers unchanged),
the fingerprints, the builders' flag, and csrc/zs_render.hpp compiled into a stand-alone program under AddressSanitizer
and UBSan (tests/render_plan_host.cpp: the C++ rasteriser against the recorded atlas, the per-pixel rule against
render.compose, the launch plan, the tracker's rule)."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import golden_util as G
import render_cases as RC
from libzombsole_amd import _abi
from libzombsole_amd import render as R

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _cfg(**kw):
    return _abi.multi_env_config(4, "extermination", ["terminator"], "bridge", ["0", "1"], initial_zombies=10, minimum_zombies=5, **kw)


def test_the_builders_set_the_flag_with_the_death_log():
    assert not _cfg().cfg.flags & (_abi.FLAG_RENDER | _abi.FLAG_DEATH_LOG)
    f = _cfg(render=True).cfg.flags
    assert f & _abi.FLAG_RENDER and f & _abi.FLAG_DEATH_LOG
    assert _abi.FLAG_RENDER == 64


@pytest.mark.parametrize("env_params", [False, True])
@pytest.mark.parametrize("episode_stats", [False, True])
def test_record_layout_of_every_flag_combination(env_params, episode_stats):
    plain = _cfg(env_params=env_params, episode_stats=episode_stats)
    flagged = _cfg(env_params=env_params, episode_stats=episode_stats, render=True)
    L0, L1 = plain.snapshot_layout(), flagged.snapshot_layout()
    W, H = plain.map.size
    body = (W * H + 15) & ~15
    assert "body_col" not in L0
    for k, v in L0.items():
        if k not in ("pad", "rec_bytes", "fingerprint"):
            assert L1[k] == v, k  # every section before it is where it was
    assert L1["body_col"] == L0["pad"] and L1["body_bytes"] == body and L1["pad"] == L0["pad"] + body
    assert L1["rec_bytes"] == (L1["pad"] + 15) // 16 * 16
    assert L1["fingerprint"] != L0["fingerprint"]


def test_unflagged_layout_numbers_are_what_they_were():
    # the bridge config's record before this feature (E = 13, O = 274 on the bundled bridge map)
    L = _cfg().snapshot_layout()
    b = _cfg()
    E, O = 13, len(b.map.obstacles)
    W, H = b.map.size
    DW, OW = (W * H + 31) // 32, (O + 31) // 32
    words = 1248 + DW + O + 2 * OW + 3 * E + 9 + 3 + 2
    assert L["weapon"] == 4 * words and L["pad"] == 4 * words + 3 * E + 2
    assert L == dict(_abi.snapshot_layout(E, O, DW, OW, 2), fingerprint=L["fingerprint"])


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    cxx = shutil.which("clang++") or shutil.which("g++") or shutil.which("c++")
    if cxx is None and os.path.exists("/opt/rocm/llvm/bin/clang++"):
        cxx = "/opt/rocm/llvm/bin/clang++"
    assert cxx, "a host C++ compiler"
    exe = str(tmp_path_factory.mktemp("render_plan") / "render_plan_host")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "libzombsole_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "render_plan_host.cpp")])
    return exe


def test_host_program_atlas_plan_pixels_and_tracker(host_program, tmp_path):
    rec = RC.recorded_atlas()
    out = json.loads(subprocess.check_output([host_program], text=True))
    masks, palette = R.default_atlas()
    assert out["masks"] == [[int(w) for w in m] for m in masks]
    assert out["rgb"][:6] == [int(p[0]) | int(p[1]) << 8 | int(p[2]) << 16 for p in palette[:6]]
    assert [sum(bin(w).count("1") for w in m) for m in out["masks"]] == [rec["pixels"][s] for s in R.SHAPES]
    # the plan: every band within the LDS the kernel may ask for, the bands cover the rows
    for W, H, rows, bands, lds, body in out["plans"]:
        assert bands == -(-H // rows) and 1 <= rows <= H and lds <= 64 * 1024 and body == (W * H + 15) & ~15 and body >= W * H
        assert lds >= 112 + (W + 1) * (rows + 1)
    # the per-pixel rule over a crowded 5 x 4 world against compose
    w = out["world"]
    ents = [(x, y, c) for x, y, c in w["entities"]]
    frame = R.compose(w["W"], w["H"], ents, [tuple(o) for o in w["obstacles"]], [tuple(b) for b in w["bodies"]],
                      [tuple(o) for o in w["objectives"]])
    got = np.array(w["frame"], dtype=np.uint32).reshape(10 * w["H"], 10 * w["W"])
    exp = frame[..., 0].astype(np.uint32) | frame[..., 1].astype(np.uint32) << 8 | frame[..., 2].astype(np.uint32) << 16
    assert np.array_equal(got, exp)
    # the tracker: the later death of a cell wins, entries off the map or of no slot are skipped
    assert out["track"] == w["track_expected"]


@pytest.mark.parametrize("row", sorted(RC.ROWS))
def test_census_of_the_gpu_rows_by_the_oracle_alone(row):
    """Every class a GPU row is relied on for shows in three envs or more of its 13, in the oracle's run (its state and
    its death log; the body colours accumulated in Python)."""
    _frames, census = RC.oracle_trace(row, 13, RC.steps_of(row), False)
    count = {c: sum(c in s for s in census) for c in RC.CLASSES}
    for c in sorted(RC.REQUIRED[row]):
        assert count[c] >= 3, (row, c, count)


def test_every_class_has_a_row():
    assert set().union(*RC.REQUIRED.values()) == set(RC.CLASSES)
    assert set(RC.REQUIRED) == set(RC.ROWS)
