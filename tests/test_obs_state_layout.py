"""The observation-state record (libzombsole_amd/csrc/zs_obs_state.hpp) on the CPU: the header compiled with the
host compiler into tests/obs_state_layout_dump.cpp, against _abi.obs_state_layout (the pure-Python mirror the
gloo stand-ins and the byte tables use) and the sizes the record was designed to."""
import os
import re

import pytest

import step_plan_table as T
from libzombsole_amd import _abi, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I32, I64, I16 = _abi.DTYPE_I32, _abi.DTYPE_I64, _abi.DTYPE_I16

# (E, O, DW, OW, dtype): the workloads' shapes, the test maps', and the degenerate ones
C3 = (12, 384, 128, 12, I64)
C5 = (24, 384, 128, 12, I16)
C4 = (54, 3640, 512, 114, I64)
SHAPES = [C3, C5, C4,
          (1, 0, 1, 0, I32), (1, 0, 1, 0, I16), (1, 1, 1, 1, I16),     # E = 1, O = 0, DW = 1
          (2, 16, 1, 1, I16), (2, 16, 1, 1, I32),                      # wall_hp
          (7, 33, 47, 2, I32), (7, 33, 47, 2, I16),                    # odd E, odd O: the u8 rows at a 2-B offset
          (3, 5, 1, 1, I16), (254, 32767, 1 << 19, 1024, I16), (254, 32767, 1 << 19, 1024, I64)]


@pytest.fixture(scope="module")
def rows():
    lines = ["%d %d %d %d %d %d" % (s + (_abi.ENC_CHANNELS,)) for s in SHAPES]
    return T.dump("obs_state_layout_dump", lines)


def test_header_equals_the_python_mirror(rows):
    for s, r in zip(SHAPES, rows):
        exp = _abi.obs_state_layout(*s)
        assert {k: r[k] for k in exp} == exp, (s, r, exp)


def test_designed_sizes(rows):
    by = dict(zip(SHAPES, rows))
    assert by[C3]["rec_bytes"] == 2224
    assert by[C5]["rec_bytes"] == 1584
    assert by[C4]["rec_bytes"] == 17616
    assert _abi.obs_state_layout(*C3)["rec_bytes"] == 2224
    assert _abi.obs_state_layout(*C5)["rec_bytes"] == 1584
    assert _abi.obs_state_layout(*C4)["rec_bytes"] == 17616


def test_sections_tile_the_record(rows):
    for (E, O, DW, OW, dtype), r in zip(SHAPES, rows):
        hp = r["hp_bytes"]
        assert hp == (2 if dtype == I16 else 4)
        sizes = (4, 4, 4 * E, 4 * E, 4 * DW, 4 * OW, hp * O, E, E)
        o = 0
        for name, nb in zip(_abi.OBS_STATE_SECTIONS, sizes):  # in order, no overlap, no gap
            assert r[name] == o, (name, r)
            o += nb
        assert r["pad"] == o
        assert r["rec_bytes"] % 16 == 0 and 0 <= r["rec_bytes"] - o < 16
        for name in _abi.OBS_STATE_SECTIONS[:7]:  # the 4-byte items and the HP are 4-byte aligned
            assert r[name] % 4 == 0


def test_record_dtype_of_the_simple_encoding():
    """int16 observations of the simple encoding fold the unsaturated life into their code: wide HP."""
    lines = ["2 16 1 1 %d %d" % (d, e) for d in (I32, I64, I16) for e in (_abi.ENC_SIMPLE, _abi.ENC_CHANNELS)]
    got = [r["record_dtype"] for r in T.dump("obs_state_layout_dump", lines)]
    assert got == [I32, I32, I64, I64, I32, I16]
    assert got == [_abi.obs_state_record_dtype(d, e) for d in (I32, I64, I16)
                   for e in (_abi.ENC_SIMPLE, _abi.ENC_CHANNELS)]


def test_builder_layout_and_viewer_config():
    b = _abi.multi_env_config(5, "extermination", [], "bridge64", ["0", "1", "2", "3"], initial_zombies=20,
                              obs_dtype=I16)
    assert b.obs_state_layout() == _abi.obs_state_layout(*C5)
    assert not b.cfg.flags & _abi.FLAG_VIEWER
    v = b.viewer(11)
    assert v.cfg.num_envs == 11 and v.cfg.flags & _abi.FLAG_VIEWER and b.cfg.num_envs == 5
    assert not b.cfg.flags & _abi.FLAG_VIEWER and v.obs_state_layout() == b.obs_state_layout()
    v2 = _abi.multi_env_config(3, "extermination", [], "bridge64", ["0", "1"], initial_zombies=10, viewer=True)
    assert v2.cfg.flags & _abi.FLAG_VIEWER and v2.obs_state_layout() == _abi.obs_state_layout(*C3)
    s = _abi.single_env_config(3, "extermination", ["terminator"], "bridge", 0, initial_zombies=4, viewer=True)
    assert s.cfg.flags & _abi.FLAG_VIEWER


def test_symbols_and_flag(rows):
    for name in ("zs_obs_state_layout", "zs_obs_state_pack", "zs_obs_state_unpack"):
        assert name in engine.SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "zombsole_mi355x.h")).read()
    m = re.search(r"^#define ZS_FLAG_VIEWER (\d+)u", hdr, re.M)
    assert m and int(m.group(1)) == _abi.FLAG_VIEWER == rows[0]["flag_viewer"]
    assert _abi.FLAG_VIEWER not in (_abi.FLAG_AUTORESET, _abi.FLAG_DEBUG, _abi.FLAG_DEATH_LOG)
