"""Per-env zombie counts and time limits on the CPU: the snapshot record with and without the env_params section
(tests/env_params_layout_dump.cpp, the headers compiled with the host compiler), the Python mirrors, and the table of
the GPU cases (env_params_cases.py) checked with the oracle alone."""
import re

import pytest

import env_params_cases as EP
import step_plan_table as T
from libzombsole_amd import _abi, engine
from test_snapshot_layout import SHAPES, by_hand

WORDS = 13  # the 4-byte sections of an unflagged record


@pytest.fixture(scope="module")
def layouts():
    rows = T.dump("env_params_layout_dump", ["L %d %d %d %d %d %d" % (s + (f,)) for s in SHAPES.values() for f in (0, 1)])
    return {(name, f): rows[2 * i + f] for i, name in enumerate(SHAPES) for f in (0, 1)}


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_unflagged_layout_is_todays(layouts, shape):
    r, o = layouts[(shape, 0)], 0
    for name, nb in by_hand(*SHAPES[shape]):  # the engine arrays' per-env sizes, written out by hand
        assert r[name] == o, name
        o += nb
    assert r["pad"] == o and r["rec_bytes"] == (o + 15) // 16 * 16 and r["env_params"] == 0
    assert {k: r[k] for k in _abi.snapshot_layout(*SHAPES[shape])} == _abi.snapshot_layout(*SHAPES[shape])
    old = T.dump("snapshot_layout_dump", ["L %d %d %d %d %d" % SHAPES[shape]])[0]  # the existing program, unchanged
    assert {k: r[k] for k in r if k != "env_params"} == {k: old[k] for k in old if k not in ("nscal", "ring_words", "nsec")}


def test_bridge64_record_sizes(layouts):
    assert layouts[("bridge64_E12_A2", 0)]["rec_bytes"] == 7376  # test_snapshot_layout.py's number
    assert layouts[("bridge64_E12_A2", 1)]["pad"] == layouts[("bridge64_E12_A2", 0)]["pad"] + 24


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_flagged_layout(layouts, shape):
    r0, r1 = layouts[(shape, 0)], layouts[(shape, 1)]
    sizes = by_hand(*SHAPES[shape])
    assert r1["pad"] == r0["pad"] + 24  # six int32 words, before padding
    assert r1["rec_bytes"] == (r1["pad"] + 15) // 16 * 16
    for name, _ in sizes[:WORDS]:  # every 4-byte section where it was, and aligned
        assert r1[name] == r0[name] and r1[name] % 4 == 0, name
    name, nb = sizes[WORDS - 1]
    assert name == "prev_life" and r1["env_params"] == r0[name] + nb and r1["env_params"] % 4 == 0
    for name, _ in sizes[WORDS:]:  # the byte rows, 24 bytes on
        assert r1[name] == r0[name] + 24, name
    assert r1["weapon"] == r1["env_params"] + 24
    exp = _abi.snapshot_layout(*SHAPES[shape], env_params=True)
    assert {k: r1[k] for k in exp} == exp


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_walker_takes_the_section(shape):
    E, O, DW, OW, A = SHAPES[shape]
    r = T.dump("env_params_layout_dump", ["W %d %d %d %d %d 5" % (E, O, DW, OW, A)])[0]
    assert r.get("ok"), r
    assert r["rec_bytes"] == _abi.snapshot_layout(E, O, DW, OW, A, env_params=True)["rec_bytes"]
    assert r["nsec"] == 18 - (O == 0) * 3  # a map without obstacles has three empty sections


def test_fingerprint_covers_the_flag():
    mk = lambda **kw: _abi.multi_env_config(13, "extermination", [], "bridge64", ["0", "1"], initial_zombies=6,  # noqa: E731
                                            minimum_zombies=3, max_episode_steps=5, **kw)
    plain, flagged, flagged2 = mk().snapshot_layout(), mk(env_params=True).snapshot_layout(), \
        mk(env_params=True, lanes_per_env=8, obs_dtype=_abi.DTYPE_I16).snapshot_layout()
    assert plain["fingerprint"] != flagged["fingerprint"] == flagged2["fingerprint"]
    assert flagged["rec_bytes"] != plain["rec_bytes"] and flagged["pad"] == plain["pad"] + 24
    assert "env_params" not in plain and flagged["env_params"] == plain["weapon"]
    # the unflagged fingerprint is what the header gives without the flag (the existing host program)
    from test_snapshot_layout import _builder_line
    got = T.dump("snapshot_layout_dump", [_builder_line(mk())])[0]
    assert got["fp_lo"] | (got["fp_hi"] << 32) == plain["fingerprint"]


def test_header_constants_and_symbols():
    src = open(T.ROOT + "/include/zombsole_mi355x.h").read()
    assert int(re.search(r"#define ZS_FLAG_ENV_PARAMS (\d+)u", src).group(1)) == _abi.FLAG_ENV_PARAMS == 16
    assert int(re.search(r"#define ZS_OVF_PARAM_RANGE (\d+)u", src).group(1)) == _abi.OVF_PARAM_RANGE == 4
    for name in ("zs_env_params_set", "zs_env_params_get", "zs_env_params_check"):
        assert name in engine.SYMBOLS and re.search(r"\bint %s\(" % name, src)
    b = _abi.multi_env_config(3, "extermination", [], "bridge64", ["0"], env_params=True)
    assert b.cfg.flags & _abi.FLAG_ENV_PARAMS and not _abi.multi_env_config(3, "extermination", [], "bridge64", ["0"]).cfg.flags & 16


# -- the case table ------------------------------------------------------------------------------------------------
def test_rows_cover_the_matrix():
    rows = EP.ROWS
    assert {r.G for r in rows} == {1, 8, 16, 64}
    for G in (1, 8, 16, 64):
        assert {r.step_kernel for r in rows if r.G == G} == {"k_step", "k_tick"}, G
    for kernel in ("k_step", "k_tick"):
        assert {r.defer for r in rows if r.step_kernel == kernel} == {-1, 1}, kernel
        assert {r.graph for r in rows if r.step_kernel == kernel} == {False, True}, kernel
    assert {r.config for r in rows} == set(EP.CONFIGS) and {EP.CONFIGS[c][2] for c in EP.CONFIGS} == {6, 7}
    assert len({r.id for r in rows}) == len(rows) and all(r.n % 2 == 1 and 13 <= r.n <= 67 for r in rows)
    ch = EP.CHANGE_ROWS
    assert {r.step_kernel for r in ch} == {"k_step", "k_tick"} and {r.defer for r in ch} == {-1, 1}
    assert {r.graph for r in ch} == {False, True} and {EP.CONFIGS[r.config][2] for r in ch} == {6, 7}


@pytest.mark.parametrize("config", sorted(EP.CONFIGS))
def test_triples_hold_the_edge_values(config):
    I, M, ms = EP.CONFIGS[config][1]
    t = EP.TRIPLES(I, M)
    assert len(t) == 13 and {0, 1, I} <= {v[0] for v in t} and {0, M} <= {v[1] for v in t}
    assert {0, 1} <= {v[2] for v in t} and {v[2] for v in t} & {3, 4, 5, 6}
    assert all(0 <= v[0] <= I and 0 <= v[1] <= M and v[2] >= 0 for v in t)
    # the engine's slots are the caps': an env's own config never needs more
    assert all(max(v[0], v[1]) <= max(I, M) for v in t)


@pytest.mark.parametrize("row", EP.ROWS, ids=lambda r: r.id)
def test_row_shows_its_claims(row):
    trip = row.triples()
    assert {v[0] for v in trip} >= {0, 1, row.caps[0]} and {v[1] for v in trip} >= {0, row.caps[1]}
    assert {v[2] for v in trip} >= {0, 1}
    got = EP.census(row)
    for c in EP.CLAIMS:
        assert got.get(c, 0) >= 3, (c, got)
    assert T.defer_respawn(row.builder(env_params=False), row.launch) == (1 if row.defer > 0 else 0)


@pytest.mark.parametrize("row", EP.CHANGE_ROWS, ids=lambda r: r.id)
def test_changed_rows_reset_after_the_change(row):
    """Case 2 means something only if envs that got a new triple reset afterwards, and some of them mid-episode at
    the change (they keep their old triple for the rest of the episode)."""
    tracks = [EP.Track(row, s, tr) for s, tr in zip(row.seeds(), row.triples())]
    for k in tracks:
        k.reset()
    mid, took = 0, 0
    for t in range(1, EP.STEPS + 1):
        if t == EP.CHANGE_AFTER + 1:
            for e, tr in row.changed().items():
                tracks[e].pending = tr
                mid += (not tracks[e].need) and tr != tracks[e].triple
        before = [k.pending is not None for k in tracks]
        for k in tracks:
            k.step(t)
        took += sum(1 for b, k in zip(before, tracks) if b and k.pending is None)
    assert mid >= 3 and took >= 3, (mid, took)
    got = EP.census(row, change=True)
    assert got.get("timelimit", 0) >= 3, got
