"""The geometry table (geometry_shapes.py) on the CPU: every row on the side of every threshold it claims, by the
compiled plans (tests/step_plan_dump.cpp, tests/obs_plan_dump.cpp) and by the predicates as the headers state them;
every refusal the plans make, with its message; and, by the oracle alone over each row's own config, seeds, stream
and steps, the events the row is there for."""
import pytest

import geometry_shapes as G
import obs_plan_table as OT
import step_plan_table as T
from libzombsole_amd import _abi

IDS = [r.id for r in G.ROWS]
_census = {}


def census(row):
    if row.id not in _census:
        _census[row.id] = G.oracle_census(row, max(G.ENVS))
    return _census[row.id]


def _launch(b):
    return {f: getattr(b._launch, f) for f in _abi.LAUNCH_FIELDS} if b._launch else {}


def _obs_plan(b, lo):
    return T.dump("obs_plan_dump", [" ".join(str(v) for v in [0] + OT.shape_ints(b, lo) + T.launch_ints(lo))])[0]


def test_thresholds_are_the_headers():
    """The table's rows sit one cell either side of each threshold, evaluated from W and H as the code states them."""
    side = {r.id: G.closest_side(r.W, r.H) for r in G.ROWS}
    assert (side["c182x182"], side["c183x182"], side["c256x2"], side["c257x2"]) == ("packed", "generic", "packed", "generic")
    assert 2 * 181 * 181 == 65522 and 182 * 182 + 181 * 181 >= 65536 and 255 * 255 + 1 < 65536 <= 256 * 256 + 1
    assert 255 * 257 == 65535 and 256 * 256 == 65536
    assert G.patch_admitted(3100, 1) and not G.patch_admitted(3101, 1)
    assert G.patch_admitted(1, 4095) and not G.patch_admitted(1, 4096)
    assert G.w_m(255, 16) and not G.w_m(256, 16)
    for r in G.ROWS:
        assert r.closest == side[r.id], r.id
        if r.wm_zero is not None:
            assert (G.w_m(r.W, r.H) == 0) == r.wm_zero, r.id


@pytest.mark.parametrize("W,H", [(255, 16), (132, 31), (1023, 1), (1, 4096), (16, 255)])
def test_w_m_is_exact_where_it_is_taken(W, H):
    """c / W == (c * w_m) >> 20 in uint32 for every cell of maps that take the multiply-shift, of 16, 31
    and 1 rows among them.  The product must also stay below 2^32: a 1 x 16 000 map has w_m = 2^20 and would wrap
    from cell 4 096 on, but the walks that use w_m (zs_obs.hpp's padded-table encoders) run only where the plan
    admits k_obs_pipe's shape, DW <= 64 * OBS_PF_D = 128 words, so no cell index is above 4 095."""
    m = G.w_m(W, H)
    assert m and (W * H + 31) // 32 <= 128, (W, H)
    assert G.w_m(1, 16000) == 1 << 20 and (4096 << 20) == 1 << 32
    for c in range(W * H):
        assert c * m < (1 << 32) and (c * m) >> 20 == c // W, (W, H, c)


@pytest.mark.parametrize("rid", IDS)
def test_row_resolves_to_its_claims(rid):
    """The compiled step plan and observation plan of every row, variant, requested G and kernel: the lanes per
    env, the candidate list's place (cand_cap), the respawn path and the observation kernels the row names."""
    row = G.BY_ID[rid]
    for n in G.ENVS:
        for vname, _ in row.variants:
            for g in G.GS:
                for kernel in ("k_step", "k_tick"):
                    b = row.builder(n, g, kernel, 1, vname)
                    lo = _launch(b)
                    p = T.plans([(b, lo)])[0]
                    what = (rid, n, vname, g, kernel, p)
                    assert "error" not in p, what
                    assert p["G"] == row.G[g] and p["fused"] == (kernel == "k_step"), what
                    nzs = b.cfg.map.n_zombie_spawns
                    assert (p["cand_cap"] >= nzs > 0) == (row.cand[vname] == "lds"), what
                    assert p["cand_cap"] == 0 or row.W * row.H <= 65535, what
                    assert p["defer_respawn"] == (vname == "k_respawn"), what
                    assert p["obs_bytes"] == 0, what
                    o = _obs_plan(b, lo)
                    assert not o["fobs"], what
                    if row.obs:
                        assert (o["full"]["name"], o["masked"]["name"], o["full"]["encoders"]) == row.obs, (what, o)
                        patched = o["full"]["name"] == "k_obs_patch" or o["full"]["encoders"] == "patched"
                        assert not patched or G.patch_admitted(row.W, row.H), what


@pytest.mark.parametrize("rid", sorted(k for k, v in G.REFUSED.items() if v[2]))
def test_plan_refusals(rid):
    """What the plans refuse, and in whose words (zs_create runs the observation plan first)."""
    make, msg, which = G.REFUSED[rid]
    b = make(13)
    o = _obs_plan(b, {})
    if which == "obs":
        assert o.get("error") == msg, o
        return
    assert "error" not in o, o
    for lanes in (0,) + G.GS:
        b.cfg.lanes_per_env = lanes
        for lo in ({}, {"fused": -1}, {"fused": 1}):
            assert T.plans([(b, lo)])[0].get("error") == msg, (rid, lanes, lo)


def test_size_refusals_are_past_the_limits():
    for rid in ("w16001", "h16001", "cells_2p24"):
        m = G.REFUSED[rid][0](1).cfg.map
        assert m.width > 16000 or m.height > 16000 or m.width * m.height > (1 << 24), rid
        assert G.REFUSED[rid][1] == G.MSG_SIZE and G.REFUSED[rid][2] is None


@pytest.mark.parametrize("rid", IDS)
def test_oracle_meets_the_rows_events(rid):
    """By the oracle alone: closest decisions at d^2 >= 65 536 in three envs or more of every row on a map that has
    such a pair and claims the generic branch for it, at d^2 >= 60 000 on 182 x 182, ties at the minimum at such a
    d^2 on the two square maps; autoresets and respawns everywhere; every offset class with each of move, attack
    and heal; an attack and a heal on a thing exactly at range and one cell past it (the agents carry rifles)."""
    row = G.BY_ID[rid]
    cs = census(row)

    def envs(key):
        return sum(1 for c in cs if c[key])
    if rid in ("c183x182", "c257x2", "x16000x1", "x1x16000"):
        assert envs("far") >= 3, (rid, envs("far"))
    if rid in ("c182x182", "c183x182", "c256x2"):
        assert envs("high") >= 3, (rid, envs("high"))
    if rid in ("c182x182", "c183x182"):
        assert envs("far_ties") >= 3, (rid, envs("far_ties"))
    if rid.startswith("c") or rid.startswith("n"):
        assert envs("ties") >= 3, (rid, envs("ties"))
    assert all(c["autoresets"] >= 3 for c in cs) and envs("respawns") >= 3, rid
    if row.obs:  # a zombie or a body in the map's last cell and in the first row's last cell, in an agent's window
        assert envs("last_cell") >= 3 and envs("row_end") >= 3, (rid, envs("last_cell"), envs("row_end"))
    classes = set().union(*[c["classes"] for c in cs])
    need = {(k, cn) for k in ("move", "attack", "heal") for ext in (row.W, row.H) for cn in G.offset_classes(ext)}
    assert not need - classes, (rid, sorted(need - classes))
    edge = set().union(*[c["edge"] for c in cs])
    assert edge == {("attack", "at"), ("attack", "past"), ("heal", "at"), ("heal", "past")}, (rid, sorted(edge))


def test_far_stream_reaches_every_offset():
    """The stream's offsets: every value of the issue's set on both axes, about half of all targets within a
    rifle's reach (or one cell past it), +-2^40 only on request, and saturated to int32 by encode_action."""
    from libzombsole_amd import actions as A
    seen_x, seen_y, near = set(), set(), 0
    N = 20000
    for i in range(N):
        a = G.far_action(5, i, i % 3, 183, 182)["parameter"]
        seen_x.add(a[0])
        seen_y.add(a[1])
        near += abs(a[0]) <= 11 and abs(a[1]) <= 11
    assert set(G.far_offsets(183)) | set(G.NEAR) == seen_x and set(G.far_offsets(182)) | set(G.NEAR) == seen_y
    assert 0.4 < near / N < 0.6, near / N
    big = {v for i in range(4000) for v in G.far_action(5, i, 0, 183, 182, beyond=True)["parameter"]}
    assert {1 << 40, -(1 << 40)} <= big
    assert A.encode_action({"action_type": "move", "parameter": [1 << 40, -(1 << 40)]}) == (A.ACT_MOVE, G.I32_MAX, G.I32_MIN)
    assert A.encode_action({"action_type": "heal", "parameter": [-(1 << 40), 3]}) == (A.ACT_HEAL, G.I32_MIN, 3)
