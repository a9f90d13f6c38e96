"""The table of reset_shapes.py on the CPU: the compiled step plan (zs_step_plan.hpp through step_plan_dump.cpp)
resolves every row and launch variant to what the variant's name says (respawn deferred to k_respawn or left to the
tick's leader, the spawn lists staged in LDS or read from HBM, the tick's candidate list in LDS or in HBM, a reset
image that fits), the shapes are the ones the rows are named for, and the oracle's own run of every row's config,
seeds, action stream and steps meets the events the row claims.  A row whose claim its reference run does not
meet is a wrong row."""
import pytest

import reset_shapes as R
import step_plan_table as T

ALL = R.ROWS + R.FAIL_ROWS


def _shape(row):
    c = row.make(1).cfg
    E = c.num_agents + c.num_bots + max(c.initial_zombies, c.minimum_zombies)
    return {"A": c.num_agents, "P": c.num_bots, "E": E, "nps": c.map.n_player_spawns, "nzs": c.map.n_zombie_spawns,
            "cells": c.map.width * c.map.height, "O": c.map.n_obstacles, "initial": c.initial_zombies,
            "minimum": c.minimum_zombies}


def test_rows_have_the_shapes_they_are_named_for():
    s = {r.id: _shape(r) for r in ALL}
    assert [s[k]["A"] + s[k]["P"] for k in ("p63", "p64", "p65", "p100", "single65")] == [63, 64, 65, 100, 65]
    assert s["single65"]["A"] == 1 and s["single65"]["P"] >= 64
    assert [s[k]["E"] for k in ("e64", "e65", "e254")] == [64, 65, 254]
    assert [s[k]["nzs"] for k in ("z0", "z1", "z64", "z65", "z512", "z513", "z600")] == [0, 1, 64, 65, 512, 513, 600]
    assert [s[k]["nzs"] for k in ("hbm0", "hbm1", "hbm65", "hbm512", "hbm513", "hbm600")] == [0, 1, 65, 512, 513, 600]
    assert sum(1 for r in ALL for _, ov in r.variants if ov.get("reset_lists", 0) < 0) == 2
    assert s["z0"]["cells"] % 64 and s["e65"]["nzs"] == 0 and s["e65"]["cells"] % 64
    assert s["z1"]["initial"] == 0 < s["z1"]["minimum"] and s["init_only"]["minimum"] == 0 < s["init_only"]["initial"]
    for k, extra in (("ps_exact", 0), ("ps_plus1", 1), ("fail_agents", -1), ("fail_agents0", -1)):
        assert s[k]["nps"] == s[k]["A"] + s[k]["P"] + extra, k
    assert s["fail_bots"]["nps"] == s["fail_bots"]["P"] - 1
    assert s["walls4200"]["O"] > 4096 + 32 and (s["walls4200"]["O"] + 31) // 32 > 128
    assert s["short"]["nzs"] < s["short"]["minimum"] // 3
    # no random pick at all: fixed agent weapons, bots that bring theirs
    c = R.ROWS[[r.id for r in R.ROWS].index("nrw0")].make(1)
    assert not (c._aw == 255).any() and set(c._bt.tolist()) <= {1, 2}
    # the player rows mix fixed and random agent weapons and hold bots of all five types, in an order in which
    # weapon-bringing and weapon-drawing bots interleave
    for k in ("p63", "p64", "p65", "p100"):
        c = R.ROWS[[r.id for r in R.ROWS].index(k)].make(1)
        aw = c._aw.tolist()
        assert 255 in aw and set(aw) - {255} and aw[0] == 255 and aw[1] != 255
        assert set(c._bt.tolist()) == {1, 2, 3, 4, 5} and c._bt.tolist()[:5] == [4, 1, 3, 2, 5]
    for r in ALL:
        assert 5 <= r.n <= 37 and r.n % 2 == 1, r.id
        assert len({v for v, _ in r.variants}) == len(r.variants), r.id
    for r in R.ROWS:
        assert 12 <= r.steps <= 24, r.id
    assert len({r.id for r in ALL}) == len(ALL)


def test_the_plan_resolves_every_variant():
    pairs, keys = [], []
    for r in ALL:
        for vid, ov in r.variants:
            b = r.builder(ov)
            launch = dict(ov, fobs=-1)
            launch.pop("lanes_per_env", None)
            pairs.append((b, launch))
            keys.append((r, vid, ov))
    for (r, vid, ov), p in zip(keys, T.plans(pairs)):
        s = _shape(r)
        total = s["nzs"] or s["cells"]
        assert "error" not in p, (r.id, vid, p)
        assert bool(p["fused"]) == (ov["fused"] > 0), (r.id, vid, p)
        if "defer_respawn" in ov:
            assert p["defer_respawn"] == (1 if ov["defer_respawn"] > 0 and s["minimum"] > 0 else 0), (r.id, vid, p)
        assert p["reset_lds"] <= 160 * 1024, (r.id, vid, p)  # zs_create's bound on the reset image
        if r.id.startswith("hbm"):  # no list staged anywhere: wave_spawn and spawn_at read them from HBM
            assert s["nps"] + s["nzs"] > 4096 and p["rlists_cap"] == 0 == p["lists_cap"], (r.id, vid, p)
        else:  # the lists staged in the reset work's LDS image (reset_lists = -1: because the tick stages them)
            assert p["rlists_cap"] == s["nps"] + s["nzs"] > 0, (r.id, vid, p)
        if ov.get("reset_lists", 0) < 0:
            assert not p["fused"] and p["rlists_cap"] == p["lists_cap"], (r.id, vid, p)
        if p["fused"]:
            assert p["rlists_cap"] == p["lists_cap"], (r.id, vid, p)
        if "lanes_per_env" in ov:
            assert p["G"] == ov["lanes_per_env"], (r.id, vid, p)
        if vid == "leader_cand_hbm":  # either side of the tick's `total <= cand_cap`, the plan's cand_cap read
            assert not total <= p["cand_cap"], (r.id, vid, p)
        if vid == "leader_cand_lds":
            assert total <= p["cand_cap"], (r.id, vid, p)


def test_reset_lists_off_alone_does_not_reach_hbm():
    """zs_launch.reset_lists = -1 keeps k_reset from staging the lists on its own; the reset work still shares the
    tick's staged lists (rlists_cap = lists_cap), which the plan stages whenever they fit.  So the override alone
    reads no list from HBM on any map whose lists fit the tick's image (bridge64's 272 entries here): the hbm rows
    exist for that path."""
    import step_instantiations as S
    b = S.c2(37).set_launch({"fused": -1, "reset_lists": -1, "fobs": -1})
    p = T.plans([(b, {"fused": -1, "reset_lists": -1, "fobs": -1})])[0]
    assert p["rlists_cap"] == p["lists_cap"] == 272, p


@pytest.fixture(scope="module")
def runs():
    return {r.id: R.oracle_run(r)[0] for r in R.ROWS}


@pytest.mark.parametrize("row", R.ROWS, ids=[r.id for r in R.ROWS])
def test_rows_meet_their_claims(row, runs):
    c = runs[row.id]
    assert row.claims, row.id
    for k in row.claims:
        assert c[k] > 0, (row.id, k, c)
    for k in row.zero:
        assert c[k] == 0, (row.id, k, c)
    assert c["player_fails"] == 0, (row.id, c)
    if "autoresets" in row.claims:  # every env went through two autoresets or more
        assert c["autoresets"] >= 2 * row.n, (row.id, c)


def test_short_of_room_is_short_at_every_respawn(runs):
    """`short`: every respawn finds fewer cells than it needs.  `z1`: the walled-in cell gives n = 0 and n = 1."""
    c = runs["short"]
    assert c["respawns"] > 0 and c["spawn_short"] >= c["respawns"], c
    c = runs["z1"]
    assert c["spawn_empty"] > 0 and c["spawn_one"] > 0, c


@pytest.mark.parametrize("row", R.FAIL_ROWS, ids=[r.id for r in R.FAIL_ROWS])
def test_failing_rows_fail_in_the_oracle(row):
    from libzombsole_amd import _abi
    for rc, _, cen, _ in R.oracle_failing_reset(row):
        assert rc == _abi.ZS_ENOSPACE
        for k in row.claims:
            assert cen[k] > 0, (row.id, k, cen)
        assert cen["player_fails"] == 1
