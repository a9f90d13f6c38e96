"""The action-mask rules on the CPU: what the mask fixtures (tests/golden/masks_*.json.gz, the reference's own masks,
make_mask_golden.py) cover, and the host model (mask_model.py) held to every call of them.  The GPU tests
(test_action_mask.py) compare the kernel with the fixtures and, beyond them, with this model."""
import collections

import pytest

import golden_util as G
import mask_census as C
import mask_model as M


@pytest.fixture(scope="module")
def fixtures():
    return [G.load_fixture(n) for n in C.mask_fixture_names()]


def test_mask_fixtures_cover_every_case(fixtures):
    """Every case of mask_census.NEED, and every bit of every id seen both 0 and 1, from the files alone."""
    assert len(fixtures) >= 4
    got = collections.Counter()
    for fx in fixtures:
        C.census(fx, got)
    assert not C.missing(got), (C.missing(got), dict(got))
    # what the fixtures were chosen for, one by one
    per = {fx["name"]: C.census(fx) for fx in fixtures}
    want = {"masks_multi_open_a4_weapons": ("attack_knife_in", "attack_knife_out", "attack_axe_in", "attack_axe_out",
                                            "attack_shotgun_in", "attack_shotgun_out", "attack_gun_in",
                                            "attack_gun_out", "dest_obstacle_nonpos_tick1", "dest_obstacle_gone",
                                            "corner", "no_zombies", "terminal_call"),
            "masks_multi_open_a2_rifle_bot": ("heal_closest_bot_in_range", "heal_closest_bot_out_of_range",
                                              "dead_beside_live", "attack_rifle_in"),
            "masks_multi_open_a3_rifle_sparse": ("attack_rifle_out", "attack_rifle_in"),
            "masks_multi_strip_a2_knife": ("lone_agent", "dead_beside_live"),
            "masks_single_strip_bot": ("surface_single", "dest_obstacle_nonpos_tick1")}
    for name, cases in want.items():
        for c in cases:
            assert per[name][c] > 0, (name, c, dict(per[name]))


def _mismatches(fixtures, **mutation):
    bad = []
    for fx in fixtures:
        mp = M.MapInfo(G.map_path(fx["kwargs"]["map_name"]))
        nd = 7 if fx["surface"] == "multi" else 6
        for run in fx["runs"]:
            for i, (rec, want) in enumerate(zip(run["calls"], run["masks"])):
                got = M.masks(rec["state"], mp, len(want), nd, **mutation)
                for a, (g, w) in enumerate(zip(got, want)):
                    bad += [(fx["name"], run["seed"], i, a, k) for k in range(8) if g[k] != w[k]]
    return bad


def test_model_equals_the_reference_on_every_fixture_call(fixtures):
    bad = _mismatches(fixtures)
    assert not bad, (len(bad), bad[:10])


@pytest.mark.parametrize("mutation,ids", [
    (dict(dead_obstacles_block=False), {0, 1, 2, 3}),  # present with life <= 0 does not block
    (dict(heal_r2=8), {6}),                            # the range test off by one at d2 = 9
    (dict(others_exclude_self=False), {6}),            # the other-player scan includes the agent itself
])
def test_the_fixtures_catch_a_wrong_rule(fixtures, mutation, ids):
    bad = _mismatches(fixtures, **mutation)
    assert bad and {b[4] for b in bad} <= ids, (len(bad), bad[:5])
