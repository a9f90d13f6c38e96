"""The decision table (decision_cases.py) under the oracle alone: every row reaches every branch it claims, the rows
together reach every counter of the decision census but those argued unreachable, and the runs recorded from the
reference (tests/golden/dec_*.json.gz) took the branches the table lists for them.  Also the drop-ins' range
thresholds against the reference's own comparison."""
import math

import pytest

import decision_cases as D
import golden_util as G
from oracle.oracle import CENSUS_DECISIONS


@pytest.fixture(scope="module")
def censuses():
    return {r.id: D.oracle_census(r, r.seeds(D.N_PLAN)) for r in D.ROWS}


@pytest.mark.parametrize("row", D.ROWS, ids=[r.id for r in D.ROWS])
def test_row_meets_its_claims(row, censuses):
    assert set(row.claims) <= set(CENSUS_DECISIONS), set(row.claims) - set(CENSUS_DECISIONS)
    c = censuses[row.id]
    missing = [k for k in row.claims if c[k] < 1]
    assert not missing, (row.id, missing)


def test_rows_meet_every_counter(censuses):
    assert set(D.UNREACHABLE) <= set(CENSUS_DECISIONS)
    tot = {k: sum(c[k] for c in censuses.values()) for k in CENSUS_DECISIONS}
    claimed = {k for r in D.ROWS for k in r.claims}
    for k in CENSUS_DECISIONS:
        if k in D.UNREACHABLE:
            assert tot[k] == 0 and k not in claimed, (k, tot[k])
        else:
            assert tot[k] >= 1 and k in claimed, (k, tot[k])


@pytest.mark.parametrize("row", D.FIXTURES, ids=[r.id for r in D.FIXTURES])
def test_fixture_took_its_branches(row):
    """The fixture's own config, stream, seeds and calls, as recorded, replayed by the oracle (which
    test_oracle_golden.py holds to the recording call by call)."""
    fx = G.load_fixture("dec_" + row.id)
    seeds, calls, claims = row.fixture
    assert fx["kwargs"] == row.kwargs and fx["stream"] == row.stream and fx["max_steps"] == row.max_steps
    assert (fx.get("extras") or {}) == row.extras
    assert [r["seed"] for r in fx["runs"]] == list(seeds) and all(len(r["calls"]) == calls for r in fx["runs"])
    assert calls <= 40
    for r in fx["runs"]:  # the actions the recording took are the row's stream
        for i, rec in enumerate(r["calls"]):
            if rec["kind"] == "step":
                want = row.actions([r["seed"]], i, row.n_agents)[0]
                assert (G.action_triples(fx, rec, row.n_agents)[:row.n_agents] == want).all(), (row.id, r["seed"], i)
    c = D.oracle_census(row, seeds, calls=calls)
    missing = [k for k in claims if c[k] < 1]
    assert not missing, (row.id, missing)


def test_fixtures_hold_the_rare_branches():
    held = {k for r in D.FIXTURES for k in r.fixture[2]}
    need = ["z_blocked_obst_first", "z_blocked_obst_later", "z_blocked_tie", "z_blocked_idle", "z_move_tie",
            "z_move_offmap", "h_move_offmap", "r_move_offmap", "z_wander_stuck"]
    need += ["z_blocked_skip_dir%d" % k for k in range(4)] + ["z_wander_n%d" % k for k in range(1, 5)]
    need += ["c_tie_zombie", "c_tie_order_zombie"]
    need += ["hit_edge_%s_%s" % (s, w) for s in ("in", "out") for w in ("knife", "axe", "gun", "rifle", "shotgun", "heal")]
    need += ["hit_edge_in_claws"]
    assert not [k for k in need if k not in held], [k for k in need if k not in held]


# (max_range, the next d^2 past max_range^2 that two integers give): weapons.py:18-25, core.py:9 HEALING_RANGE
RANGES = {"ZombieClaws": (1.5, 2, 4), "Knife": (1.5, 2, 4), "Axe": (1.5, 2, 4), "Gun": (6, 36, 37),
          "Rifle": (10, 100, 101), "Shotgun": (3, 9, 10)}
CODES = {"ZombieClaws": 1, "Knife": 10, "Axe": 11, "Gun": 12, "Rifle": 13, "Shotgun": 14}


def test_dropin_thresholds_are_the_references_comparison():
    """things.weapon_r2 (what game.py's event views test d^2 against) at r^2 and at the next d^2 of a grid, against
    sqrt(d^2) <= max_range with the ranges of this table.  The views' messages themselves at those distances, a
    heal's among them, are in the dec_edge fixture's event log (test_dropin_golden.py)."""
    from libzombsole_amd import things
    for name, (rng, d_in, d_out) in RANGES.items():
        r2 = things.weapon_r2(CODES[name])
        # the largest in-range d^2 and the smallest out-of-range one are the table's pair
        assert math.sqrt(d_in) <= rng < math.sqrt(d_out), name
        assert not any(math.sqrt(d_in) < math.sqrt(a * a + b * b) <= rng for a in range(12) for b in range(12)), name
        for d2 in (d_in, d_out):
            assert (d2 <= r2) == (math.sqrt(d2) <= rng), (name, d2, r2)
        assert float(things.weapon_for_code(CODES[name]).max_range) == float(rng), name
    assert set(CODES.values()) == set(things._WEAPONS)
