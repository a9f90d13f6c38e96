"""What the reference's recorded runs (tests/golden/*.json.gz) contain of the ways an episode can end: counted
from the fixture files alone (outcomes.classify over consecutive records), per rule and surface.  Every outcome of
NEED must be present, so that a later regeneration of the fixtures cannot silently lose one: these records are
what holds the oracle's restatement of the four rules to the reference (test_oracle_golden.py), and the oracle is
what the engine is compared with everywhere else."""
import collections

import pytest

import golden_util as G
import outcomes as O
from libzombsole_amd.maps import load_map

# (rule, surface or None for either) -> the outcomes some fixture must hold
NEED = {
    ("safehouse", "multi"): ("safe_won", "safe_won_death", "safe_lost"),
    ("evacuation", None): ("evac_won_bot_first", "evac_won_agents_only", "evac_won_dead_member", "evac_apart",
                           "evac_apart_diag", "evac_lost"),
    ("survival", "multi"): ("surv_lost",),
    ("survival", "single"): ("surv_lost", "single_lost", "agents_dead_bot_alive"),
    ("extermination", None): ("ext_won", "ext_lost", "ext_min_won", "ext_min_goes_on"),
    (None, None): ("done_and_timelimit",),
}


def fixture_census(fx):
    kw = fx["kwargs"]
    info = {"rule": kw["rules_name"], "surface": fx["surface"], "min_z": kw.get("minimum_zombies", 0),
            "objectives": {tuple(p) for p in load_map(G.map_path(kw["map_name"])).objectives}, "G": 0}
    got = collections.Counter()
    for run in fx["runs"]:
        prev = None
        for rec in run["calls"]:
            if rec["kind"] == "step" and "raised" not in rec and prev is not None:
                got.update(O.classify(info, prev, rec["state"], rec["done"], rec["trunc"]))
            prev = rec["state"]
    return info, got


@pytest.fixture(scope="module")
def census():
    tot = collections.defaultdict(collections.Counter)
    for name in G.fixture_names():
        info, got = fixture_census(G.load_fixture(name))
        for key in ((info["rule"], info["surface"]), (info["rule"], None), (None, None)):
            tot[key].update(got)
    return tot


def test_every_terminal_outcome_is_recorded(census):
    missing = [(key, o) for key, outs in NEED.items() for o in outs if census[key][o] == 0]
    assert not missing, (missing, {k: dict(v) for k, v in census.items()})


def test_the_terminal_fixtures_hold_what_they_were_chosen_for():
    """The fixtures recorded for the outcomes, one by one (make_golden.py names them in its comments)."""
    want = {"term_safe_tiny_a2": ("safe_won", "done_and_timelimit"),
            "term_safe_crowd_a2": ("safe_won_death", "safe_lost"),
            "term_evac_tiny_a4": ("evac_won_agents_only", "evac_apart_diag", "done_and_timelimit"),
            "term_evac_tiny_bot_a2": ("evac_won_bot_first", "evac_apart_diag"),
            "term_evac_crowd_a4": ("evac_lost", "evac_won_dead_member"),
            "term_surv_melee_a2": ("surv_lost",),
            "term_surv_single_troll": ("surv_lost", "single_lost", "agents_dead_bot_alive"),
            "term_ext_one_spawn_a2": ("ext_min_won", "ext_min_goes_on")}
    for name, outs in want.items():
        _, got = fixture_census(G.load_fixture(name))
        for o in outs:
            assert got[o] > 0, (name, o, dict(got))
