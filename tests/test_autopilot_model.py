"""The scripted policies' rules on the CPU: libzombsole_amd/autopilot.py's decide equals the reference's own decisions
(tests/golden/pilot/pilot_*.json.gz: every call, agent and policy), the fixtures hold every case a wrong kernel would miss
(pilot_census.py), and a triple's action dict comes back as the triple through the drop-ins' action parsing."""
import numpy as np
import pytest

import golden_util as G
import pilot_census as PC
from libzombsole_amd import actions as A
from libzombsole_amd import autopilot as AP

NAMES = PC.pilot_fixture_names()


def test_there_are_fixtures():
    assert len(NAMES) >= 6 and any("single" in n for n in NAMES)


@pytest.mark.parametrize("name", NAMES)
def test_decide_equals_the_reference(name):
    fx = G.load_fixture(name)
    st_map = PC.static_of(fx)
    n = PC.n_agents(fx)
    for run in fx["runs"]:
        assert len(run["calls"]) == len(run["pilot"]) == 40
        for c, (rec, pl) in enumerate(zip(run["calls"], run["pilot"])):
            view = PC.View(rec["state"], fx, st_map)
            for pname in PC.POLICY_NAMES:
                got = AP.decide(view, st_map, n, pname)
                assert got.dtype == np.int32 and got.tolist() == pl[pname], (name, run["seed"], c, pname, got.tolist(), pl[pname])
            mixed = [(a + c) % 4 for a in range(n)]  # per-agent codes, 0 among them: those rows keep the caller's values
            out = np.full((n, 3), 77, dtype=np.int32)
            AP.decide(view, st_map, n, mixed, out=out)
            want = [[77, 77, 77] if k == 0 else pl[PC.POLICY_NAMES[k - 1]][a] for a, k in enumerate(mixed)]
            assert out.tolist() == want, (name, run["seed"], c)


def test_the_census_has_nothing_missing():
    total = None
    for name in NAMES:
        total = PC.census(G.load_fixture(name), total)
    assert PC.missing(total) == [], PC.missing(total)


def test_the_steps_took_the_recorded_triples():
    """A config driven by its policies steps with the previous call's triples of those policies."""
    for name in NAMES:
        fx = G.load_fixture(name)
        how = fx["extras"]["pilot"]
        if how == "discrete":
            continue
        for run in fx["runs"]:
            for c in range(1, len(run["calls"])):
                rec = run["calls"][c]
                if rec["kind"] != "step":
                    continue
                acts = rec["act"] if fx["surface"] == "multi" else [rec["act"]]
                want = [AP.to_action_dict(run["pilot"][c - 1][p][a]) for a, p in enumerate(how)]
                assert acts == want, (name, run["seed"], c)


def test_unknown_codes_idle_and_absent_agents_idle():
    fx = G.load_fixture("pilot/pilot_multi_open_a4_weapons")
    st_map = PC.static_of(fx)
    view = PC.View(fx["runs"][0]["calls"][0]["state"], fx, st_map)
    assert AP.decide(view, st_map, 4, 9).tolist() == [[0, 0, 0]] * 4
    view.ent[1][1] = 0
    assert AP.decide(view, st_map, 4, "troll").tolist() == [[4, 0, 0], [0, 0, 0], [4, 0, 0], [4, 0, 0]]
    with pytest.raises(ValueError):
        AP.policy_code("hamster")  # the bots that draw from the env's stream are left out


def test_action_dicts_round_trip():
    """to_action_dict -> the drop-ins' parsing (actions.encode_action) -> the triple, for every triple of the fixtures."""
    seen = set()
    for name in NAMES:
        for run in G.load_fixture(name)["runs"]:
            for pl in run["pilot"]:
                seen |= {tuple(t) for rows in pl.values() for t in rows}
    assert {t[0] for t in seen} == {A.ACT_IDLE, A.ACT_MOVE, A.ACT_ATTACK, A.ACT_ATTACK_CLOSEST, A.ACT_HEAL}
    for t in sorted(seen):
        d = AP.to_action_dict(t)
        assert set(d) == {"action_type", "parameter"} and tuple(A.encode_action(d)) == t, (t, d)
    assert AP.to_action_dict((A.ACT_IDLE, 0, 0))["action_type"] is None
