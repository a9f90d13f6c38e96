"""The table of terminal_outcomes.py on the CPU: the oracle alone, over every row's own config, seeds, stream and
steps, shows every outcome the row claims in three envs or more and no row ends only at an episode's first step;
the rows of every lane count provide every outcome between them (and at G = 1 and 2 the decisive thing in a slot
>= G and more agents than lanes); every lane count has k_step and k_tick rows; and the compiled step plan
(zs_step_plan.hpp through tests/step_plan_dump.cpp) resolves every row to the fields its describe() names."""
import os

import pytest

import step_instantiations as S
import step_plan_table as T
import terminal_outcomes as TO

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "libzombsole_amd", "csrc")


@pytest.fixture(scope="module")
def census():
    return {r.id: TO.census(r) for r in TO.ROWS}


def test_every_claimed_outcome_occurs_in_three_envs(census):
    for r in TO.ROWS:
        assert r.claims, r.id
        for o in r.claims:
            assert census[r.id].get(o, 0) >= 3, (r.id, o, census[r.id])


def test_no_row_ends_only_on_first_steps(census):
    for r in TO.ROWS:
        c = census[r.id]
        assert c.get("late_terminal", 0) >= 3 and c["terminal"] >= 3, (r.id, c)
    assert S.STEPS <= 24


def test_every_lane_count_has_every_outcome():
    assert len({r.id for r in TO.ROWS}) == len(TO.ROWS)
    with open(os.path.join(CSRC, "zs_step_plan.hpp")) as f:
        src = f.read()
    for key, cond in TO.UNREACHABLE.items():
        assert cond and cond in src, key
    for G in S.GS:
        rows = [r for r in TO.ROWS if r.G == G]
        have = {o for r in rows for o in r.claims}
        lost = {o for (g, cfg) in TO.UNREACHABLE if g == G for o in TO.CONFIGS[cfg][4] if isinstance(o, str)}
        assert set(TO.OUTCOMES) - lost <= have, (G, set(TO.OUTCOMES) - have)
        if G in TO.LATE_GS:
            assert set(TO.LATE) <= have, (G, have)
            assert any(r.make(1).num_agents == 4 > G for r in rows), G  # A > G through multi_rewards
        assert {r.step_kernel for r in rows} == {"k_step", "k_tick"}, G
        assert {r.n for r in rows} == {S.ENVS[G]}
        # respawn by the tick and deferred to k_respawn, by the override and by a spawn list past 64 cells
        assert {(r.respawn, "defer_respawn" in r.launch) for r in rows if "ext_min_goes_on" in r.claims} == \
            {("tick", False), ("k_respawn", True), ("k_respawn", False)}, G
        assert {r.respawn for r in rows if "ext_min_won" in r.claims} == {"tick", "k_respawn"}, G
    # the agents_dead_bot_alive truncation on both surfaces, the single surface's end reward won and lost
    for G in S.GS:
        surf = {r.info()["surface"] for r in TO.ROWS if r.G == G and "agents_dead_bot_alive" in r.claims}
        assert surf == {"multi", "single"}, G
    zs = {cfg: len(TO.CONFIGS[cfg][0](1).map.zombie_spawns) for cfg in ("ext_min", "ext_min_defer", "ext_wide")}
    assert zs["ext_min"] == zs["ext_min_defer"] == 1 and zs["ext_wide"] > 64, zs


def test_the_plan_resolves_every_row():
    """describe()'s fields of every row (lanes per env, kernel, wave budget, par_exec, respawn) are what the
    compiled step plan resolves the row's config and overrides to, for both par_exec values."""
    for par in (1, -1):
        plans = T.plans([(r.builder(par_exec=par), dict(r.launch, par_exec=par)) for r in TO.ROWS])
        for r, p in zip(TO.ROWS, plans):
            assert "error" not in p, (r.id, p)
            d = r.describe(par)
            assert d["envs"] == r.n == S.ENVS[r.G]
            assert (p["G"], "k_step" if p["fused"] else "k_tick", p["tick_waves"]) == \
                (d["lanes_per_env"], d["step_kernel"], d["tick_waves"]), (r.id, p)
            assert ("k_respawn" if p["defer_respawn"] else "tick") == d["respawn"], (r.id, p)
            assert T.defer_respawn(r.builder(), r.launch) == p["defer_respawn"], r.id
            assert d["par_exec"] == (1 if par >= 0 else 0) and p["obs_bytes"] == 0, (r.id, p)
            if "par_exec" in p:
                assert p["par_exec"] == d["par_exec"], (r.id, p)
