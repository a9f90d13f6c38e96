"""The case table of step_instantiations.py on the CPU: the rows and the justified unreachable entries are the 21
device functions of k_tick_g.hip; the compiled step plan (zs_step_plan.hpp) resolves every row's config and
overrides to the row's instantiation, and every row's requested lanes-per-env count fits its LDS image, so the
plan keeps it; the env counts give partial workgroups; and the oracle's census of every row's own config,
seeds, action stream and steps shows the action-list regimes and the conflict cases the rows claim."""
import os

import pytest

import step_instantiations as S
import step_plan_table as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "libzombsole_amd", "csrc")


def test_rows_cover_all_21():
    every = S.all_instantiations()
    assert len(every) == len(set(every)) == 21
    rows = [(r.G, r.kernel) for r in S.ROWS]
    assert len(rows) == len(set(rows))
    assert not set(rows) & set(S.UNREACHABLE)
    assert set(rows) | set(S.UNREACHABLE) == set(every)
    assert len(rows) + len(S.UNREACHABLE) == 21
    with open(os.path.join(CSRC, "zs_step_plan.hpp")) as f:
        src = f.read()
    for key, cond in S.UNREACHABLE.items():  # every unreachable entry quotes a condition that stands in the plan
        assert cond and cond in src, key
    # launches of less than one workgroup: one per kernel kind
    assert {r.step_kernel for r in S.SMALL_ROWS} == {"k_step", "k_tick"}
    assert {(r.G, r.n) for r in S.SMALL_ROWS} == {(1, 3), (16, 1)}
    assert len({r.id for r in S.ROWS + S.SMALL_ROWS}) == len(S.ROWS) + len(S.SMALL_ROWS)


ALL_ROWS = S.ROWS + S.SMALL_ROWS


def test_the_plan_resolves_every_row_to_its_instantiation():
    """The compiled step plan, given every row's config and overrides, names the row's lanes per env, kernel and
    wave budget (what describe() must report), and step_defer_respawn() the row's respawn."""
    plans = T.plans([(r.builder(), dict(r.launch, par_exec=1)) for r in ALL_ROWS])
    for r, p in zip(ALL_ROWS, plans):
        assert "error" not in p, (r.id, p)
        assert (p["G"], bool(p["fused"]), p["tick_waves"]) == (r.G, r.fused, r.tick_waves), (r.id, p)
        assert ("k_step" if p["fused"] else "k_tick") == r.step_kernel == r.describe()["step_kernel"], r.id
        assert ("k_respawn" if p["defer_respawn"] else "tick") == r.respawn, (r.id, p)
        assert T.defer_respawn(r.builder(), r.launch) == p["defer_respawn"], r.id
        assert p["obs_bytes"] == 0, (r.id, p)  # fobs = -1: no observation image in the step's LDS
        assert r.launch["fobs"] == -1 and r.launch["fused"] == (1 if r.fused else -1)
        assert r.launch.get("tick_waves", 0) == (0 if r.fused else r.tick_waves)
        assert r.describe()["tick_waves"] == (3 if r.fused else int(r.kernel[-1]))
        assert {k: p[k] for k in T.FIELDS} == {k: T.expected("row:" + r.id, r.launch)[k] for k in T.FIELDS}, r.id


def test_requested_lanes_fit_their_image():
    """The plan raises a requested G only when not even the smallest image of 64 / G envs fits 64 KiB."""
    def min_bytes(builder, G, fused):
        return T.images([S.min_image_args(builder, G, fused)])[0]["bytes"]
    sizes = T.images([S.min_image_args(r.builder(1), r.G, r.fused) for r in ALL_ROWS])
    for r, im in zip(ALL_ROWS, sizes):
        assert im["bytes"] <= 64 * 1024, (r.id, im)
    # the arithmetic bites: city128's bitmap alone (512 words an env) fills 64 KiB with 32 envs, so the city128
    # rows start at G = 16; and bridge64's 12 entities leave 64 envs to an image little room (the c2 row of G = 1)
    assert min_bytes(S.c4(1), 1, False) > min_bytes(S.c4(1), 2, False) > 64 * 1024
    assert min_bytes(S.c4(1), 4, True) <= 64 * 1024
    assert 56 * 1024 < min_bytes(S.c2(1), 1, False) <= 64 * 1024 < min_bytes(S.c5(1), 1, False)


def test_env_counts_leave_partial_workgroups():
    for r in S.ROWS:
        per_wg = 64 // r.G
        assert r.n == S.ENVS[r.G] <= 130
        assert r.n > per_wg, r.id  # two workgroups or more ...
        assert r.n % per_wg != 0 or r.G == 64, r.id  # ... the last one partial (G = 64: one env a workgroup)
    assert S.ENVS[1] == 64 + 3 and S.ENVS[16] == 9 * 4 + 1 and S.ENVS[32] == 18 * 2 + 1
    for G in S.GS:  # xcd_remap over tick workgroups whose number is no multiple of 8 (2, 2, 3, 5, 10, 19, 13)
        assert -(-S.ENVS[G] // (64 // G)) % 8, G
    for r in S.SMALL_ROWS:
        assert r.n < 64 // r.G, r.id


@pytest.fixture(scope="module")
def census():
    return {r.id: S.census(r) for r in S.ROWS + S.SMALL_ROWS}


def test_rows_meet_the_regimes_they_claim(census):
    """A condition on the inputs, met by the oracle alone: every regime a row claims shows in the census of its
    config, seeds, stream and steps at chunk size G; the rows of one G provide every regime between them."""
    for r in S.ROWS + S.SMALL_ROWS:
        c = census[r.id]
        assert r.regimes, r.id
        for regime in r.regimes:
            for counter in S.REGIME_COUNTERS[regime]:
                assert c[counter] > 0, (r.id, regime, counter, c)
    for G in S.GS:
        have = {g for r in S.ROWS + S.SMALL_ROWS if r.G == G for g in r.regimes}
        assert set(S.NEED[G]) <= have, (G, have)
    # both paths inside one launch (and at G = 1 inside one workgroup)
    for rid in ("G4-k_step-brawl9@37", "G1-k_step-pen_quad@3"):
        assert census[rid]["lists"] > 0 and census[rid]["lists_serial"] > 0, census[rid]


def test_rows_meet_the_conflict_cases(census):
    for G in S.GS:
        tot = {k: sum(census[r.id][k] for r in S.ROWS + S.SMALL_ROWS if r.G == G) for k in S.CONFLICTS}
        for k in S.CONFLICTS_NEED[G]:
            assert tot[k] > 0, (G, k, tot)
    assert all(census[r.id]["obst_int16"] == 0 for r in S.ROWS)


def test_rows_respawn_and_reset(census):
    """Every config that keeps a minimum of zombies respawns during its rows' runs, and every env of every row is
    truncated at EPISODE steps or ends earlier: four autoresets or more in STEPS steps."""
    for r in S.ROWS:
        # (the fort config starts with twelve zombies and keeps eight: none of them dies within five steps)
        if r.make(1).cfg.minimum_zombies > 0 and r.config != "fort_bots":
            assert census[r.id]["respawns"] > 0, r.id
    assert S.STEPS // (S.EPISODE + 1) >= 4
