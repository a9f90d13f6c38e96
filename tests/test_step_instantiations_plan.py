"""The case table of step_instantiations.py on the CPU: the rows and the justified unreachable entries are the 21
device functions of k_tick_g.hip; every row's requested lanes-per-env count fits its LDS image, so choose_layout()
(engine.hip) keeps it; the env counts give partial workgroups; and the oracle's census of every row's own config,
seeds, action stream and steps shows the action-list regimes and the conflict cases the rows claim."""
import os

import pytest

import step_instantiations as S

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
    with open(os.path.join(CSRC, "engine.hip")) as f:
        src = f.read()
    for key, cond in S.UNREACHABLE.items():  # every unreachable entry quotes a condition that stands in the source
        assert cond and cond in src, key
    # launches of less than one workgroup: one per kernel kind
    assert {r.step_kernel for r in S.SMALL_ROWS} == {"k_step", "k_tick"}
    assert {(r.G, r.n) for r in S.SMALL_ROWS} == {(1, 3), (16, 1)}
    assert len({r.id for r in S.ROWS + S.SMALL_ROWS}) == len(S.ROWS) + len(S.SMALL_ROWS)


def test_overrides_are_the_ones_the_layout_reads():
    """The conditions the table's expectations were written from still stand in create_step_layout() /
    choose_layout() / zs_describe()."""
    with open(os.path.join(CSRC, "engine.hip")) as f:
        src = f.read()
    for cond in ("h->fused = h->ov.fused ? h->ov.fused > 0 :",
                 "if (h->ov.tick_waves > 0) h->tick_waves = h->ov.tick_waves == 5 ? 5 : 6;",
                 "for (int G = g0; G <= 64; G *= 2) {",
                 "if (bytes > kMax) continue;",
                 "h->fused ? ZS_FUSED_WAVES : h->tick_waves",
                 "d.defer_respawn = d.minimum_zombies > 0 && (dr ? dr > 0 : cands > 64);",
                 "d.par_exec = h->ov.par_exec >= 0;"):
        assert cond in src, cond
    with open(os.path.join(CSRC, "zs_device.hpp")) as f:
        assert "#define ZS_FUSED_WAVES 3" in f.read()
    for r in S.ROWS + S.SMALL_ROWS:
        assert r.launch["fobs"] == -1 and r.launch["fused"] == (1 if r.fused else -1)
        assert r.launch.get("tick_waves", 0) == (0 if r.fused else r.tick_waves)
        assert r.describe()["tick_waves"] == (3 if r.fused else int(r.kernel[-1]))


def test_requested_lanes_fit_their_image():
    """choose_layout() raises a requested G only when not even the smallest image of 64 / G envs fits 64 KiB."""
    for r in S.ROWS + S.SMALL_ROWS:
        b = r.builder(1)
        assert S.min_image_bytes(b, r.G, r.fused) <= 64 * 1024, (r.id, S.min_image_bytes(b, r.G, r.fused))
    # the arithmetic bites: city128's bitmap alone (512 words an env) fills 64 KiB with 32 envs, so the city128
    # rows start at G = 16; and bridge64's 12 entities leave 64 envs to an image little room (the c2 row of G = 1)
    assert S.min_image_bytes(S.c4(1), 1, False) > S.min_image_bytes(S.c4(1), 2, False) > 64 * 1024
    assert S.min_image_bytes(S.c4(1), 4, True) <= 64 * 1024
    assert 56 * 1024 < S.min_image_bytes(S.c2(1), 1, False) <= 64 * 1024 < S.min_image_bytes(S.c5(1), 1, False)


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
