"""The step plan (libzombsole_amd/csrc/zs_step_plan.hpp) on the CPU: the header compiled with the host compiler into
tests/step_plan_dump.cpp, every (shape, overrides) pair of step_plan_table against what the engine's layout
functions resolved it to before the plan existed (step_plan_expected.json)."""
import pytest

import step_plan_table as T
from libzombsole_amd import _abi

PAIRS = T.pairs()


@pytest.fixture(scope="module")
def rows():
    return T.resolve(PAIRS)


def test_matrix_is_the_one_asked_for():
    names = {n for n, _ in PAIRS}
    for cfg, firsts in T.FLIPS.items():  # the last env count before and the first after every flip
        for n in firsts:
            assert {"%s@%d" % (cfg, n - 1), "%s@%d" % (cfg, n)} <= names
    assert {"c3@%d" % n for n in (8192, 12288, 16384, 24576, 32768, 49152, 65536)} <= names
    assert len(PAIRS) == len({(n, T.ov_key(lo)) for n, lo in PAIRS})
    for lo in T.OVERRIDES:  # every set of overrides with the c3, c5, c4 and pen shapes (and the rest of CORE)
        for shape in T.CORE:
            assert (shape, T.ov_key(lo)) in {(n, T.ov_key(l)) for n, l in PAIRS}
    assert set(k for lo in T.OVERRIDES for k in lo) - {"lanes_per_env"} <= set(_abi.LAUNCH_FIELDS)


def test_rows_match_the_table(rows):
    bad = []
    for (shape, lo), got in zip(PAIRS, rows):
        exp = T.expected(shape, lo)
        assert "error" not in exp, (shape, lo)
        if got["obs_bytes"] != exp["obs_bytes"] or {k: got.get(k) for k in T.FIELDS} != {k: exp[k] for k in T.FIELDS}:
            bad.append((shape, lo, got, exp))
    assert not bad, bad[:5]


def test_rows_fit_and_are_resident(rows):
    for (shape, lo), r in zip(PAIRS, rows):
        assert 0 < r["lds"] <= 64 * 1024 and r["resident"] >= 1, (shape, lo, r)
        assert r["G"] in (1, 2, 4, 8, 16, 32, 64) and 1 <= r["want"] <= 32, (shape, lo, r)


def test_the_table_meets_every_decision():
    """Both outcomes of every decision the matrix is built round occur in the table (defaults unless named)."""
    def row(shape, lo=None):
        return T.expected(shape, lo or {})
    assert (row("c3@24576")["G"], row("c3@24577")["G"]) == (8, 8)  # the retry's 8, then the automatic 8
    assert (row("c3@11264")["G"], row("c3@11265")["G"]) == (16, 8)  # 8 instead of 16 ...
    assert (row("c3@22528")["G"], row("c3@22529")["G"], row("c3@23553")["G"]) == (8, 16, 8)  # ... and its fallback
    assert (row("c3@47104")["fused"], row("c3@47105")["fused"]) == (1, 0)
    assert (row("c3@49152")["G"], row("c3@49153")["G"]) == (16, 8)  # automatic G, unfused
    assert (row("c3@49152")["tick_waves"], row("c3@49153")["tick_waves"]) == (6, 5)
    assert (row("c5@24576")["tick_waves"], row("c5@24577")["tick_waves"], row("c5@40961")["tick_waves"]) == (6, 5, 6)
    assert (row("c5@23552")["fused"], row("c5@23553")["fused"]) == (1, 0)
    assert (row("c4@11776")["fused"], row("c4@11777")["fused"]) == (1, 0)
    for a, b in (("c3@63488", "c3@63489"), ("c5@31744", "c5@31745"), ("c4@15872", "c4@15873")):
        assert row(a)["want"] == 31 and row(b)["want"] == 32
    assert any(T.expected(n, lo)["obs_bytes"] > 0 for n, lo in PAIRS)  # the step launch's observation image


def test_no_image_fits_is_an_error():
    """A map near the 2^24-cell limit: one env's bitmap alone (DW words) is 2 MiB, so not even the G = 64 image of
    one env, with a 32-word window and no optional copy, fits 64 KiB, and the plan says so instead of a layout."""
    W, H, E, A = 4096, 4095, 12, 2
    cells = W * H
    DW = (cells + 31) // 32
    assert cells <= 1 << 24
    smallest, = T.images([(0, 1, E, DW, 32, 0, 0, A, cells, 0)])
    assert smallest["tick"] > 64 * 1024
    ints = [64, W, H, E, A, DW, cells, 0, 0, 0, 0, 0] + [0] * len(_abi.LAUNCH_FIELDS)
    row, = T.dump("step_plan_dump", ["P " + " ".join(str(v) for v in ints)])
    assert row.get("error") and "G" not in row, row
    # forcing the lanes or the kernel changes nothing
    ints[10] = 64
    ints[12 + _abi.LAUNCH_FIELDS.index("fused")] = -1
    row, = T.dump("step_plan_dump", ["P " + " ".join(str(v) for v in ints)])
    assert row.get("error"), row
