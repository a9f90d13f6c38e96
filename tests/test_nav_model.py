"""The path-distance model on the CPU: libzombsole_amd/nav.py's field and encode against an independent, deliberately
naive BFS (nav_cases.naive_field: a deque over cells, no code shared with nav.py) on the oracle's states of every row of
the case table, every field and every cap; hand-built states for the rules a trace cannot be steered into; and the
census, by the oracle and the naive BFS alone, of the case classes the table shows."""
import numpy as np
import pytest

import nav_cases as NC
from entity_obs_cases import View, ent
from libzombsole_amd import _abi
from libzombsole_amd import nav as NV
from libzombsole_amd.entity_obs import Static


@pytest.mark.parametrize("row", sorted(NC.ROWS))
def test_model_equals_the_naive_bfs_on_the_oracle_states(row):
    views, _states, _census = NC.oracle_trace(row, 13)
    static = Static.of_map(NC.builder(row, 1).map)
    envs = range(13) if row != "fort_e132" else range(3)
    for t in range(len(views)):
        for k in envs:
            v = views[t][k]
            for cap in NC.caps_of(row):
                for which in (NV.OBJECTIVE, NV.ZOMBIES):
                    got, want = NV.field(v, static, which, cap), NC.naive_field(v, static, which, cap)
                    assert got.dtype == np.uint16 and got.shape == (static.H, static.W) and np.array_equal(got, want), (row, t, k, cap)
                for fields in (1, 2, 3):
                    got, want = NV.encode(v, static, fields, cap), NC.naive_rows(v, static, fields, cap)
                    assert got.dtype == np.int16 and np.array_equal(got, want), (row, t, k, cap, fields)


def test_every_class_occurs_in_three_envs_or_more():
    tot = NC.census_counts(13)
    for c in NC.CLASSES:
        assert tot[c] >= 3, (c, dict(tot))


def test_rows_show_what_they_are_in_the_table_for():
    _v, _s, census = NC.oracle_trace("wall5x4", 13)
    assert sum("obstacle_removed" in s for s in census) >= 3  # the wall that falls changes the field
    _v, _s, census = NC.oracle_trace("crowd9x7", 13)
    assert sum("absent_agent" in s for s in census) >= 3 and sum("obstacle_removed" in s for s in census) >= 3
    for row, cls in (("pocket_in", "unreachable"), ("pocket_out", "unreachable"), ("arduino", "unreachable"),
                     ("serpentine", "cut"), ("open33x3", "cut"), ("easy_exit", "tie")):
        assert sum(cls in s for s in NC.oracle_trace(row, 13)[2]) >= 3, (row, cls)
    b = NC.builder("fort_e132", 1)
    assert b.num_agents + b.num_bots + max(b.cfg.initial_zombies, b.cfg.minimum_zombies) > 64
    b = NC.builder("bridge_a4", 1)
    assert b.num_agents == 4 and b.num_bots == 2 and len(b.map.objectives) == 28
    assert not NC.builder("arduino", 1).map.objectives


def test_pockets_are_finite_in_one_field_and_unreachable_in_the_other():
    for row, closed, open_ in (("pocket_in", 0, 1), ("pocket_out", 1, 0)):
        views, _s, _c = NC.oracle_trace(row, 13)
        static = Static.of_map(NC.builder(row, 1).map)
        rows = NV.encode(views[0][0], static, 3)
        assert (rows[:, closed, 0] == -1).all() and (rows[:, closed, 5:7] == -1).all() and (rows[:, closed, 7] == 1).all()
        assert (rows[:, open_, 0] >= 0).all()


def test_serpentine_runs_longer_than_any_straight_line_bound_and_zombies_are_answered_first():
    """The objective field's distance at the agents exceeds W + H; the zombie queries are all answered many levels
    before the objective queries (the shared loop must not end the objective field with the zombie field)."""
    views, _s, _c = NC.oracle_trace("serpentine", 13)
    static = Static.of_map(NC.builder("serpentine", 1).map)
    for k in range(13):
        rows = NV.encode(views[0][k], static, 3).astype(int)
        obj, zom = rows[:, 0, :5], rows[:, 1, :5]
        assert obj[obj >= 0].min() > static.W + static.H
        assert zom[zom >= 0].max() + 40 <= obj[obj >= 0].min()
        cut = NV.encode(views[0][k], static, 3, 80).astype(int)
        assert (cut[:, 0, :5] == -1).all()  # 80 cuts the corridor in the middle: nothing of the objective field arrives
        assert np.array_equal(cut[:, 1, :5], np.where(rows[:, 1, :5] <= 80, rows[:, 1, :5], -1))
        assert NV.levels(views[0][k], static, NV.OBJECTIVE) == 168


def test_no_objectives_is_all_unreachable():
    views, _s, _c = NC.oracle_trace("arduino", 13)
    static = Static.of_map(NC.builder("arduino", 1).map)
    assert (NV.field(views[0][0], static, "objective") == NV.UNREACHED).all()
    rows = NV.encode(views[0][0], static, "objective")
    assert rows.shape == (2, 1, 8) and (rows[:, 0, :7] == -1).all() and (rows[:, 0, 7] == NV.PRESENT).all()


# ---- hand-built states --------------------------------------------------------------------------------------------------
def test_corner_edges_ties_sources_and_absent_agents():
    st = Static(5, 4, [], [(2, 1)])
    # agents: in the corner (0, 0), on the objective, on each edge, absent
    v = View(6, 0, [ent(1, 0, 0), ent(1, 2, 1), ent(1, 2, 0), ent(1, 0, 2), ent(1, 4, 1), ent(0, 2, 3)])
    rows = NV.encode(v, st, NV.OBJECTIVE)[:, 0].tolist()
    assert rows[0] == [3, 2, -1, -1, 2, 0, 0, 1]          # corner: (-1,0) and (0,-1) leave the map; a tie at both ends: k = 0
    assert rows[1] == [0, 1, 1, 1, 1, 0, 0, 1 | 2]        # own cell a source; four equal neighbours: the smallest k
    assert rows[2] == [1, 0, 2, -1, 2, 0, 1, 1]           # the edge y = 0; the maximum's tie: k = 1 before k = 3
    assert rows[3] == [3, 4, -1, 2, 2, 2, 0, 1]           # the edge x = 0; the minimum's tie: k = 2 before k = 3
    assert rows[4] == [2, 3, 1, 3, -1, 1, 0, 1]           # the edge x = 4
    assert rows[5] == [0] * 8                             # absent: flags bit 0 tells it from distance 0
    both = NV.encode(v, st, 3)
    assert both.shape == (6, 2, 8) and (both[:5, 1, :7] == -1).all()  # no zombies: that field is unreachable


def test_a_blocked_source_is_no_source_and_caps_cut():
    st = Static(6, 1, [(0, 0), (3, 0)], [(0, 0), (1, 0)])
    v = View(1, 0, [ent(1, 2, 0), ent(1, 5, 0)], [1, 1])
    assert NV.field(v, st, 1).tolist() == [[0xFFFF, 0, 1, 0xFFFF, 0xFFFF, 0xFFFF]]
    assert NV.field(v, st, 2).tolist() == [[0xFFFF] * 4 + [1, 0]]
    gone = View(1, 0, [ent(1, 2, 0), ent(1, 5, 0)], [0, 0])  # a removed obstacle opens the cell, and a source under it
    assert NV.field(gone, st, 1).tolist() == [[0, 0, 1, 2, 3, 4]]
    assert NV.field(gone, st, 1, 2).tolist() == [[0, 0, 1, 2, 0xFFFF, 0xFFFF]]
    assert NV.encode(gone, st, 3, 1)[0].tolist() == [[1, -1, 0, -1, -1, 1, 1, 1], [-1] * 7 + [1]]
    life0 = View(1, 0, [ent(1, 2, 0), ent(1, 5, 0)], [1, 1])  # presence alone counts, whatever the life
    assert np.array_equal(NV.field(life0, st, 1), NV.field(v, st, 1))


def test_arguments():
    st = Static(3, 3, [], [(0, 0)])
    v = View(1, 0, [ent(1, 1, 1)])
    for bad in (0, 4, -1, "players", ("objective", "x")):
        with pytest.raises(ValueError):
            NV.encode(v, st, bad)
    for bad in (0, -1, 32767):
        with pytest.raises(ValueError):
            NV.encode(v, st, 1, bad)
        with pytest.raises(ValueError):
            NV.field(v, st, 1, bad)
    with pytest.raises(ValueError):
        NV.field(v, st, 3)
    assert NV.fields_mask(("objective", "zombies")) == 3 and NV.fields_mask("zombies") == 2 and NV.field_bits(3) == [1, 2]
    assert (NV.OBJECTIVE, NV.ZOMBIES, NV.MAX_DIST, NV.ROW_WORDS) == (_abi.NAV_OBJECTIVE, _abi.NAV_ZOMBIES, _abi.NAV_MAX_DIST,
                                                                    _abi.NAV_ROW_WORDS)
    assert NV.DIRS == ((0, 1), (-1, 0), (0, -1), (1, 0))


def test_greedy_follower_on_easy_exit_in_the_oracle():
    """The condition test_nav.py's follower test rests on, shown with the model and the oracle alone for its seeds:
    following word 5 while word 0 > 0 (else heal), an agent's word 0 never increases while its env is not reset and it
    stays in the world, every fall is by exactly one, and the 13 envs make progress."""
    from libzombsole_amd import actions as A
    from oracle.oracle import OracleEnv
    import entity_obs_cases as EC

    def mk():
        return _abi.multi_env_config(1, "extermination", [], "easy_exit", ["0", "1"], initial_zombies=4, minimum_zombies=4)

    b = mk()
    static = Static.of_map(b.map)
    assert not b.map.obstacles  # nothing but the agent's own move changes its distance
    fell = 0
    for k in range(13):
        o = OracleEnv(mk())
        o.seed(NC.SEED0 + k)
        o.reset()
        rows = NV.encode(EC.oracle_view(b, o.state()), static, "objective")[:, 0].astype(int)
        for _t in range(8):
            ids = [int(r[5]) if r[0] > 0 and r[5] >= 0 else 5 for r in rows]
            _obs, _r, d, tr, _l = o.step(np.stack([A.DISCRETE_TRIPLES[i] for i in ids]))
            if d or tr:
                break
            new = NV.encode(EC.oracle_view(b, o.state()), static, "objective")[:, 0].astype(int)
            for a in range(2):
                if rows[a][7] & 1 and new[a][7] & 1:
                    assert new[a][0] <= rows[a][0] and new[a][0] >= rows[a][0] - 1, (k, a)
                    fell += new[a][0] < rows[a][0]
            rows = new
    assert fell >= 13
