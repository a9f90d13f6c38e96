"""The action and death logs (ZS_FLAG_DEATH_LOG: zs_action_log, zs_death_log) of every step-kernel instantiation on
the GPU against the C oracle's (zo_set_logs), every env at every step: the rows of log_cases.py, whose census
test_log_plan.py takes on the CPU.  The logs are written by four pieces of zs_tick.hpp (the leader's serial loop,
its debug-raise exit, the lanes' chunked execution, env_cleanup_group<G>'s ballots), all inside the 21 k_step<G> /
k_tick<G, W> instantiations; the comparison runs beside step_runner.run_engines' comparison of observations,
rewards, flags and states, so a log that is wrong shows next to a state that is right.  Then the reading calls
themselves (a cap below the count), a graph launch of several steps, a handle without autoreset whose envs are
stepped on after they ended, and the host record's log sections.
"""
import ctypes as C

import numpy as np
import pytest

import log_cases as L
from libzombsole_amd import _abi
from step_runner import check_logs, run_engines

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("row", L.ALL_ROWS, ids=[r.id for r in L.ALL_ROWS])
def test_logs_of_instantiation(row):
    """One row, with the lanes' execution (par_exec 1) and with the leader's serial loop for every list (par_exec
    -1): 24 steps with autoreset, eager launches on the discrete rows and the replayed caller-actions graph on the
    others; both logs of every env of both engines against the oracle's after every step, and none on a reset."""
    pars = (1, -1)
    resets, _ = run_engines([row.builder(par_exec=p) for p in pars], row.make, row.seeds(), L.STEPS, row,
                            graph=row.stream != "discrete", states_at=(L.STEPS,),
                            expect=[row.describe(p) for p in pars], logs=True)
    assert sum(resets) >= row.n  # every env went through an autoreset (on average): reset steps were compared


def _stepped(make, n, seed0, until, max_steps=16):
    """An engine of `make` and its oracles, stepped (rich stream) until `until(eng, env)` holds for an env."""
    import torch
    from libzombsole_amd.engine import Engine
    row = L.LogRow(8, "k_step", "melee_bots", n)
    eng = Engine(make(n))
    seeds = [seed0 + i for i in range(n)]
    eng.seed(seeds)
    eng.reset()
    for t in range(1, max_steps + 1):
        eng.actions.copy_(torch.from_numpy(row.actions(seeds, t, eng.A)))
        eng.step()
        torch.cuda.synchronize()
        for e in range(n):
            if until(eng, e):
                return eng, e
    raise AssertionError("no env met the condition within %d steps" % max_steps)


@pytest.mark.parametrize("which", ["action", "death"])
def test_truncated_reads(which):
    """zs_action_log / zs_death_log with a cap below the count: *n_out is the full count, only cap entries are
    written (guard words behind them stay), and cap = 0 with out_host = NULL gives the count alone."""
    words = 2 if which == "action" else 5
    full = (lambda eng, e: eng.action_log(e)[0]) if which == "action" else (lambda eng, e: eng.death_log(e))
    eng, e = _stepped(L.melee_bots, 8, 4100, lambda eng, e: len(full(eng, e)) >= 3)
    call = eng.L.zs_action_log if which == "action" else eng.L.zs_death_log
    entries = [tuple(x) for x in full(eng, e)]
    count = len(entries)
    GUARD = 0x5A5A5A5A
    for cap in (0, 1, count - 1, count, count + 2):
        buf = (C.c_int32 * (words * (count + 2) + 4))(*([GUARD] * (words * (count + 2) + 4)))
        n = C.c_int32(-99)
        assert call(eng.h, e, buf, cap, C.byref(n), eng._stream()) == 0
        assert n.value == count, (cap, n.value, count)
        got = np.frombuffer(buf, dtype=np.int32)
        k = min(cap, count)
        assert (got[words * k:] == GUARD).all(), (cap, got)
        dec = _decode(which, got, k, eng.E)
        assert dec == entries[:k], (cap, dec, entries)
    n = C.c_int32(-99)
    assert call(eng.h, e, None, 0, C.byref(n), eng._stream()) == 0 and n.value == count
    assert call(eng.h, e, None, 1, C.byref(n), eng._stream()) == _abi.ZS_EINVAL  # a cap without a buffer is refused
    eng.close()


def _decode(which, words, n, E):
    from libzombsole_amd.engine import decode_action_log, decode_death_log
    return decode_action_log(words, n, E)[0] if which == "action" else decode_death_log(words, n, E)


def _oracles(make, seeds):
    from oracle.oracle import OracleEnv
    refs = []
    for s in seeds:
        o = OracleEnv(make(1))
        o.seed(s)
        o.reset()
        o.set_logs()
        refs.append(o)
    return refs


def test_multi_step_graph_keeps_the_last_steps_logs():
    """zs_step_graph_n with 4 steps a launch: the logs after the launch are the fourth step's.  A twin handle
    stepped eagerly gives the state before that step (held to the oracle's), which maps the slots to cells."""
    import torch
    from libzombsole_amd.engine import Engine
    n, per, launches = 9, 4, 4
    seeds = [5200 + i for i in range(n)]
    row = L.LogRow(8, "k_step", "melee", n)
    eng, twin = Engine(L.melee(n)), Engine(L.melee(n))
    kinds = [o[2] for o in eng.builder.map.obstacles]
    for e in (eng, twin):
        e.seed(seeds)
        e.reset()
    refs = _oracles(L.melee, seeds)
    need = [False] * n
    slots = eng.E - eng.A
    compared = removed = 0
    for launch in range(launches):
        t0 = 1 + launch * per
        eng.step_graph(t0, 7, steps=per)
        torch.cuda.synchronize()
        for t in range(t0, t0 + per):
            last = t == t0 + per - 1
            acts = row.actions(seeds, t, eng.A)
            if last:
                pre = [twin.get_state(k) for k in range(n)]
                for k, o in enumerate(refs):
                    assert pre[k].canonical(kinds) == o.state(), ("twin state", k, t)
            twin.gen_actions(t, 7)
            twin.step()
            for k, o in enumerate(refs):
                was_reset = need[k]
                if need[k]:
                    o.reset()
                    need[k] = False
                else:
                    _, _, d, tr, _ = o.step(acts[k])
                    need[k] = d or tr
                if last:
                    if was_reset:
                        assert eng.action_log(k) == ([], False) and eng.death_log(k) == [], (k, t)
                    else:
                        check_logs(eng, k, pre[k], eng.get_state(k), o, slots, (k, t))
                        compared += len(o.action_log()[1])
                        removed += len(o.death_log())
    assert compared > 100 and removed >= 3, (compared, removed)
    eng.close()
    twin.close()


def melee_kept(n):
    b = _abi.multi_env_config(n, "survival", [], L._melee(), ["0", "1", "2", "3"], initial_zombies=14,
                              minimum_zombies=14, agent_weapons=["shotgun", "axe", "shotgun", "rifle"],
                              max_episode_steps=6, autoreset=False)
    b.cfg.flags |= _abi.FLAG_DEATH_LOG
    return b


def test_logs_of_an_env_stepped_on_after_its_end():
    """A handle without ZS_FLAG_AUTORESET: every env is truncated at step 6 and stepped on to step 24 (some end by
    the rule as well, every player dead, and their zombies wander: deferred decisions); the logs follow the
    oracle's at every step."""
    row = L.LogRow(8, "k_tick5", "melee", 11)
    row.make, row.stream = melee_kept, "rich"
    resets, _ = run_engines([row.builder(par_exec=p) for p in (1, -1)], melee_kept, row.seeds(), L.STEPS, row,
                            states_at=(L.STEPS,), keep=True, logs=True)
    assert sum(resets) == 0


def test_host_record_logs_against_the_oracle():
    """The log sections of the host record (zs_host_step) of a handle of 5 envs against the oracle's, every env at
    every step; the record's state section gives the state after the step."""
    import torch
    from libzombsole_amd.engine import Engine, StateView, decode_action_log, decode_death_log
    n = 5
    seeds = [6300 + i for i in range(n)]
    row = L.LogRow(8, "k_tick6", "melee_bots", n)
    eng = Engine(row.builder())
    lay = eng.host_layout()
    scratch = Engine(row.builder())
    scratch.seed(seeds)
    rng = np.stack([scratch.get_rng(e) for e in range(n)]).astype(np.uint32)
    scratch.close()
    rec = eng.host_record()
    eng.host_reset(rng, rec)
    refs = _oracles(row.make, seeds)
    slots = eng.E - eng.A - eng.builder.num_bots
    pre = [StateView(eng, rec[e][lay["state"]:lay["state"] + eng.state_words].copy()) for e in range(n)]
    need = [False] * n
    compared = removed = 0

    class Rec(object):  # the record's log sections behind Engine's reading calls, for check_logs
        A, E, builder = eng.A, eng.E, eng.builder

        def __init__(self, r):
            self.r = r

        def action_log(self, k):
            return decode_action_log(self.r[k][lay["alog"]:], int(self.r[k][2]), eng.E)  # ZS_HOST_ALOG_N

        def death_log(self, k):
            return decode_death_log(self.r[k][lay["dlog"]:], int(self.r[k][3]), eng.E)  # ZS_HOST_DLOG_N

    for t in range(1, 19):
        acts = row.actions(seeds, t, eng.A)
        rec = eng.host_record()
        eng.host_step(acts, None, rec)
        torch.cuda.synchronize()
        view = Rec(rec)
        for k, o in enumerate(refs):
            post = StateView(eng, rec[k][lay["state"]:lay["state"] + eng.state_words].copy())
            if need[k]:
                o.reset()
                need[k] = False
                assert view.action_log(k) == ([], False) and view.death_log(k) == [], (k, t)
            else:
                _, _, d, tr, _ = o.step(acts[k])
                need[k] = d or tr
                check_logs(view, k, pre[k], post, o, slots, (k, t))
                compared += len(o.action_log()[1])
                removed += len(o.death_log())
            pre[k] = post
    assert compared > 500 and removed >= 10, (compared, removed)
    eng.close()
