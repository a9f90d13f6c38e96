"""The runner shared by the GPU tests that step engines against the C oracle (test_step_instantiations.py,
test_terminal_outcomes.py): guard bands round every buffer zs_step writes, and one OracleEnv per env compared at
every step.

Guard bands: rewards, done, truncated, listed, the reset flag and the actions each lie inside a byte tensor
filled with 0x5A, 64 B before and after.  Before every step the payloads are filled with 0x5A too: 0x5A is no
value done, truncated, listed or the reset flag can hold, so after the step every such byte of every env must
have been written, and every guard byte must still be 0x5A (a partial workgroup's idle lanes are where a store
past the last env would come from).
"""
import numpy as np

from test_obs_instantiations import FILL, GUARD


class Band(object):
    """A tensor of `shape` and `dtype` at byte GUARD of a 0x5A-filled byte tensor with GUARD bytes after it."""

    def __init__(self, eng, shape, dtype):
        torch = eng.torch
        self.nbytes = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        self.raw = torch.full((GUARD + self.nbytes + GUARD,), FILL, dtype=torch.uint8, device=eng.device)
        assert self.raw.data_ptr() % 16 == 0 and GUARD >= 64 and GUARD % 8 == 0
        self.view = self.raw[GUARD:GUARD + self.nbytes].view(dtype).view(shape)
        assert self.view.data_ptr() == self.raw.data_ptr() + GUARD

    def guards_hold(self):
        raw = self.raw.cpu().numpy()
        return bool((raw[:GUARD] == FILL).all() and (raw[GUARD + self.nbytes:] == FILL).all())


class GuardedStep(object):
    """The output set of Engine.step / step_graph (obs, rewards, done, trunc, listed, was_reset) and the action
    tensor, each but the observations (test_obs_instantiations.py guards those) inside its own Band."""
    FLAGS = ("done", "trunc", "listed", "was_reset")

    def __init__(self, eng):
        torch = eng.torch
        n, a = eng.N, eng.A
        self.bands = {"rewards": Band(eng, (n, a if eng.multi else 1), torch.float64),
                      "done": Band(eng, (n,), torch.uint8), "trunc": Band(eng, (n,), torch.uint8),
                      "listed": Band(eng, (n, a), torch.uint8), "was_reset": Band(eng, (n,), torch.uint8),
                      "actions": Band(eng, (n, a, 3), torch.int32)}
        for k, b in self.bands.items():
            setattr(self, k, b.view)
        self.obs = eng.obs

    def clear(self):
        """0x5A over every output payload (not the actions, which the step reads)."""
        for k, b in self.bands.items():
            if k != "actions":
                b.raw.fill_(FILL)

    def check(self, what):
        for k, b in self.bands.items():
            assert b.guards_hold(), ("guard bytes written", k, what)
        for k in self.FLAGS:  # every env's flags were stored
            v = getattr(self, k).cpu().numpy()
            assert (v != FILL).all(), ("flag bytes never written", k, what, np.argwhere(v == FILL)[:8].tolist())


def removed_by_oracle(prev, cur, A):
    """What a step of the oracle removed, from its states before and after: (the number of things and obstacles
    gone, the obstacles among them, {(slot, x, y, life)} of the players that died, the number of zombies that
    died, the cells that hold a body now and held none before)."""
    ob_prev = {o[0] for o in prev["obst"] if not o[2]}
    n_obst = sum(1 for o in cur["obst"] if not o[2] and o[0] not in ob_prev)
    slots = list(range(A)) + list(range(A, A + len(cur["players"])))
    players = {(s, p[0], p[1], p[2]) for s, q, p in zip(slots, prev["agents"] + prev["players"],
                                                        cur["agents"] + cur["players"]) if q[2] > 0 >= p[2]}
    return (cur["ctr"][1] - prev["ctr"][1], n_obst, players, cur["ctr"][2] - prev["ctr"][2],
            set(cur["dead"]) - set(prev["dead"]))


def check_death_log(log, prev, cur, A, W, where):
    """An engine's death log of one step ([(slot, serial, x, y, life)]) against what the oracle removed."""
    gone, n_obst, players, n_zombies, new_cells = removed_by_oracle(prev, cur, A)
    P = len(cur["players"])
    assert len(log) == gone - n_obst, ("death log count", where, log, gone, n_obst)
    assert {(s, x, y, life) for s, _, x, y, life in log if s < A + P} == players, ("death log players", where, log)
    zs = [e for e in log if e[0] >= A + P]
    assert len(zs) == n_zombies and len(zs) + len(players) == len(log), ("death log zombies", where, log)
    assert len({e[0] for e in log}) == len(log) and all(e[4] <= 0 for e in log), ("death log entries", where, log)
    cells = {y * W + x for _, _, x, y, _ in log}
    assert new_cells <= cells <= set(cur["dead"]), ("death log cells", where, log, cur["dead"])


def engine_action_log(log, pre):
    """An engine's action log ([(slot, kind, target)], Engine.action_log) in the oracle's canonical form
    (OracleEnv.action_log without its last field): every thing named by its cell in `pre`, the engine's own state
    from before the step."""
    rows = []
    for slot, kind, tgt in log:
        r = pre.ent[slot]
        assert int(r[1]), ("the actor's slot was empty before the step", slot)
        if kind == 1:
            x = tgt & 0xffff
            target = ("cell", x - 0x10000 if x >= 0x8000 else x, tgt >> 16)
        elif tgt < 0:
            target = ("obst", -1 - tgt)
        else:
            assert int(pre.ent[tgt][1]), ("the target's slot was empty before the step", slot, tgt)
            target = ("thing", int(pre.ent[tgt][2]), int(pre.ent[tgt][3]))
        rows.append(((int(r[2]), int(r[3])), int(r[0]), kind, target))
    return rows


def check_logs(eng, k, pre, post, o, zombie_slots, where):
    """Both logs of env k's last step against the oracle's (OracleEnv.set_logs), entry by entry and in order.
    Actions: the count (-1 - j after a debug raise), and every entry's actor, kind and target.  Deaths: agent / bot
    index or zombie, x, y and life at removal; the entry's slot held that thing in the engine's state before the
    step (its cell there is the oracle's pre-step cell of the thing), the entry's serial is the slot's serial
    there, and a zombie slot that is taken again after the step carries another serial.  pre, post: the engine's
    states before and after the step.  Returns whether the step refilled a removed zombie's slot."""
    A, P = eng.A, eng.builder.num_bots
    n, rows, _ = o.action_log()
    acts, raised = eng.action_log(k)
    got = engine_action_log(acts, pre)
    assert (-1 - len(got) if raised else len(got)) == n, ("action log count", where, n, acts, raised)
    assert got == [r[:4] for r in rows], ("action log", where, got, rows)
    exp = o.death_log()
    log = eng.death_log(k)
    assert len(log) == len(exp), ("death log count", where, log, exp)
    reused = False
    for (slot, serial, x, y, life), (kind, idx, ex, ey, elife, cell) in zip(log, exp):
        who = (7, slot) if slot < A else (6, slot - A) if slot < A + P else (5, -1)  # ZS_THING_AGENT, _PLAYER, _ZOMBIE
        assert (who, x, y, life) == ((kind, idx), ex, ey, elife), ("death log entry", where, log, exp)
        r = pre.ent[slot]
        assert int(r[1]) and int(r[0]) == kind and (int(r[2]), int(r[3])) == cell, ("death log slot", where, slot, r, cell)
        assert int(r[7]) == serial, ("death log serial", where, slot, serial, r)
        if slot >= A + P and int(post.ent[slot][1]):
            assert int(post.ent[slot][7]) != serial, ("a refilled slot kept its serial", where, slot, serial)
            reused = True
    if any(e[0] == 5 for e in exp) and sum(int(r[1]) for r in post.ent[A + P:]) == zombie_slots:
        # every zombie slot is taken after the step: each removed zombie's slot was refilled
        assert all(int(post.ent[e[0]][1]) for e in log if e[0] >= A + P), ("slot reuse", where, log)
    return reused


def run_engines(builders, make_oracle, seeds, steps, stream_row, graph=False, states_at=(), expect=None,
                terminal=False, after_step=None, keep=False, logs=False):
    """One engine per builder (the same config and seeds under different launch overrides), stepped in lock step
    and each compared with one OracleEnv per env at every step: the reset observation; observations, rewards
    (bit-exact, the listed ones), done, truncated, the autoreset flag and `listed`; the canonical state of every
    env at the steps `states_at`.  expect: per builder, the describe() fields it must report.  terminal: also the
    state of every env at the step it ends or is truncated (the pending env still shows the terminal world) and
    at the step of its autoreset, with ZS_FLAG_DEATH_LOG the death log of the terminal step against the things the
    oracle removed, and after the last step every env's RNG stream.  keep: the builders hold no
    ZS_FLAG_AUTORESET; an env that ended is stepped on, in the engines and in the oracle, and never reset.  after_step(t, engs, refs): called after the
    comparisons of step t (and with t = 0 after the reset).  logs: the builders hold ZS_FLAG_DEATH_LOG; both logs of
    every env of every engine are compared with the oracle's after every step (check_logs; a reset step reports
    none), and a step the oracle stops at a debug raise is compared in what it defines: zero rewards, no flag,
    the state.  A stream other than "discrete" goes through step_graph
    with no policy: the graph replays the step on the guarded action tensor, filled before every call.  Returns
    per step (1-based; index 0 unused) the number of envs the oracle reset and the number it respawned zombies
    in."""
    import torch
    from libzombsole_amd.engine import Engine
    from oracle.oracle import OracleEnv, OracleRaised

    n = len(seeds)
    engs, outs = [], []
    for i, b in enumerate(builders):
        eng = Engine(b)
        if expect:
            desc = eng.describe()
            assert {k: desc[k] for k in expect[i]} == expect[i], (i, desc)
        eng.seed(seeds)
        engs.append(eng)
        outs.append(GuardedStep(eng))
    kinds = [o[2] for o in engs[0].builder.map.obstacles]
    A = engs[0].A
    refs = []
    obs0 = [eng.reset().cpu().numpy() for eng in engs]
    for k, s in enumerate(seeds):
        o = OracleEnv(make_oracle(1))
        o.seed(s)
        exp = o.reset()
        for i in range(len(engs)):
            assert np.array_equal(obs0[i][k], exp), ("reset obs", i, k)
        if logs:
            o.set_logs()
        refs.append(o)
    if after_step:
        after_step(0, engs, refs)
    pre = [[eng.get_state(k) for k in range(n)] for eng in engs] if logs else None
    zombie_slots = engs[0].E - A - engs[0].builder.num_bots
    need = [False] * n
    resets, respawns, respawned = [0] * (steps + 1), [0] * (steps + 1), [0] * n
    dlog = terminal and all(e.builder.cfg.flags & 4 for e in engs)  # _abi.FLAG_DEATH_LOG
    W = engs[0].builder.map.size[0]
    before = [o.state() for o in refs] if dlog else None
    for t in range(1, steps + 1):
        got = []
        for i, (eng, out) in enumerate(zip(engs, outs)):
            out.clear()
            if graph and stream_row.stream == "discrete":
                # the policy's actions are generated inside the replayed graph, into the guarded tensor
                eng.step_graph(t, 7, out=out, actions=out.actions)
            elif graph:
                out.actions.copy_(torch.from_numpy(stream_row.actions(seeds, t, A)))
                eng.step_graph(t, 0, out=out, actions=out.actions)
            else:
                if stream_row.stream == "discrete":
                    eng.gen_actions(t, 7, out=out.actions)
                else:
                    out.actions.copy_(torch.from_numpy(stream_row.actions(seeds, t, A)))
                eng.step(actions=out.actions, out=out)
            torch.cuda.synchronize()
            out.check((i, t))
            got.append({k: getattr(out, k).cpu().numpy() for k in
                        ("obs", "rewards", "done", "trunc", "listed", "was_reset", "actions")})
        acts = got[0]["actions"]
        for g in got[1:]:
            assert np.array_equal(g["actions"], acts)
        if stream_row.stream == "discrete":  # zs_gen_actions' stream is the oracle's (run_hashes, the CPU census)
            assert np.array_equal(acts[::max(1, n // 3)], stream_row.actions(seeds[::max(1, n // 3)], t, A))
        for k, o in enumerate(refs):
            if need[k]:
                exp, r, d, tr, lb = o.reset(), None, False, False, np.ones(A, bool)
                need[k] = False
                resets[t] += 1
            else:
                try:
                    exp, r, d, tr, lb = o.step(acts[k])
                except OracleRaised as err:
                    assert logs
                    exp, r, d, tr, lb = None, np.zeros(max(A, 1)), False, False, err.args[0]
                need[k] = (d or tr) and not keep
                c = o.census()["respawns"]
                respawns[t] += c != respawned[k]
                respawned[k] = c
            for i, g in enumerate(got):
                assert bool(g["was_reset"][k]) == (r is None), ("autoreset flag", i, k, t)
                assert bool(g["done"][k]) == d and bool(g["trunc"][k]) == tr, ("flags", i, k, t)
                assert np.array_equal(g["listed"][k].astype(bool), lb), ("listed", i, k, t)
                if r is None:
                    assert not g["rewards"][k].any(), ("rewards of a reset", i, k, t)
                else:
                    assert np.array_equal(g["rewards"][k][lb].view(np.uint64), r[:A][lb].view(np.uint64)), \
                        ("rew", i, k, t, g["rewards"][k], r)
                if exp is None:  # a debug raise: of the step's outputs only the state is defined
                    assert not g["rewards"][k].any(), ("rewards of a raise", i, k, t)
                    assert engs[i].get_state(k).canonical(kinds) == o.state(), ("state after a raise", i, k, t)
                else:
                    assert np.array_equal(g["obs"][k], exp), ("obs", i, k, t)
            if logs:
                for i, eng in enumerate(engs):
                    post = eng.get_state(k)
                    if r is None:
                        assert eng.action_log(k) == ([], False) and eng.death_log(k) == [], ("logs of a reset", i, k, t)
                        assert o.action_log()[0] == 0 and o.death_log() == []
                    else:
                        check_logs(eng, k, pre[i][k], post, o, zombie_slots, (i, k, t))
                    pre[i][k] = post
            if terminal and (need[k] or r is None):
                st = o.state()
                for i, eng in enumerate(engs):
                    assert eng.get_state(k).canonical(kinds) == st, ("terminal state" if need[k] else "reset state", i, k, t)
                    if dlog and need[k]:
                        check_death_log(eng.death_log(k), before[k], st, A, W, (i, k, t))
            if dlog:
                before[k] = o.state()
        if after_step:
            after_step(t, engs, refs)
        if t in states_at:
            for i, eng in enumerate(engs):
                for k, o in enumerate(refs):
                    assert eng.get_state(k).canonical(kinds) == o.state(), ("state", i, k, t)
    if terminal:
        for i, eng in enumerate(engs):
            for k, o in enumerate(refs):
                assert np.array_equal(eng.get_rng(k), o.get_rng()), ("rng stream", i, k)
    for eng in engs:
        eng.close()
    return resets, respawns
