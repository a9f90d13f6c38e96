"""Snapshot records on one MI355X: zs_snapshot / zs_restore and BatchedZombsole.clone against the C oracle.

Every env is driven by the bench policy's host twin (libzombsole_amd/actions.py) with episodes of five steps and
followed by an OracleEnv.  A masked reset of every other env after step 2 puts the envs out of phase: half of
them are pending their autoreset after steps 6, 12, ..., the other half after steps 7, 13, ...; the tests take their
snapshots at such steps and assert that some envs are pending and some are not.  A Follower keeps the log of what happened to its
env (resets and action triples), so the oracle of a rewound or forked env is a fresh OracleEnv replayed through the
source's log.
"""
import numpy as np
import pytest

from libzombsole_amd import _abi
from libzombsole_amd import actions as A
from test_obs_state import _bridge64, _bridge_single, _city128, _wall_hp

pytestmark = pytest.mark.gpu

I64, I16 = _abi.DTYPE_I64, _abi.DTYPE_I16
WALL_POKES = ((5, -32700), (6, -32768), (7, -32769), (8, -40000), (9, -33000))


def _death_log(n, **kw):
    b = _bridge64(2, 10, I64)(n, **kw)
    b.cfg.flags |= _abi.FLAG_DEATH_LOG
    return b


# id -> (config builder, envs, policy size, obstacle pokes)
SHAPES = {
    "bridge64_a2_z10_i64": (_bridge64(2, 10, I64), 37, 7, ()),
    "bridge64_a4_z20_i16": (_bridge64(4, 20, I16), 67, 7, ()),
    "bridge_single_E7": (_bridge_single, 13, 6, ()),       # E = 7: the byte rows of env e start at byte 7 e
    "city128_a4_z50": (_city128, 13, 7, ()),               # long sections, respawn by k_respawn
    "wall_hp_i16": (_wall_hp(I16), 13, 7, WALL_POKES),     # int32 lives below the int16 floor, int16 observations
    "bridge64_death_log": (_death_log, 13, 7, ()),
}
OUT_KEYS = ("obs", "rewards", "done", "trunc", "listed", "was_reset")


class Follower(object):
    """One env's oracle and the log that built it."""

    def __init__(self, mk, seed, pokes, log=()):
        from oracle.oracle import OracleEnv
        self.mk, self.seed, self.pokes = mk, seed, pokes
        self.o = OracleEnv(mk(1))
        for i, life in pokes:
            self.o.poke_obstacle(i, life)
        self.o.seed(seed)
        self.need, self.log = True, []  # a new handle's envs are pending
        for ev in log:
            self.apply(ev)

    def apply(self, ev):
        """ev: "reset" (a masked zs_reset) or the action triples of a step.  Returns what the engine must report:
        (obs, rewards or None for a reset, done, truncated, listed, was_reset)."""
        self.log.append(ev)
        if isinstance(ev, str) or self.need:
            self.need = False
            return self.o.reset(), None, False, False, np.ones(self.o.A, bool), not isinstance(ev, str)
        obs, r, d, tr, lb = self.o.step(ev)
        self.need = d or tr
        return obs, r, d, tr, lb, False

    def fork(self, upto=None):
        return Follower(self.mk, self.seed, self.pokes, self.log[:upto])


class Sim(object):
    """An engine of n envs, one Follower per env, stepped together and compared at every step."""

    def __init__(self, mk, n, nd, pokes=(), seed0=4000, **kw):
        from libzombsole_amd.engine import Engine
        self.eng = Engine(mk(n, **kw), device=0)
        self.torch = self.eng.torch
        self.n, self.nd, self.t = n, nd, 0
        self.seeds = [seed0 + 3 * i for i in range(n)]
        self.eng.seed(self.seeds)
        for e in range(n if pokes else 0):
            st = self.eng.get_state(e)
            for i, life in pokes:
                st.obst_life[i] = life
            self.eng.set_state(e, st)
        self.f = [Follower(mk, s, pokes) for s in self.seeds]
        self.kinds = [o[2] for o in self.eng.builder.map.obstacles]

    def actions(self, t):
        return np.array([[A.DISCRETE_TRIPLES[A.discrete_action_id(s, t, a, self.nd)] for a in range(self.eng.A)]
                         for s in self.seeds], dtype=np.int32)

    def step(self, acts=None, graph=False, follow=True):
        """One step on `acts` (default: the policy's at the next step number); returns (acts, outputs as numpy)."""
        eng, torch = self.eng, self.torch
        self.t += 1
        acts = self.actions(self.t) if acts is None else acts
        eng.actions.copy_(torch.from_numpy(acts))
        (eng.step_graphed if graph else eng.step)(eng.actions)
        torch.cuda.synchronize()
        got = {k: getattr(eng.out, k)[:self.n].cpu().numpy().copy() for k in OUT_KEYS}
        if follow:
            for k, f in enumerate(self.f):
                self.check(k, f.apply(acts[k]), got)
        return acts, got

    def check(self, k, exp, got):
        obs, r, d, tr, lb, was_reset = exp
        what = (k, self.t)
        assert bool(got["was_reset"][k]) == was_reset, ("was_reset",) + what
        assert bool(got["done"][k]) == d and bool(got["trunc"][k]) == tr, ("flags",) + what
        assert np.array_equal(got["listed"][k].astype(bool), lb), ("listed",) + what
        if r is None:
            assert not got["rewards"][k].any(), ("rewards of a reset",) + what
        else:
            nr = got["rewards"].shape[1]
            sel = lb[:nr] if nr > 1 else np.ones(1, bool)
            assert np.array_equal(got["rewards"][k][sel].view(np.uint64), r[:nr][sel].view(np.uint64)), ("rew",) + what
        assert np.array_equal(got["obs"][k], obs), ("obs",) + what

    def masked_reset(self, envs):
        mask = self.torch.zeros(self.n, dtype=self.torch.uint8)
        mask[list(envs)] = 1
        obs = self.eng.reset(mask.to(self.eng.device)).cpu().numpy()
        for k in envs:
            assert np.array_equal(obs[k], self.f[k].apply("reset")[0]), ("masked reset", k)

    def warm_up(self, steps, graph=False):
        """`steps` steps with the masked resets that put the envs out of phase (see the module docstring)."""
        for _ in range(steps):
            self.step(graph=graph)
            if self.t == 1 and all(f.need for f in self.f):  # every episode is one step long (wall_hp): a third first
                self.masked_reset(range(0, self.n, 3))
            if self.t == 2:
                self.masked_reset(range(0, self.n, 2))

    def pending(self):
        return [k for k, f in enumerate(self.f) if f.need]

    def state(self, e):
        return self.eng.get_state(e).buf.copy(), self.eng.get_rng(e)

    def check_states(self):
        for k, f in enumerate(self.f):
            assert self.eng.get_state(k).canonical(self.kinds) == f.o.state(), ("state", k, self.t)
            assert np.array_equal(self.eng.get_rng(k), f.o.get_rng()), ("stream", k, self.t)

    def close(self):
        self.eng.close()


def _guarded(torch, dev, rows, nb, fill=0x5A):
    big = torch.full((64 + rows * nb + 64,), fill, dtype=torch.uint8, device=dev)
    return big, big[64:64 + rows * nb].view(rows, nb)


def _guards_hold(big, fill=0x5A):
    return bool((big[:64] == fill).all()) and bool((big[-64:] == fill).all())


def _check_record(eng, r, e):
    """One record (numpy bytes) against zs_get_state / zs_get_rng of env e, through the layout's offsets."""
    L, E, Ag = eng.snapshot_layout(), eng.E, eng.A
    st, rng = eng.get_state(e), eng.get_rng(e)

    def sec(name, nbytes, dt):
        return r[L[name]:L[name] + nbytes].copy().view(dt)
    scal = sec("scal", 36, np.int32)
    b = st.buf
    assert list(scal[:8]) == [b[0], b[1], b[2], b[3], b[4], b[5], b[10], b[12]], ("scal", e, list(scal), list(b[:13]))
    pos = sec("pos", 4 * E, np.int32)
    assert np.array_equal((pos & 0xffff).astype(np.int16).astype(np.int32), st.ent[:, 2]), ("x", e)
    assert np.array_equal(pos >> 16, st.ent[:, 3]), ("y", e)
    assert np.array_equal(sec("life", 4 * E, np.int32), st.ent[:, 4]), ("life", e)
    assert np.array_equal(sec("serial", 4 * E, np.int32), st.ent[:, 7]), ("serial", e)
    assert np.array_equal(sec("weapon", E, np.uint8).astype(np.int32), st.ent[:, 5]), ("weapon", e)
    assert np.array_equal(sec("present", E, np.uint8).astype(np.int32), st.ent[:, 1]), ("present", e)
    assert np.array_equal(sec("order", E, np.uint8).astype(np.int32), st.order), ("order", e)
    assert np.array_equal(sec("prev_life", 4 * Ag, np.int32), st.prev_life), ("prev_life", e)
    assert np.array_equal(sec("listed", Ag, np.uint8).astype(np.int32), st.listed), ("listed", e)
    dw = len(st.dead_words)
    assert np.array_equal(sec("dead", 4 * dw, np.uint32), st.dead_words.view(np.uint32)), ("dead", e)
    ow = (st.O + 31) // 32
    bits = np.unpackbits(sec("obst_present", 4 * ow, np.uint32).view(np.uint8), bitorder="little")[:st.O]
    assert np.array_equal(bits.astype(np.int32), st.obst_present), ("obst_present", e)
    hp = sec("obst_hp", 4 * st.O, np.int32)
    assert np.array_equal(hp, st.obst_life), ("obst_hp", e)
    nonpos = np.unpackbits(sec("obst_nonpos", 4 * ow, np.uint32).view(np.uint8), bitorder="little")[:st.O]
    assert not (nonpos.astype(bool) & (hp > 0)).any(), ("obst_nonpos marks a positive life", e)
    rngst = int(sec("rngst", 4, np.uint32)[0])
    ring = sec("ring", 4 * 1248, np.uint32)
    slot = (rngst >> 10) & 1
    assert np.array_equal(ring[624 * slot:624 * slot + 624], rng[:624]) and (rngst & 1023) == int(rng[624]), ("rng", e)
    assert L["rec_bytes"] - L["pad"] < 16 and not r[L["pad"]:].any(), ("padding", e)


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_content(shape):
    """Every section of every record against get_state / get_rng, zero padding, guard bands, index lists."""
    import torch
    mk, n, nd, pokes = SHAPES[shape]
    sim = Sim(mk, n, nd, pokes)
    eng, dev = sim.eng, sim.eng.device
    L = eng.snapshot_layout()
    nb = L["rec_bytes"]
    assert {k: v for k, v in L.items()} == eng.builder.snapshot_layout() and nb % 16 == 0
    sim.warm_up(6)
    pend = sim.pending()
    assert 0 < len(pend) < n, pend
    big, rec = _guarded(torch, dev, n, nb)
    got = eng.snapshot(out=rec)
    big2, rec2 = _guarded(torch, dev, n, nb, 0xA5)
    eng.snapshot(out=rec2)
    torch.cuda.synchronize()
    assert got.data_ptr() == rec.data_ptr() and _guards_hold(big) and _guards_hold(big2, 0xA5)
    assert torch.equal(rec, rec2)  # every byte written, whatever was there
    host = rec.cpu().numpy()
    for e in range(n):
        _check_record(eng, host[e], e)
    flags = host[:, L["scal"] + 20:L["scal"] + 24].copy().view(np.int32).ravel()
    assert [k for k in range(n) if flags[k]] == pend
    if pokes:  # the int32 lives below the int16 floor travel unnarrowed
        hp = host[0, L["obst_hp"]:L["weapon"]].copy().view(np.int32)
        assert min(hp) <= -40000 and eng.obs_dtype == torch.int16, hp
    # an index list in shuffled order with a duplicate: row k is env idx[k]
    idx = list(np.random.default_rng(3).permutation(n)[:min(n, 9)]) + [n - 1, 0, 0]
    big3, rec3 = _guarded(torch, dev, len(idx), nb)
    eng.snapshot(envs=idx, out=rec3)
    torch.cuda.synchronize()
    assert _guards_hold(big3) and torch.equal(rec3, rec[torch.as_tensor(idx, device=dev).long()])
    assert torch.equal(eng.snapshot(envs=torch.tensor(idx[:3], device=dev)), rec3[:3])
    sim.close()


# every shape after 7 steps with eager steps; the fused, the unfused (city128) and the logging handle also after 12
# steps (the other pending-list parity) and with replayed step graphs.  With episodes of five steps and the masked
# reset after step 2, half the envs are pending after steps 6, 12, ... and the other half after steps 7, 13, ...
REWINDS = [(s, 7, False) for s in sorted(SHAPES)] + \
          [(s, b, g) for s in ("bridge64_a2_z10_i64", "city128_a4_z50", "bridge64_death_log")
           for b, g in ((12, False), (7, True), (12, True))]


@pytest.mark.parametrize("shape,before,graph", REWINDS, ids=["%s-%d-%s" % (s, b, "graph" if g else "eager") for s, b, g in REWINDS])
def test_rewind(shape, before, graph):
    """`before` steps, snapshot, 12 more recorded; restore, replay the same 12 action tensors: every output of
    every step bit-identical to the first pass (itself checked against the oracle at every step), the final state
    and stream of every env equal to the first pass's and to the oracle's.  Both pending-list parities (an odd
    and an even number of steps before the snapshot), eager steps and replayed step graphs.  On the handle with
    ZS_FLAG_DEATH_LOG the restored envs' logs are empty until their next step, then the first pass's."""
    import torch
    mk, n, nd, pokes = SHAPES[shape]
    sim = Sim(mk, n, nd, pokes)
    eng = sim.eng
    logs = bool(eng.builder.cfg.flags & _abi.FLAG_DEATH_LOG)
    sim.warm_up(before, graph=graph)
    assert 0 < len(sim.pending()) < n
    lists0 = eng.debug_lists()
    snap = eng.snapshot()
    first, first_logs = [], None
    for _ in range(12):
        first.append(sim.step(graph=graph))
        if logs and first_logs is None:
            first_logs = [(eng.death_log(e), eng.action_log(e)) for e in range(n)]
    sim.check_states()
    final = [sim.state(e) for e in range(n)]
    eng.restore(snap)
    assert eng.debug_lists() == lists0
    if logs:
        assert all(eng.death_log(e) == [] and eng.action_log(e) == ([], False) for e in range(n))
    assert torch.equal(eng.snapshot(), snap)
    t0 = sim.t
    for j, (acts, exp) in enumerate(first):
        _, got = sim.step(acts, graph=graph, follow=False)
        for k in OUT_KEYS:
            a, b = got[k], exp[k]
            if k == "rewards":
                a, b = a.view(np.uint64), b.view(np.uint64)
            assert np.array_equal(a, b), (k, j)
        if logs and j == 0:
            assert [(eng.death_log(e), eng.action_log(e)) for e in range(n)] == first_logs
    assert sim.t == t0 + 12
    for e in range(n):
        st, rng = sim.state(e)
        assert np.array_equal(st, final[e][0]) and np.array_equal(rng, final[e][1]), ("final", e)
    sim.check_states()  # the followers stand where the first pass left them
    sim.close()


def test_fork_across_handles():
    """Records of a 13-env handle into a 21-env handle of the same fingerprint, other lanes per env, unfused."""
    import torch
    mk, _, nd, _ = SHAPES["bridge64_a2_z10_i64"]
    a = Sim(lambda n, **kw: mk(n, lanes_per_env=16 if n > 1 else 0, **kw), 13, nd, seed0=4000)
    b = Sim(lambda n, **kw: mk(n, lanes_per_env=8 if n > 1 else 0, **kw).set_launch({"fused": -1} if n > 1 else None),
            21, nd, seed0=7000)
    assert a.eng.snapshot_layout() == b.eng.snapshot_layout()
    assert a.eng.describe()["lanes_per_env"] == 16 and b.eng.describe()["lanes_per_env"] == 8
    assert b.eng.describe()["step_kernel"] == "k_tick"
    a.warm_up(7)
    b.warm_up(6)
    assert not a.f[3].need and a.f[0].need and a.f[12].need  # a running record and two pending ones ...
    assert b.f[5].need and b.f[7].need and not b.f[0].need and not b.f[20].need  # ... over pending and running envs
    src, dst = [3, 3, 3, 0, 12], [0, 5, 11, 20, 7]
    others = [e for e in range(21) if e not in dst]
    assert len(others) == 16
    before = {e: b.state(e) for e in others}
    rec = a.eng.snapshot()
    b.eng.restore(rec, src=src, dst=dst)
    for e in others:
        st, rng = b.state(e)
        assert np.array_equal(st, before[e][0]) and np.array_equal(rng, before[e][1]), ("untouched env", e)
    for s, d in zip(src, dst):
        sa, sb = a.state(s), b.state(d)
        assert np.array_equal(sa[0], sb[0]) and np.array_equal(sa[1], sb[1]), ("copied env", s, d)
        f = a.f[s].fork()
        f.mk = b.f[d].mk
        b.f[d] = f
    flagged = sorted(b.pending())
    lists = b.eng.debug_lists()
    assert lists[lists[3]] == len(flagged) and lists[1 - lists[3]] == 0 and lists[2] == 0
    for _ in range(9):  # every destination on its own actions, every other env on its own oracle
        b.step()
    b.check_states()
    a.step()  # the source handle is untouched
    a.check_states()
    assert torch.equal(a.eng.snapshot(envs=[1]), a.eng.snapshot()[1:2])
    a.close()
    b.close()


def test_pending_list_and_clone():
    from libzombsole_amd.vector import BatchedZombsole
    mk, n, nd, _ = SHAPES["bridge64_a2_z10_i64"]
    sim = Sim(mk, n, nd)
    eng = sim.eng
    sim.warm_up(6)
    rec0, p0, len0 = eng.snapshot(), sim.pending(), [len(f.log) for f in sim.f]
    sim.step()
    p1 = sim.pending()
    pa = [e for e in p0 if e not in p1][0]      # pending in the record, running now
    pb = [e for e in p1 if e not in p0][0]      # running in the record, pending now
    eng.restore(rec0, src=[pa, pb], dst=[pa, pb])
    for e in (pa, pb):
        sim.f[e] = sim.f[e].fork(len0[e])
    flagged = sorted(set(p1) - {pb} | {pa})
    assert sim.pending() == flagged and pb not in flagged
    c0, c1, resp, par = eng.debug_lists()
    assert (c0, c1)[par] == len(flagged) and (c0, c1)[1 - par] == 0 and resp == 0
    _, got = sim.step()  # check(): was_reset for exactly the followers that were pending
    assert [k for k in range(n) if got["was_reset"][k]] == flagged
    _, got = sim.step()
    assert not any(got["was_reset"][k] for k in flagged)  # each was reset once
    sim.check_states()
    # clone through BatchedZombsole: a 3-cycle, destinations overlapping sources
    venv = BatchedZombsole.__new__(BatchedZombsole)
    venv.engine, venv.torch, venv.num_envs, venv.env0, venv.base_seed = eng, eng.torch, n, 0, 0
    for _ in range(8):  # on to a step that leaves some envs pending and some running
        if 0 < len([e for e in sim.pending() if e != n - 1]) and len(sim.pending()) < n - 1:
            break
        sim.step()
    x = [e for e in sim.pending() if e != n - 1][0]
    y, z = [e for e in range(n - 1) if e not in sim.pending()][0], n - 1
    assert len({x, y, z}) == 3
    pre = {e: sim.state(e) for e in (x, y, z)}
    obs = venv.clone([x, y, z], [y, z, x])
    eng.torch.cuda.synchronize()
    forks = {y: sim.f[x].fork(), z: sim.f[y].fork(), x: sim.f[z].fork()}
    for d, s in ((y, x), (z, y), (x, z)):
        st, rng = sim.state(d)
        assert np.array_equal(st, pre[s][0]) and np.array_equal(rng, pre[s][1]), ("clone", s, d)
        sim.f[d] = forks[d]
        assert np.array_equal(obs[d].cpu().numpy(), sim.f[d].o.obs()), ("clone obs", d)
    lists = eng.debug_lists()
    assert lists[lists[3]] == len(sim.pending()) and lists[1 - lists[3]] == 0
    for _ in range(6):
        sim.step(graph=True)
    sim.check_states()
    sim.close()


def test_checkpoint_through_the_batched_api(tmp_path):
    """save_checkpoint / load_checkpoint on a BatchedZombsole: the loaded run continues bit for bit."""
    import torch

    from libzombsole_amd.vector import BatchedZombsole
    kw = dict(rules_name="extermination", player_names=[], map_name="bridge64", agent_ids=["0", "1"], initial_zombies=10,
              max_episode_steps=5, base_seed=11)
    v = BatchedZombsole("multi", 9, **kw)
    v.reset()
    for t in range(1, 8):
        v.step(v.sample_actions(t), graph=False)
    path = str(tmp_path / "v.ckpt")
    v.save_checkpoint(path)
    outs = []
    for t in range(8, 14):
        o, r, d, tr = v.step(v.sample_actions(t), graph=False)
        outs.append([x.clone() for x in (o, r, d, tr, v.was_reset)])
    obs = v.load_checkpoint(path)
    assert obs.data_ptr() == v.obs.data_ptr()
    for t, exp in zip(range(8, 14), outs):
        o, r, d, tr = v.step(v.sample_actions(t), graph=False)
        torch.cuda.synchronize()
        assert all(torch.equal(g, e) for g, e in zip((o, r, d, tr, v.was_reset), exp)), t
    w = BatchedZombsole("multi", 8, **kw)
    with pytest.raises(ValueError, match="envs"):
        w.load_checkpoint(path)
    u = BatchedZombsole("multi", 9, **dict(kw, initial_zombies=11))
    with pytest.raises(ValueError, match="fingerprint"):
        u.load_checkpoint(path)
    for x in (v, w, u):
        x.close()


def test_refusals_launch_nothing():
    import torch

    from libzombsole_amd.engine import Engine, EngineError, _ptr
    mk, _, nd, _ = SHAPES["bridge64_a2_z10_i64"]
    sim = Sim(mk, 9, nd)
    eng, N = sim.eng, 9
    sim.warm_up(5)
    viewer = Engine(mk(5, viewer=True), device=0)
    rec = eng.snapshot()
    nb, Lb = rec.shape[1], eng.L
    vrec = viewer.snapshot()  # zs_snapshot works on a viewer
    assert vrec.shape == (5, nb)
    assert Lb.zs_restore(viewer.h, _ptr(rec), nb, 9, None, None, 5, None) == _abi.ZS_ESTATE
    assert b"viewer" in Lb.zs_last_error()
    with pytest.raises(EngineError):
        viewer.restore(rec[:5].contiguous())
    before = [sim.state(e) for e in range(N)]
    lists = eng.debug_lists()
    for args in ((nb + 16, 9, 9), (nb - 16, 9, 9), (nb, 9, -1), (nb, -1, 9)):
        assert Lb.zs_restore(eng.h, _ptr(rec), args[0], args[1], None, None, args[2], None) == _abi.ZS_EINVAL, args
    odd = torch.empty(9 * nb + 16, dtype=torch.uint8, device=eng.device)[8:8 + 9 * nb]
    assert odd.data_ptr() % 16 == 8
    assert Lb.zs_restore(eng.h, _ptr(odd), nb, 9, None, None, 9, None) == _abi.ZS_EINVAL
    assert Lb.zs_snapshot(eng.h, None, 9, _ptr(odd), None) == _abi.ZS_EINVAL
    assert Lb.zs_snapshot(eng.h, None, -1, _ptr(rec), None) == _abi.ZS_EINVAL
    with pytest.raises(ValueError, match="repeated"):
        eng.restore(rec, src=[0, 1, 2], dst=[4, 5, 4])
    with pytest.raises(ValueError, match="outside"):
        eng.restore(rec, src=[0, 1], dst=[4, N])
    with pytest.raises(ValueError, match="outside"):
        eng.restore(rec, src=[0, 9], dst=[4, 5])
    with pytest.raises(ValueError):
        eng.restore(rec[:, :nb - 16].contiguous())
    torch.cuda.synchronize()
    assert eng.debug_lists() == lists
    for e in range(N):
        st, rng = sim.state(e)
        assert np.array_equal(st, before[e][0]) and np.array_equal(rng, before[e][1]), ("refused calls wrote", e)
    # check=False: device index tensors holding N and -1 among valid entries; only the valid entries are written
    big, grec = _guarded(torch, eng.device, 9, nb)
    grec.copy_(rec)
    src = torch.tensor([2, 0, 3, 9, -1, 5], dtype=torch.int32, device=eng.device)   # 9, -1: no such record
    dst = torch.tensor([6, N, -1, 1, 4, 8], dtype=torch.int32, device=eng.device)   # N, -1: no such env
    eng.restore(grec, src=src, dst=dst, check=False)
    torch.cuda.synchronize()
    assert _guards_hold(big) and torch.equal(grec, rec)
    for e in range(N):
        want = before[{6: 2, 8: 5}.get(e, e)]
        st, rng = sim.state(e)
        assert np.array_equal(st, want[0]) and np.array_equal(rng, want[1]), ("check=False", e)
    big2, out = _guarded(torch, eng.device, 4, nb)
    idx = torch.tensor([1, N, -1, 7], dtype=torch.int32, device=eng.device)
    Lb.zs_snapshot(eng.h, _ptr(idx), 4, _ptr(out), None)
    torch.cuda.synchronize()
    now = eng.snapshot()
    assert _guards_hold(big2) and torch.equal(out[0], now[1]) and torch.equal(out[3], now[7])
    assert bool((out[1:3] == 0x5A).all())  # skipped entries: nothing written
    # zs_set_state keeps its needs_reset refusal
    e = sim.pending()[0] if sim.pending() else 0
    st = eng.get_state(e)
    st.buf[5] ^= 1
    with pytest.raises(ValueError):
        eng.set_state(e, st)
    viewer.close()
    sim.close()


def test_an_index_beyond_int32_names_nothing():
    """An index that int32 does not hold is no record and no env (engine.as_index turns it into -1): restore refuses
    it under check=True and skips it under check=False, render leaves its frame alone.  It used to wrap into range
    (record 2**32 + 1 was record 1), and render refused every tensor that was not int32."""
    import torch

    from libzombsole_amd.engine import Engine
    mk, n, nd, _ = SHAPES["wall_hp_i16"]  # the smallest map of SHAPES
    seeds = [4000 + 3 * i for i in range(n)]
    eng = Engine(mk(n), device=0)
    eng.seed(seeds)
    eng.reset()
    for t in range(1, 4):
        eng.gen_actions(t, nd)
        eng.step()
    rec = eng.snapshot().clone()
    before = eng.snapshot([0]).clone()
    assert not torch.equal(rec[1], before[0]), "record 1 differs from env 0: a wrapped index would show"
    far = torch.tensor([2 ** 32 + 1], dtype=torch.int64)
    with pytest.raises(ValueError, match="outside"):
        eng.restore(rec, src=far, dst=[0], check=True)
    eng.restore(rec, src=far, dst=[0], check=False)
    torch.cuda.synchronize()
    assert torch.equal(eng.snapshot([0]), before)
    eng.close()
    ren = Engine(mk(n, render=True), device=0)
    ren.seed(seeds)
    ren.reset()
    want = ren.render([0]).clone()
    out = torch.full((2,) + tuple(want.shape[1:]), 0x5A, dtype=torch.uint8, device=ren.device)
    ren.render(envs=torch.tensor([0, 2 ** 32 + 1], dtype=torch.int64), out=out)
    torch.cuda.synchronize()
    assert torch.equal(out[0], want[0]) and bool((out[1] == 0x5A).all())
    ren.close()
