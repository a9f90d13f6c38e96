"""Every C ABI call on a caller's side stream, and the step-graph cache.

The header promises that a call's work goes to the stream it is given.  On the legacy default stream a launch, copy
or memset that went to stream 0 instead still lands in order, and so does a host read that waited for the wrong
stream; a torch side stream is non-blocking, so there it does not.  Every call here is made with a side stream
current, behind a device-side delay that is followed by the writes of the call's inputs (stream_cases.SideExec):
a piece of work that escaped the stream reads the inputs' stale values (well-formed: idle actions, an inverted
mask, another valid index list, another valid snapshot, other legal policy codes and env params) and the results
differ from the oracle's and from a twin engine's that made the same calls on the default stream.  The same event
checks the calls' classes (stream_cases.CALLS): it has not completed when an asynchronous call returns, and has
when a synchronising one does.

Figures of one MI355X run (printed by stream_cases.Delay): host time of a warm eager step 0.040 ms; delay
asked 2.000 ms (the floor: ten times the step is 0.4 ms), measured 2.974 ms.
"""
import numpy as np
import pytest

from libzombsole_amd import _abi
from stream_cases import CALLS, Delay, SideExec, TwinExec

pytestmark = pytest.mark.gpu

MODES = ("eager", "graphed", "policy", "policy3")  # the four ways to step, taken in turn
STEP_OUT = ("obs", "rewards", "done", "trunc", "listed", "was_reset")


def cfg(n, map_name="bridge", minimum=4, limit=5, full=True, launch=None):
    b = _abi.multi_env_config(n, "extermination", [], map_name, ["0", "1"], initial_zombies=10, minimum_zombies=minimum,
                              max_episode_steps=limit, env_params=full, episode_stats=full, render=full)
    return b.set_launch(launch) if launch else b


def policy_table(make, n, seeds, steps, nd=7):
    """[steps + 1][n][A][3]: zs_gen_actions of step numbers 0..steps for envs seeded `seeds` (a function of the seed,
    the step number and the agent alone)."""
    from libzombsole_amd.engine import Engine
    eng = Engine(make(n, full=False))
    eng.seed(seeds)
    out = np.stack([eng.gen_actions(t, nd).cpu().numpy() for t in range(steps + 1)])
    eng.close()
    return out


def delay_engine():
    """The engine whose warm eager step sizes the delay: the first configuration with everything bound."""
    from libzombsole_amd.engine import Engine
    eng = Engine(cfg(37))
    eng.seed(list(range(37)))
    eng.bind_action_masks()
    eng.bind_entity_obs(True, 4, 1)
    eng.nav_bind(True, ("objective", "zombies"), 24)
    eng.bind_autopilot("terminator")
    eng.reset()
    return eng


class In(object):
    """A device input tensor of a checked call with its two values."""

    def __init__(self, real, stale):
        assert real.shape == stale.shape and real.dtype == stale.dtype
        self.real, self.stale, self.t = real, stale, stale.clone()


def put(which, *ins):
    return lambda: [i.t.copy_(getattr(i, which)) for i in ins]


class Rig(object):
    """One engine with every buffer the script passes, allocated and filled on the default stream before the script."""

    def __init__(self, make, n, seeds, acts, grid_obs=True, full=True):
        import torch
        from libzombsole_amd.engine import Engine
        self.torch = t = torch
        self.full, self.n, self.seeds = full, n, list(seeds)
        self.eng = eng = Engine(make(n, full=full), grid_obs=grid_obs)
        dev, A = eng.device, eng.A
        i32 = dict(dtype=t.int32, device=dev)
        self.acts = t.from_numpy(acts).to(dev)  # [T][n][A][3] the caller's actions
        self.idle = t.zeros_like(self.acts[0])
        third = (t.arange(n, device=dev) % 3 == 0).to(t.uint8)
        self.emask = In(third, 1 - third)
        self.idx = In(t.tensor([n - 1, 0, 5, 5], **i32), t.tensor([1, 2, 3, 4], **i32))
        self.perm = In(t.arange(n, **i32).flip(0).contiguous(), t.arange(n, **i32).roll(7).contiguous())
        self.pol = In(t.full((n, A), 1, dtype=t.uint8, device=dev), t.full((n, A), 2, dtype=t.uint8, device=dev))
        c = eng.builder.cfg
        own = t.tensor([c.initial_zombies, c.minimum_zombies, c.max_episode_steps], **i32)
        self.params = In(own.repeat(n, 1), t.tensor([5, 2, 3], **i32).repeat(n, 1))
        over = own.repeat(n, 1)
        over[0, 0] = c.initial_zombies + 1  # a count above the config's cap: refused on the device, flagged
        self.over = In(over, own.repeat(n, 1))
        u8 = dict(dtype=t.uint8, device=dev)
        self.mbuf = t.full((n, A, 8), 0x5A, **u8)
        self.ebuf = t.full((n, A, _abi.entity_layout(3, 1)["row_words"]), 0x5A5A, dtype=t.int16, device=dev)
        self.nbuf = t.full((n, A, 1, 8), 0x5A5A, dtype=t.int16, device=dev)
        W, H = eng.builder.map.size
        self.fbuf = t.zeros((4, H, W), dtype=t.int16, device=dev).view(t.uint16)
        self.pbuf = t.full((n, A, 3), 0x5A, **i32)
        self.gbuf = t.zeros((n, A, 3), **i32)
        self.obuf = t.zeros((n,) + eng.obs_shape, dtype=eng.obs_dtype, device=dev) if grid_obs else None
        L = eng.snapshot_layout()
        self.rec_a, self.rec_b = (t.zeros((n, L["rec_bytes"]), **u8) for _ in range(2))
        self.rec4 = t.zeros((4, L["rec_bytes"]), **u8)
        self.rec_in = In(self.rec_a, self.rec_b)  # the restore's records: the snapshot it restores, and a later one
        self.srec = t.zeros((n, eng.obs_state_layout()["rec_bytes"]), **u8)
        if full:
            R = eng.episode_stats_layout()["R"]
            self.stats = {"run_ret": t.zeros((n, R), dtype=t.float64, device=dev), "last_ret": t.zeros((n, R), dtype=t.float64, device=dev),
                          "sum_ret": t.zeros((n, R), dtype=t.float64, device=dev), "last": t.zeros((n, 8), **i32), "tot": t.zeros((n, 8), **i32)}
            RL = eng.render_layout()
            self.frames = t.full((4, RL["height"], RL["width"], 3), 0x5A, **u8)
            self.pbuf3 = t.zeros((n, 3), **i32)
        self.viewer = Engine(make(n, full=False).viewer(n)) if grid_obs else None  # a viewer carries none of the flags
        t.cuda.synchronize()

    def close(self):
        if self.viewer is not None:
            self.viewer.close()
        self.eng.close()


def read_step(eng):
    d = {k: getattr(eng.out, k).clone() for k in STEP_OUT if getattr(eng.out, k) is not None}
    d["actions"] = eng.actions.clone()
    for k in ("masks", "entities", "nav", "pilot"):
        if getattr(eng, k) is not None:
            d[k] = getattr(eng, k).clone()
    return d


def others(R, X, rec, visit):
    """The calls that leave the envs as they are, each with its inputs written behind the delay."""
    eng, t = R.eng, R.torch
    m, idx = R.emask, R.idx
    a = lambda name, fn, ins=(), read=None: rec.append(  # noqa: E731
        (name, X.call("async", name, fn, put("stale", *ins), put("real", *ins), read or (lambda r: r.clone()))))
    a("zs_action_mask", lambda: eng.action_mask(m.t, out=R.mbuf), (m,))
    a("zs_entity_obs", lambda: eng.entity_obs(m.t, out=R.ebuf, kz=3, kp=1), (m,))
    a("zs_nav_obs", lambda: eng.nav_obs(m.t, out=R.nbuf, fields="zombies", max_dist=20), (m,))
    a("zs_nav_field", lambda: eng.nav_field("objective", envs=idx.t, out=R.fbuf), (idx,), lambda r: r.view(t.int16).clone())
    a("zs_autopilot", lambda: eng.autopilot(R.pol.t, out=R.pbuf), (R.pol,))
    a("zs_gen_actions", lambda: eng.gen_actions(90 + visit, 6, out=R.gbuf))
    a("zs_snapshot", lambda: eng.snapshot(idx.t, out=R.rec4), (idx,))
    a("zs_obs_state_pack", lambda: eng.pack_obs_state(R.srec))
    if R.viewer is not None:
        a("zs_obs_state_unpack", lambda: R.viewer.unpack_obs_state(R.srec), (), lambda r: R.srec.clone())
        a("zs_observe", lambda: R.viewer.observe(m.t, out=R.obuf), (m,))
        a("zs_observe", lambda: eng.observe(m.t, out=R.obuf), (m,))
    if R.full:
        stats = lambda r: {k: v.clone() for k, v in r.items()}  # noqa: E731
        a("zs_episode_stats_get", lambda: eng.episode_stats(m.t, out=R.stats), (m,), stats)
        if visit:
            a("zs_episode_stats_clear", lambda: eng.clear_episode_stats(m.t), (m,), lambda r: None)
            a("zs_episode_stats_get", lambda: eng.episode_stats(out=R.stats), (), stats)
        a("zs_env_params_set", lambda: eng.set_env_params(R.params.t, envs=R.perm.t, check=False), (R.params, R.perm), lambda r: None)
        a("zs_env_params_get", lambda: eng.env_params(out=R.pbuf3))
        a("zs_env_params_get", lambda: eng.env_params(current=True, out=R.pbuf3))
        a("zs_render", lambda: eng.render(idx.t, out=R.frames), (idx,))
    s = lambda name, fn, read=None: rec.append((name, X.call("sync", name, fn, read=read)))  # noqa: E731
    s("zs_get_state", lambda: eng.get_state(3), lambda r: r.buf.copy())
    s("zs_get_rng", lambda: eng.get_rng(2))
    s("zs_overflow", lambda: eng.overflow())
    s("zs_debug_lists", lambda: eng.debug_lists())
    if R.full:  # the logs need ZS_FLAG_DEATH_LOG, which the render flag brings
        s("zs_death_log", lambda: [eng.death_log(e) for e in (0, 1)])
        s("zs_action_log", lambda: [eng.action_log(e) for e in (0, 1)])


def drive(R, X):
    """The script: binds, seed, reset, twelve step calls in the four modes with a masked reset among them (what the
    oracle follows), the state-preserving calls twice in between, then the calls that change an env behind the
    oracle's back (what only the twin follows).  Returns the record: (name, payload) per call, and for the oracle
    ("reset", obs), ("mreset", mask, obs) and ("step", [the action rows each inner step played], outputs)."""
    eng, t = R.eng, R.torch
    rec = []
    sync = lambda name, fn, read=None, **kw: X.call("sync", name, fn, read=read, **kw)  # noqa: E731
    sync("zs_action_mask_bind", lambda: eng.bind_action_masks())
    sync("zs_entity_obs_bind", lambda: eng.bind_entity_obs(True, 4, 1))
    sync("zs_nav_bind", lambda: eng.nav_bind(True, ("objective", "zombies"), 24))
    sync("zs_autopilot_bind", lambda: eng.bind_autopilot(R.pol.real.clone()))  # not into the actions
    sync("zs_seed", lambda: eng.seed(R.seeds))
    obs = lambda r: None if eng.obs is None else eng.obs.clone()  # noqa: E731
    rec.append(("reset", sync("zs_reset", lambda: eng.reset(), obs)))
    step_no, ctr, captured, c_act = 1, None, set(), 0
    for c in range(12):
        mode = MODES[c % 4]
        if c in (5, 10):
            others(R, X, rec, c == 10)
        if c == 6:
            rec.append(("mreset", R.emask.real.cpu().numpy(),
                        sync("zs_reset", lambda: eng.reset(R.emask.t), obs, stale=put("stale", R.emask), real=put("real", R.emask))))
        first = mode not in captured
        captured.add(mode)
        acts = R.acts[c]
        wr = dict(stale=lambda: eng.actions.copy_(R.idle), real=lambda: eng.actions.copy_(acts), read=lambda r: read_step(eng))
        if mode == "eager":
            played, out = [("acts", c)], X.call("async", "zs_step", lambda: eng.step(), **wr)
        elif mode == "graphed":
            played, out = [("acts", c)], X.call("sync" if first else "async", "zs_step_graph", lambda: eng.step_graphed(), **wr)
        else:
            k = 3 if mode == "policy3" else 1
            if first:
                ctr = step_no  # the capture writes the caller's step number; a cached set plays the counter's
            played = [("pol", ctr + j) for j in range(k)]
            ctr += k
            out = X.call("sync" if first else "async", "zs_step_graph_n" if k > 1 else "zs_step_graph",
                         lambda: eng.step_graph(step_no, 7, steps=k), **wr)
        step_no += len(played)
        rec.append(("step", played, out))
    # --- from here the envs leave the oracle's trajectory: the twin alone is the reference
    a = lambda name, fn, ins=(), read=None: rec.append(  # noqa: E731
        (name, X.call("async", name, fn, put("stale", *ins), put("real", *ins), read or (lambda r: None))))
    s = lambda name, fn, read=None, **kw: rec.append((name, sync(name, fn, read, **kw)))  # noqa: E731
    step = lambda k: rec.append(("zs_step", X.call("async", "zs_step", lambda: eng.step(), lambda: eng.actions.copy_(R.idle),  # noqa: E731
                                                    lambda: eng.actions.copy_(R.acts[k]), lambda r: read_step(eng))))
    a("zs_snapshot", lambda: eng.snapshot(out=R.rec_a), (), lambda r: r.clone())
    step(12)
    a("zs_snapshot", lambda: eng.snapshot(out=R.rec_b), (), lambda r: r.clone())
    step(13)
    a("zs_restore", lambda: eng.restore(R.rec_in.t, src=R.perm.t, dst=R.perm.t, check=False), (R.rec_in, R.perm))
    step(14)
    a("zs_restore", lambda: eng.restore(eng.snapshot(R.idx.t, out=R.rec4), dst=R.perm.t[:4], check=False), (R.idx, R.perm))  # a clone
    # a synchronising read right behind an asynchronous call shows that call's results
    s("zs_get_state", lambda: (eng.step(), eng.get_state(3))[1], lambda r: (r.buf.copy(), read_step(eng)),
      stale=lambda: eng.actions.copy_(R.idle), real=lambda: eng.actions.copy_(R.acts[15]))
    view = sync("zs_get_state", lambda: eng.get_state(4))
    view.ent[0][4] = 37  # agent 0's life
    s("zs_set_state", lambda: eng.set_state(4, view))
    s("zs_get_state", lambda: eng.get_state(4), lambda r: r.buf.copy())
    s("zs_set_rng", lambda: eng.set_rng(5, eng.get_rng(6)))
    s("zs_get_rng", lambda: eng.get_rng(5))
    if R.full:
        s("zs_overflow", lambda: (eng.set_env_params(R.over.t, check=False), eng.overflow(clear=True))[1],
          stale=put("stale", R.over), real=put("real", R.over))
        assert rec[-1][1] & _abi.OVF_PARAM_RANGE, rec[-1]  # the flag a delayed call raised
        s("zs_overflow", lambda: eng.overflow())
        s("zs_env_params_check", lambda: eng.set_env_params(R.params.t, check=True), stale=put("stale", R.params), real=put("real", R.params))
    step(16)
    hrec = eng.host_record()
    s("zs_host_step", lambda: eng.host_step(np.zeros((R.n, eng.A, 3), np.int32), None, hrec).copy())
    s("zs_host_observe", lambda: eng.host_observe(hrec).copy())
    s("zs_host_reset", lambda: eng.host_reset(None, hrec).copy())
    step(17)
    step(18)
    s("zs_debug_lists", lambda: eng.debug_lists())
    return rec


def same(a, b, where):
    import torch
    if isinstance(a, dict):
        assert set(a) == set(b), where
        for k in a:
            same(a[k], b[k], where + (k,))
    elif isinstance(a, (tuple, list)):
        assert len(a) == len(b), where
        for k, (x, y) in enumerate(zip(a, b)):
            same(x, y, where + (k,))
    elif torch.is_tensor(a):
        x, y = a.cpu().numpy(), b.cpu().numpy()
        assert x.tobytes() == y.tobytes(), where + ("%d bytes differ" % int((x.view(np.uint8) != y.view(np.uint8)).sum()),)
    elif isinstance(a, np.ndarray):
        assert a.tobytes() == b.tobytes(), where
    else:
        assert a == b, where + (a, b)


def check_oracle(rec, make, n, seeds, tables, grid_obs=True, min_resets=0):
    """The record's resets and steps against one OracleEnv per env driven by the same actions: observations, the
    listed agents' rewards as float64 bytes, done, truncated, listed and was_reset at every call."""
    from oracle.oracle import OracleEnv
    orc = []
    for s in seeds:
        o = OracleEnv(make(1, full=False))
        o.seed(s)
        orc.append(o)
    need = [False] * n
    resets = 0
    for k, e in enumerate(rec):
        if e[0] == "reset":
            exp = np.stack([o.reset() for o in orc])
            if grid_obs:
                assert np.array_equal(e[1].cpu().numpy(), exp), k
            prev = exp
        elif e[0] == "mreset":
            for i, o in enumerate(orc):
                if e[1][i]:
                    prev[i] = o.reset()
                    need[i] = False
            if grid_obs:
                assert np.array_equal(e[2].cpu().numpy(), prev), k  # the other envs' rows untouched
        elif e[0] == "step":
            g = {name: v.cpu().numpy() for name, v in e[2].items()}
            for j, (src, num) in enumerate(e[1]):
                rows = tables[src][num]
                last = j == len(e[1]) - 1
                for i, o in enumerate(orc):
                    if need[i]:
                        ob, need[i] = o.reset(), False
                        resets += 1
                        if last:
                            assert g["was_reset"][i] == 1 and not g["done"][i] and not g["trunc"][i], (k, i)
                    else:
                        ob, rew, d, tr, listed = o.step(rows[i])
                        need[i] = d or tr
                        if last:
                            assert g["was_reset"][i] == 0 and bool(g["done"][i]) == d and bool(g["trunc"][i]) == tr, (k, i)
                            assert np.array_equal(g["listed"][i].astype(bool), listed), (k, i)
                            for a in range(len(listed)):
                                if listed[a]:
                                    assert g["rewards"][i, a].tobytes() == rew[a].tobytes(), (k, i, a)
                    if last:
                        prev[i] = ob
            if src != "acts":  # the policy the graph generated is the table's
                assert np.array_equal(g["actions"], tables[src][num]), k
            if grid_obs:
                assert np.array_equal(g["obs"], prev), k
    assert resets >= min_resets, resets
    return resets


CONFIGS = {
    # name: (config maker, envs, grid_obs, what describe() must show)
    "bridge37": (cfg, 37, True, {}),
    "bridge64_side13": (lambda n, full=True: cfg(n, "bridge64", 6, full=full, launch={"fused": -1, "defer_respawn": 1}), 13, True,
                        {"step_kernel": "k_tick", "respawn": "k_respawn", "reset_side_stream": 1}),
    "bridge37_nogrid": (cfg, 37, False, {"step_tail_launch": "k_tail"}),
}
_shared = {}


def shared(name):
    """Per config, computed once: the actions, the policy table, and the twin's record on the default stream, held to
    the oracle."""
    if name not in _shared:
        make, n, grid, want = CONFIGS[name]
        seeds = [700 + 3 * i for i in range(n)]
        ids = np.random.RandomState(11).randint(0, 7, size=(19, n, 2))
        from libzombsole_amd.actions import DISCRETE_TRIPLES
        acts = np.ascontiguousarray(np.asarray(DISCRETE_TRIPLES, dtype=np.int32)[ids])
        pol = policy_table(make, n, seeds, 40)
        R = Rig(make, n, seeds, acts, grid)
        twin = drive(R, TwinExec())
        R.torch.cuda.synchronize()
        d = R.eng.describe()
        for k, v in want.items():
            assert d[k] == v, (k, d)
        R.close()
        check_oracle(twin, make, n, seeds, {"acts": acts, "pol": pol}, grid, min_resets=2 * n)  # TimeLimit 5 over 18 steps
        _shared[name] = (seeds, acts, pol, twin)
    return _shared[name]


def side_run(name, n_streams):
    make, n, grid, want = CONFIGS[name]
    seeds, acts, pol, twin = shared(name)
    R = Rig(make, n, seeds, acts, grid)
    delay = Delay.get(delay_engine)
    R.torch.cuda.synchronize()
    X = SideExec(R.torch, delay, n_streams)
    rec = drive(R, X)
    X.finish()
    d = R.eng.describe()
    R.close()
    assert not X.wrong, "calls that missed their class (call number, name, class, event completed on return): %s" % X.wrong
    for k, v in want.items():
        assert d[k] == v, (k, d)
    check_oracle(rec, make, n, seeds, {"acts": acts, "pol": pol}, grid, min_resets=2 * n)
    assert len(rec) == len(twin)
    for k, (x, y) in enumerate(zip(rec, twin)):
        assert x[0] == y[0], k
        same(x[1:], y[1:], (k, x[0]))
    return X


@pytest.mark.parametrize("name", list(CONFIGS))
def test_one_side_stream(name):
    """Regime (a): every call on one side stream."""
    X = side_run(name, 1)
    if name == "bridge37":  # every call of the table was made, under its class
        assert set(X.seen) >= set(CALLS), sorted(set(CALLS) - set(X.seen))
        for call, (cls, _) in CALLS.items():
            assert X.seen[call] == ({"sync", "async"} if cls == "first-call-sync" else {cls}), (call, X.seen[call])


@pytest.mark.parametrize("name", list(CONFIGS))
def test_two_side_streams_alternating(name):
    """Regime (b): two side streams, call by call, ordered by the caller's event alone; the handle's shared scratch
    (the state and seed rows, the step counter, the env-params row) survives it."""
    side_run(name, 2)


def test_batched_env_under_a_side_stream(tmp_path):
    """BatchedZombsole with every option on, driven under a side stream for 15 steps against the oracle, with a restore
    from a snapshot taken on that stream and a checkpoint saved and loaded."""
    import torch

    from libzombsole_amd.vector import BatchedZombsole
    n = 37
    seeds, acts, pol, _ = shared("bridge37")
    venv = BatchedZombsole("multi", n, "extermination", [], "bridge", agent_ids=["0", "1"], initial_zombies=10,
                           minimum_zombies=4, max_episode_steps=5, base_seed=900, action_masks=True, env_params=True,
                           episode_stats=True, render=True, entity_obs=(4, 1), autopilot="terminator",
                           nav=("objective", "zombies"))
    delay = Delay.get(delay_engine)
    dacts = torch.from_numpy(acts).to(venv.engine.device)
    torch.cuda.synchronize()
    rec = []
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        rec.append(("reset", venv.reset().clone()))
        for k in range(15):
            venv.actions.zero_()
            delay.queue()
            venv.actions.copy_(dacts[k])
            venv.step(venv.actions)
            rec.append(("step", [("acts", k)], read_step(venv.engine)))
            if k == 6:
                snap = venv.snapshot()
                rec.append(("mark", "snap"))
            if k == 9:
                rec.append(("rewind", "snap", venv.restore(snap).clone()))
            if k == 11:
                venv.save_checkpoint(str(tmp_path / "ck.pt"))
                rec.append(("mark", "ck"))
            if k == 12:
                rec.append(("rewind", "ck", venv.load_checkpoint(str(tmp_path / "ck.pt")).clone()))
    s.synchronize()
    venv.close()
    # the calls in the order the envs lived them: a rewind drops what followed its mark
    lived, marks = [], {}
    for e in rec:
        if e[0] == "mark":
            marks[e[1]] = len(lived)
        elif e[0] == "rewind":
            lived = lived[:marks[e[1]]]
            assert torch.equal(e[2], lived[-1][2]["obs"])  # the restored envs show the observation they showed
        else:
            lived.append(e)
    assert len(lived) == 1 + 15 - 3 - 1
    check_oracle(lived, cfg, n, [900 + i for i in range(n)], {"acts": acts}, min_resets=n)


# ---------------------------------------------------------------------------------------------------------------
# the step-graph cache: four sets, least recently used; the key (seven pointers, n_discrete, n_steps); one step counter
# ---------------------------------------------------------------------------------------------------------------
def c3(n, limit=6):
    return _abi.multi_env_config(n, "extermination", [], "bridge64", ["0", "1"], initial_zombies=10, minimum_zombies=0,
                                 max_episode_steps=limit)


class HashRun(object):
    """A 48-env C3-shaped engine whose every env-step is compared with oracle.run_hashes through StepHasher."""

    N, SEED0 = 48, 4100

    def __init__(self):
        from libzombsole_amd.engine import Engine
        from parity_hash import StepHasher
        self.eng = Engine(c3(self.N))
        self.eng.seed([self.SEED0 + i for i in range(self.N)])
        self.eng.reset()
        self.hs = StepHasher(self.eng)
        self.got = [self.hs.obs_hash().cpu().numpy().view(np.uint64)]

    def took(self, o=None):
        """The hashes of the step just made into output set `o`."""
        eng = self.eng
        o = eng.out if o is None else o
        keep = eng.out
        for k in STEP_OUT:
            setattr(eng, k, getattr(o, k))
        self.got.append(self.hs.step_hash().cpu().numpy().view(np.uint64))
        for k in STEP_OUT:
            setattr(eng, k, getattr(keep, k))

    def check(self, min_resets=0):
        from oracle.oracle import run_hashes
        got = np.stack(self.got, axis=1)
        exp = run_hashes(c3(1), self.SEED0, self.N, got.shape[1] - 1, 7, threads=0)
        bad = np.argwhere(got != exp)
        assert bad.size == 0, "%d of %d env-steps differ; first (env, step): %s" % (len(bad), got.size, bad[:12].tolist())
        self.eng.close()


@pytest.mark.parametrize("sets,nd", [(6, 7), (6, 0), (4, 7)])
def test_graph_cache_eviction(sets, nd):
    """Six output sets round-robin over 24 steps: from the fifth on every call evicts a set and recaptures, and the
    counter is written again from the caller's t; with n_discrete = 0 on caller-written actions; and four sets, each
    replayed from the cache after its capture."""
    H = HashRun()
    outs = [H.eng.outputs() for _ in range(sets)]
    for t in range(1, 25):
        o = outs[(t - 1) % sets]
        if nd == 0:
            H.eng.gen_actions(t, 7)
        H.eng.step_graph(t, nd, out=o)
        H.took(o)
    H.check()


def test_graph_cache_key_change_on_the_same_buffers():
    """n_discrete 7 -> 5 -> 7 and steps 1 -> 2 -> 1 on the same buffers: distinct keys, distinct graphs, every one a
    policy graph, so the counter sees every step and the truthful t is the step played: captures and cached replays
    of each key against oracle envs given the two policies' actions."""
    from libzombsole_amd.engine import Engine
    n = 48
    seeds = [4100 + i for i in range(n)]
    tables = {"pol7": policy_table(lambda m, full=False: c3(m), n, seeds, 20, 7),
              "pol5": policy_table(lambda m, full=False: c3(m), n, seeds, 20, 5)}
    eng = Engine(c3(n))
    eng.seed(seeds)
    rec = [("reset", eng.reset().clone())]
    t = 1
    for nd, steps, calls in ((7, 1, 3), (5, 1, 2), (7, 1, 2), (7, 2, 2), (7, 1, 2), (5, 1, 2), (7, 2, 1)):
        for _ in range(calls):
            eng.step_graph(t, nd, steps=steps)
            rec.append(("step", [("pol%d" % nd, t + j) for j in range(steps)], read_step(eng)))
            t += steps
    eng.torch.cuda.synchronize()
    eng.close()
    assert t == 18
    check_oracle(rec, lambda m, full=False: c3(m), n, seeds, tables, min_resets=2 * n)  # TimeLimit 6 over 17 steps


@pytest.mark.parametrize("between", ["eager", "graphed"])
@pytest.mark.parametrize("evict", [False, True])
def test_graph_step_counter_rule(between, evict):
    """The rule as the header states it: graphed policy steps 1..4, then two steps on gen_actions(5) and (6) that the
    counter does not see (eager zs_step, or n_discrete = 0 graphs, captured right there), then step_graph(7, 7).  On
    the cached set that call plays step number 5's actions; with the set evicted in between it is recaptured and
    plays 7's."""
    from libzombsole_amd.engine import Engine
    n = 48
    seeds = [4100 + i for i in range(n)]
    pol = policy_table(lambda m, full=False: c3(m), n, seeds, 8)
    eng = Engine(c3(n))
    eng.seed(seeds)
    rec = [("reset", eng.reset().clone())]
    for t in range(1, 5):
        eng.step_graph(t, 7)
        rec.append(("step", [("pol", t)], read_step(eng)))
    for t in (5, 6):
        eng.gen_actions(t, 7)
        eng.step() if between == "eager" else eng.step_graphed()
        rec.append(("step", [("acts", t)], read_step(eng)))
    if evict:  # four other keys push the policy set out of the cache (captures run nothing)
        outs = [eng.outputs() for _ in range(4)]
        snap = eng.snapshot()
        for o in outs:
            eng.step_graph(0, 0, out=o)
        eng.restore(snap)  # the envs where they were: the four steps above were made for their captures alone
    eng.step_graph(7, 7)
    rec.append(("step", [("pol", 7 if evict else 5)], read_step(eng)))
    eng.torch.cuda.synchronize()
    eng.close()
    check_oracle(rec, lambda m, full=False: c3(m), n, seeds, {"pol": pol, "acts": pol})


def test_bind_and_unbind_between_replays():
    """zs_action_mask_bind between replays drops the cached graphs: bind, three steps, unbind, three steps, bind
    another buffer, three steps, parity throughout; the first buffer is not written after the unbind."""
    import torch
    H = HashRun()
    eng = H.eng
    first = eng.bind_action_masks()
    t = 1
    for phase in range(3):
        for _ in range(3):
            eng.step_graph(t, 7)
            H.took()
            t += 1
        if phase == 0:
            assert int(first.sum()) > 0
            eng.bind_action_masks(None)
            first.fill_(0x5A)
        if phase == 1:
            second = eng.bind_action_masks()
    torch.cuda.synchronize()
    assert bool((first == 0x5A).all())
    assert eng.masks is second and int(second.sum()) > 0 and second.data_ptr() != first.data_ptr()
    assert torch.equal(second, eng.action_mask(out=torch.zeros_like(second)))
    H.check()


def test_host_read_into_pinned_memory_waits_for_the_stream():
    """zs_get_state through the C ABI into page-locked host memory, where the device-to-host copy itself does not hold
    the host (into pageable memory, which Engine.get_state passes, it does): the call still returns only when the
    stream it was given is done, with the world the delayed step left."""
    import ctypes as C

    import torch
    from libzombsole_amd.engine import Engine
    eng = Engine(cfg(37))
    eng.seed(list(range(37)))
    eng.reset()
    delay = Delay.get(delay_engine)
    pinned = torch.zeros(eng.state_words, dtype=torch.int32).pin_memory()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        delay.queue()
        ev = torch.cuda.Event()
        ev.record(s)
        eng.gen_actions(1, 7)
        eng.step()
        eng._call("zs_get_state", 3, C.c_void_p(pinned.data_ptr()), eng._stream())
        done = ev.query()
        got = pinned.numpy().copy()
    s.synchronize()
    exp = eng.get_state(3).buf
    eng.close()
    assert done
    assert exp[0] == 0 and np.array_equal(got, exp)  # World.t: -1 after the reset (core.py:17), 0 after the first step
