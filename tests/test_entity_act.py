"""k_entity_act_* (csrc/zs_entity_act.hpp) through the C ABI and the Python layers: decode, mask and encode of every
id against libzombsole_amd/entity_act.py on the engine's own state records, on the worlds of entity_obs_cases (E below
64 and E = 132 with 32 agents, K pairs (1, 0), (4, 1), (16, 16), fewer zombies than KZ, equidistant zombies, dead
agents) at 5 and 13 envs; against the same handle's entity observation and action masks, and on a viewer; the effect of
a row id through the action log; the bound decode and the bound masks under every step shape; guard bands and
refusals; and the batched and drop-in layers."""
import ctypes as C

import numpy as np
import pytest

import entity_obs_cases as EC
import golden_util as G
import pilot_census as PC
from libzombsole_amd import _abi
from libzombsole_amd import actions as ACT
from libzombsole_amd import entity_act as EA
from libzombsole_amd import entity_obs as EO

pytestmark = pytest.mark.gpu


def _engine(b, **kw):
    from libzombsole_amd.engine import Engine
    return Engine(b, **kw)


def _row_engine(row, n, launch=None, death_log=False, **over):
    b = EC.builder(row, n, **over)
    if launch:
        b.set_launch(launch)
    if death_log:
        b.cfg.flags |= _abi.FLAG_DEATH_LOG
    eng = _engine(b)
    eng.seed([EC.SEED0 + k for k in range(n)])
    eng.reset()
    return eng


def _model(eng, static, kz, kp, envs=None):
    """(triples [n, A, NID, 3], bits [n, A, RB], ids [n, A, NID]) of the model on the engine's state records: the
    table, its masks, and the encode of every id's own triple."""
    L = EA.layout(kz, kp)
    envs = range(eng.N) if envs is None else envs
    dec = np.zeros((len(envs), eng.A, L["nid"], 3), dtype=np.int32)
    bits = np.zeros((len(envs), eng.A, L["row_bytes"]), dtype=np.uint8)
    enc = np.zeros((len(envs), eng.A, L["nid"]), dtype=np.int32)
    for i, k in enumerate(envs):
        view = eng.get_state(k)
        for a in range(eng.A):
            table = EA.agent_table(view, static, kz, kp, a)
            triples = [tuple(t) for t, _b in table]
            dec[i, a] = triples
            bits[i, a, :L["nid"]] = [b for _t, b in table]
            enc[i, a] = [triples.index(t) for t in triples]
    return dec, bits, enc


def _decode_all(eng, kz, kp):
    import torch
    nid = EA.layout(kz, kp)["nid"]
    ids = torch.zeros((eng.N, eng.A), dtype=torch.int32, device=eng.device)
    out = []
    for j in range(nid):
        ids.fill_(j)
        out.append(eng.entity_act_decode(ids, kz=kz, kp=kp).cpu().numpy())
    return np.stack(out, axis=2)  # [N, A, NID, 3]


def _encode_all(eng, kz, kp, dec):
    import torch
    out = []
    for j in range(dec.shape[2]):
        out.append(eng.entity_act_encode(torch.from_numpy(np.ascontiguousarray(dec[:, :, j])).to(eng.device), kz=kz, kp=kp).cpu().numpy())
    return np.stack(out, axis=2)  # [N, A, NID]


# ---- 1. every id against the model, the entity observation and the action masks -----------------------------------------
@pytest.mark.parametrize("row,n", [(r, (5, 13)[i % 2]) for i, r in enumerate(EC.ROWS)] + [("field9x7", 13), ("fort_e132", 13)])
def test_table_equals_the_model(row, n):
    """After 0, 1 and 12 steps (autoresets included): decode, mask and encode of every id equal the model; the rows'
    triples and bits are the same handle's entity-observation rows and IN_RANGE flags; bytes 0..6 are zs_action_mask's
    (byte 6 by the multi surface's rule); encode after decode is the identity where the triple is the agent's only one."""
    import torch
    eng = _row_engine(row, n)
    static = EO.Static.of_map(eng.builder.map)
    envs = list(range(n)) if row != "fort_e132" else [0, n // 2, n - 1]  # 32 agents x 100 zombies: three envs of the model
    viewer = _engine(EC.builder(row, n, viewer=True))
    t = 0
    for upto in (0, 1, 12):
        while t < upto:
            t += 1
            eng.gen_actions(t, 7)
            eng.step()
        viewer.unpack_obs_state(eng.pack_obs_state())
        for kz, kp in EC.KS:
            L = EA.layout(kz, kp)
            dec, bits, enc = _model(eng, static, kz, kp, envs)
            got_dec = _decode_all(eng, kz, kp)
            got_bits = eng.entity_act_mask(kz=kz, kp=kp).cpu().numpy()
            got_enc = _encode_all(eng, kz, kp, got_dec)
            where = (row, n, t, kz, kp)
            assert np.array_equal(got_dec[envs], dec), (where, np.argwhere(got_dec[envs] != dec)[:5].tolist())
            assert np.array_equal(got_bits[envs], bits), (where, np.argwhere(got_bits[envs] != bits)[:5].tolist())
            assert np.array_equal(got_enc[envs], enc), (where, np.argwhere(got_enc[envs] != enc)[:5].tolist())
            # the entity observation of the same handle
            EL = EO.layout(kz, kp)
            ent = eng.entity_obs(kz=kz, kp=kp).cpu().numpy().astype(np.int32)
            for name, first, K, kind in (("zombies", L["zombie_rows"], kz, ACT.ACT_ATTACK), ("players", L["player_rows"], kp, ACT.ACT_HEAL)):
                rows = ent[:, :, EL[name]:EL[name] + 4 * K].reshape(eng.N, eng.A, K, 4)
                valid = (rows[..., 3] & EO.VALID) != 0
                d = got_dec[:, :, first:first + K]
                assert np.array_equal(d[..., 0], np.where(valid, kind, ACT.ACT_IDLE)), (where, name)
                assert np.array_equal(d[..., 1:], rows[..., :2] * valid[..., None]), (where, name)
                assert np.array_equal(got_bits[:, :, first:first + K], (rows[..., 3] & EO.IN_RANGE) >> 1), (where, name)
            # zs_action_mask, here and on a viewer after zs_obs_state_unpack
            m8 = eng.action_mask(out=torch.zeros((eng.N, eng.A, 8), dtype=torch.uint8, device=eng.device)).cpu().numpy()
            assert np.array_equal(got_bits[:, :, :6], m8[:, :, :6]), where
            if eng.multi:
                assert np.array_equal(got_bits[:, :, 6], m8[:, :, 6]), where
            assert torch.equal(viewer.entity_act_mask(kz=kz, kp=kp), torch.from_numpy(got_bits).to(eng.device)), where
            v8 = viewer.action_mask().cpu().numpy()
            assert np.array_equal(got_bits[:, :, :6], v8[:, :, :6]), where
            assert np.array_equal(_decode_all(viewer, kz, kp), got_dec), where
            # encode after decode: the identity on valid ids whose triple the agent's table holds once
            for k in range(eng.N):
                for a in range(eng.A):
                    tr = [tuple(x) for x in got_dec[k, a].tolist()]
                    for j, x in enumerate(tr):
                        if x != (0, 0, 0) and tr.count(x) == 1:
                            assert got_enc[k, a, j] == j, (where, k, a, j)
    assert not eng.overflow() & _abi.OVF_PARAM_RANGE
    viewer.close()
    eng.close()


def test_the_worlds_hold_the_shapes():
    """What the rows were taken for, by the engines' own records: fewer zombies than KZ, equidistant zombies, dead agents,
    an agent at the map's edge, E below 64 and E = 132 with 32 agents."""
    seen = set()
    for row in ("wall5x4", "crowd9x7", "fort_e132", "strip1x70"):
        eng = _row_engine(row, 5)
        static = EO.Static.of_map(eng.builder.map)
        seen |= {"E%d_A%d" % (eng.E, eng.A)}
        for t in range(1, 13):
            eng.gen_actions(t, 7)
            eng.step()
        for k in range(5):
            v = eng.get_state(k)
            zs = [e for e in v.ent[eng.A + int(v.P):] if e[1]]
            for a in range(eng.A):
                if not v.ent[a][1]:
                    seen.add("dead_agent")
                    continue
                d = sorted((int(e[2]) - int(v.ent[a][2])) ** 2 + (int(e[3]) - int(v.ent[a][3])) ** 2 for e in zs)
                seen |= {"tie"} if any(x == y for x, y in zip(d, d[1:])) else set()
                seen |= {"short"} if len(d) < 4 else set()
                seen |= {"edge"} if int(v.ent[a][2]) in (0, static.W - 1) or int(v.ent[a][3]) in (0, static.H - 1) else set()
        eng.close()
    assert {"dead_agent", "tie", "short", "edge", "E132_A32"} <= seen and any(s.startswith("E") and int(s[1:].split("_")[0]) < 64 for s in seen), seen


@pytest.mark.parametrize("name", PC.pilot_fixture_names())
def test_every_terminator_triple_has_an_id(name):
    """The engine driven through a pilot fixture's calls: the encode of k_autopilot's terminator rows is never -1, and
    decodes back to the row."""
    import torch
    fx = G.load_fixture(name)
    runs = fx["runs"]
    pokes = (fx.get("extras") or {}).get("poke_things", [])
    eng = _engine(G.builder_for(fx, num_envs=len(runs)))
    eng.seed([r["seed"] for r in runs])
    for k in range(len(runs) if G.obstacle_pokes(fx) else 0):
        st = eng.get_state(k)
        for i, life in G.obstacle_pokes(fx):
            st.obst_life[i] = life
        eng.set_state(k, st)
    eng.reset()
    kinds = set()
    for i in range(len(runs[0]["calls"])):
        if any(p[1] == i for p in pokes):
            break  # the poke puts a thing outside the map, from where the engine is not stepped
        if i > 0:
            acts = np.stack([G.action_triples(fx, r["calls"][i], eng.A)[:eng.A] if r["calls"][i]["kind"] == "step"
                             else np.zeros((eng.A, 3), np.int32) for r in runs])
            eng.actions.copy_(torch.from_numpy(acts))
            eng.step()
        rows = eng.autopilot("terminator")
        ids = eng.entity_act_encode(rows, kz=4, kp=1)
        assert int(ids.min()) >= 0, (name, i, rows.cpu().tolist(), ids.cpu().tolist())
        assert torch.equal(eng.entity_act_decode(ids, kz=4, kp=1), rows), (name, i)
        kinds |= set(rows[..., 0].flatten().tolist())
    assert kinds & {ACT.ACT_MOVE, ACT.ACT_ATTACK_CLOSEST, ACT.ACT_HEAL} or any(p[1] == 0 for p in pokes)  # poked at its first call
    eng.close()


# ---- 2. the effect, through the action log -------------------------------------------------------------------------------
def test_a_row_id_attacks_the_rows_zombie():
    """Stepping with id 15 + j: where the row's mask bit is 1 the tick logs an attack of the agent whose target is the
    slot of entity row j (the j-th present zombie by (d2, slot)).  A valid row that is masked out lands no attack: the
    action log holds decisions, so the agent's entry is the attempt at that slot, which the reference reports as 'too
    far'; where the zombie cannot walk into range within the tick (one cell) and nobody else aims at it, its life is
    what it was.  An id past the present zombies is idle: no entry."""
    import torch
    n, kz, kp = 13, 16, 1
    eng = _row_engine("bridge_a4", n, death_log=True)  # knife, axe, gun, shotgun: rows in and out of range
    for t in range(1, 4):
        eng.gen_actions(t, 7)
        eng.step()
    hit = missed = 0
    for j in (0, 1, 5):
        views = [eng.get_state(k) for k in range(n)]
        bits = eng.entity_act_mask(kz=kz, kp=kp).cpu().numpy()
        ids = torch.full((n, eng.A), 15 + j, dtype=torch.int32, device=eng.device)
        acts = eng.entity_act_decode(ids, kz=kz, kp=kp)
        eng.step(acts)
        for k in range(n):
            v = views[k]
            if int(eng.was_reset[k]):
                continue
            log, raised = eng.action_log(k)
            after = eng.get_state(k)
            assert not raised
            for a in range(eng.A):
                if not v.ent[a][1]:
                    continue
                ax, ay = int(v.ent[a][2]), int(v.ent[a][3])
                order = sorted(((int(v.ent[s][2]) - ax) ** 2 + (int(v.ent[s][3]) - ay) ** 2, s)
                               for s in range(eng.A + int(v.P), eng.E) if v.ent[s][1])
                mine = [(kind, tgt) for slot, kind, tgt in log if slot == a]
                if j >= len(order):
                    assert mine == [] and acts[k, a].tolist() == [0, 0, 0]
                elif bits[k, a, 15 + j]:
                    assert mine == [(2, order[j][1])], (j, k, a, mine, order[j])
                    hit += 1
                else:
                    d2, slot = order[j]
                    assert mine == [(2, slot)], (j, k, a, mine, order[j])
                    r2 = EO.weapon_r2(v.ent[a][5])
                    others = [s for s, kind, tgt in log if kind == 2 and tgt == slot and s != a]
                    if (d2 ** 0.5 - 1) ** 2 > r2 and not others:
                        assert after.ent[slot][1] and int(after.ent[slot][4]) == int(v.ent[slot][4]), (j, k, a, slot)
                        missed += 1
    assert hit >= 10 and missed >= 10, (hit, missed)
    eng.close()


# ---- 3. the bound decode and the bound masks under every step shape --------------------------------------------------------
def _ids_for(eng, nid, t):
    """A deterministic id per agent and step over the whole table."""
    import torch
    k = torch.arange(eng.N * eng.A, dtype=torch.int64, device=eng.device).view(eng.N, eng.A)
    return ((k * 7 + t * 13 + (k * t) % 5) % nid).to(torch.int32)


def _same(a, b, where):
    import torch
    for name in ("rewards", "done", "trunc", "listed", "was_reset"):
        assert torch.equal(getattr(a, name), getattr(b, name)), (where, name)
    assert torch.equal(a.snapshot(), b.snapshot()), where  # every env's whole state, its MT19937 ring included


BOUND_SHAPES = [(mode, lanes, fused, "default") for mode in ("eager", "graph", "graph4") for lanes in (1, 16, 64) for fused in (1, -1)] + \
               [(mode, 16, -1, "side") for mode in ("eager", "graph", "graph4")]  # a caller's side stream, with the reset work's fork


@pytest.mark.parametrize("mode,lanes,fused,stream", BOUND_SHAPES)
def test_bound_decode_is_decode_then_step(mode, lanes, fused, stream):
    """ids bound: the step (eager, one graph launch, four steps per graph launch) equals a twin's standalone decode into
    its action buffer followed by zs_step, the twin re-decoding before each of the four steps; rewards, flags, the
    snapshot records (state and RNG) and the bound masks after every launch."""
    import torch
    row, n, kz, kp = "field9x7", 13, 4, 1
    launch = {"fused": fused, "fobs": -1}
    eng = _row_engine(row, n, launch=launch, lanes_per_env=lanes)
    twin = _row_engine(row, n, launch=launch, lanes_per_env=lanes)
    d = eng.describe()
    assert d["lanes_per_env"] == lanes and d["step_kernel"] == ("k_step" if fused > 0 else "k_tick"), d
    assert (d["entity_act_ids_bound"], d["entity_act_mask_bound"], d["entity_act_kernel"]) == (0, 0, "k_entity_act")
    nid = EA.layout(kz, kp)["nid"]
    ids, masks = eng.bind_entity_act(True, True, kz, kp)
    d = eng.describe()
    assert (d["entity_act_ids_bound"], d["entity_act_mask_bound"]) == (1, 1)
    per = 4 if mode == "graph4" else 1
    side = torch.cuda.Stream(device=eng.device) if stream == "side" else None
    resets = 0
    for t in range(per, 25, per):
        want = _ids_for(eng, nid, t)
        if side is not None:
            side.wait_stream(torch.cuda.current_stream(eng.device))
        with torch.cuda.stream(side) if side is not None else torch.cuda.stream(torch.cuda.current_stream(eng.device)):
            ids.copy_(want)
            eng.actions.fill_(-7)  # the decode overwrites every row
            if mode == "eager":
                eng.step()
            else:
                eng.step_graph(0, 0, steps=per)
        if side is not None:
            torch.cuda.current_stream(eng.device).wait_stream(side)
        for _ in range(per):
            twin.entity_act_decode(want, out=twin.actions, kz=kz, kp=kp)
            twin.step()
        _same(eng, twin, (mode, lanes, fused, stream, t))
        assert torch.equal(eng.actions, twin.actions), (mode, lanes, fused, stream, t)
        assert torch.equal(masks, twin.entity_act_mask(kz=kz, kp=kp)), (mode, lanes, fused, stream, t)
        resets += int(eng.was_reset.sum())
    assert resets >= 3
    eng.close()
    twin.close()


def test_bound_masks_rebinding_and_an_unbound_handle():
    """The bound masks equal a standalone call after each step; other buffers or K values recapture; unbinding stops the
    launches; a handle that never binds reports the same tail launch and outputs as before."""
    import torch
    row, n = "bridge64", 13
    eng, plain = _row_engine(row, n), _row_engine(row, n)
    ids, first = eng.bind_entity_act(None, True, 4, 1)
    assert ids is None and eng.describe()["entity_act_ids_bound"] == 0
    for t in range(1, 5):
        eng.step_graph(t, 7)  # a generated policy is fine while no ids are bound
        plain.step_graph(t, 7)
        assert torch.equal(first, eng.entity_act_mask(out=torch.zeros_like(first)))
    _same(eng, plain, "masks bound")
    assert eng.describe()["step_tail_launch"] == plain.describe()["step_tail_launch"] != ""
    kept = first.clone()
    _ids, second = eng.bind_entity_act(None, True, 16, 16)
    for t in range(5, 9):
        eng.step_graph(t, 7)
        plain.step_graph(t, 7)
    assert torch.equal(first, kept) and second.shape == (n, 2, 48)
    assert torch.equal(second, eng.entity_act_mask(out=torch.zeros_like(second)))
    assert not second[:, :, 47:].any()
    eng.bind_entity_act(None, None)
    d = eng.describe()
    assert eng.entity_act_masks is None and (d["entity_act_ids_bound"], d["entity_act_mask_bound"]) == (0, 0)
    kept = second.clone()
    for t in range(9, 13):
        eng.step_graph(t, 7)
        plain.step_graph(t, 7)
    assert torch.equal(second, kept)
    _same(eng, plain, "unbound")
    pd = plain.describe()
    assert (pd["entity_act_ids_bound"], pd["entity_act_mask_bound"]) == (0, 0) and pd == eng.describe()
    eng.close()
    plain.close()


def test_the_standalone_calls_are_asynchronous_on_a_side_stream():
    """stream_cases' side-stream check (SideExec behind a device-side Delay) for decode, mask and encode: each returns
    before the delay queued ahead of it on the side stream has completed, reads its inputs behind that delay (stale values
    ahead of it, the real ones after), and gives what the default stream gives."""
    import torch
    from stream_cases import Delay, SideExec

    def delay_engine():
        e = _row_engine("bridge64", 37)
        e.bind_entity_obs(True, 4, 1)
        return e

    eng = _row_engine("crowd9x7", 13)
    for t in range(1, 6):
        eng.gen_actions(t, 7)
        eng.step()
    kz, kp, n, A = 4, 1, 13, eng.A
    real = _ids_for(eng, 20, 2)
    stale = _ids_for(eng, 20, 5)
    env_real = (torch.arange(n, device=eng.device) % 3 != 0).to(torch.uint8)
    want_mask = eng.entity_act_mask(env_real, out=torch.full((n, A, 24), 0x5A, dtype=torch.uint8, device=eng.device), kz=kz, kp=kp).clone()
    want_dec = eng.entity_act_decode(real, env_real, out=torch.full((n, A, 3), 0x5A, dtype=torch.int32, device=eng.device), kz=kz, kp=kp).clone()
    want_enc = eng.entity_act_encode(want_dec, env_real, out=torch.full((n, A), 0x5A, dtype=torch.int32, device=eng.device), kz=kz, kp=kp).clone()
    ids, em = stale.clone(), (1 - env_real).clone()
    mbuf = torch.full((n, A, 24), 0x5A, dtype=torch.uint8, device=eng.device)
    dbuf = torch.full((n, A, 3), 0x5A, dtype=torch.int32, device=eng.device)
    ebuf = torch.full((n, A), 0x5A, dtype=torch.int32, device=eng.device)
    tri = torch.zeros_like(want_dec)
    torch.cuda.synchronize()
    X = SideExec(torch, Delay.get(delay_engine))
    put_stale = lambda: (ids.copy_(stale), em.copy_(1 - env_real), tri.zero_())  # noqa: E731
    put_real = lambda: (ids.copy_(real), em.copy_(env_real), tri.copy_(want_dec))  # noqa: E731
    got_mask = X.call("async", "zs_entity_act_mask", lambda: eng.entity_act_mask(em, out=mbuf, kz=kz, kp=kp), put_stale, put_real, lambda r: r.clone())
    got_dec = X.call("async", "zs_entity_act_decode", lambda: eng.entity_act_decode(ids, em, out=dbuf, kz=kz, kp=kp), put_stale, put_real, lambda r: r.clone())
    got_enc = X.call("async", "zs_entity_act_encode", lambda: eng.entity_act_encode(tri, em, out=ebuf, kz=kz, kp=kp), put_stale, put_real, lambda r: r.clone())
    X.finish()
    assert not X.wrong, X.wrong
    assert torch.equal(got_mask, want_mask) and torch.equal(got_dec, want_dec) and torch.equal(got_enc, want_enc)
    eng.close()


def test_host_step_decodes_and_masks():
    """zs_host_step is zs_step: bound ids are decoded into the per-call path's action rows, bound masks follow."""
    import torch
    eng = _row_engine("wall5x4", 1)
    ids, masks = eng.bind_entity_act(True, True, 4, 1)
    ids.fill_(5)
    before = eng.get_state(0)
    rec = eng.host_record()
    eng.host_step(np.zeros((1, eng.A, 3), dtype=np.int32), None, rec)  # idle rows, overwritten by the decode of `heal`
    assert torch.equal(masks, eng.entity_act_mask(out=torch.zeros_like(masks))) and int(masks[0, 0, 5]) == 1
    assert eng.get_state(0).ent[0][4] >= before.ent[0][4]
    eng.close()


# ---- 4. masked calls, guard bands, an id outside the table, refusals ------------------------------------------------------------
@pytest.mark.parametrize("kz,kp", EC.KS)
def test_guard_bands_and_masked_calls(kz, kp):
    """Each buffer inside a 0x5A-filled byte tensor: nothing before or after it is written, an env whose env-mask byte
    is 0 keeps its bytes, the mask row's padding is zero."""
    import torch
    row, n = "crowd9x7", 13
    eng = _row_engine(row, n)
    for t in range(1, 9):
        eng.gen_actions(t, 7)
        eng.step()
    L = EA.layout(kz, kp)
    nid, rb = L["nid"], L["row_bytes"]
    ids = _ids_for(eng, nid, 3)
    want = {"mask": eng.entity_act_mask(kz=kz, kp=kp).cpu().numpy(),
            "decode": eng.entity_act_decode(ids, kz=kz, kp=kp).cpu().numpy()}
    want["encode"] = eng.entity_act_encode(torch.from_numpy(want["decode"]).to(eng.device), kz=kz, kp=kp).cpu().numpy()
    assert not want["mask"][:, :, nid:].any()
    shapes = {"mask": ((n, eng.A, rb), torch.uint8), "decode": ((n, eng.A, 3), torch.int32), "encode": ((n, eng.A), torch.int32)}
    triples = torch.from_numpy(want["decode"]).to(eng.device)
    for what, (shape, dt) in shapes.items():
        nb = int(np.prod(shape)) * (1 if dt == torch.uint8 else 4)
        raw = torch.full((nb + 256,), 0x5A, dtype=torch.uint8, device=eng.device)
        lo = (-raw.data_ptr()) % 16 + 64 + (8 if what == "mask" else 4)
        view = raw[lo:lo + nb].view(dt).view(*shape)
        for m in (torch.zeros(n), torch.ones(n), torch.arange(n) % 2, (torch.arange(n) == n - 1)):
            raw.fill_(0x5A)
            mk = m.to(torch.uint8).to(eng.device)
            if what == "mask":
                eng.entity_act_mask(mk, out=view, kz=kz, kp=kp)
            elif what == "decode":
                eng.entity_act_decode(ids, mk, out=view, kz=kz, kp=kp)
            else:
                eng.entity_act_encode(triples, mk, out=view, kz=kz, kp=kp)
            got = raw.cpu().numpy()
            assert (got[:lo] == 0x5A).all() and (got[lo + nb:] == 0x5A).all(), (what, kz, kp)
            body = got[lo:lo + nb].view(want[what].dtype).reshape(shape)
            on = m.numpy().astype(bool)
            assert np.array_equal(body[on], want[what][on]), (what, kz, kp)
            assert (body[~on].view(np.uint8) == 0x5A).all(), (what, kz, kp)
    eng.close()


def test_an_id_outside_the_table_idles_and_raises_the_flag():
    import torch
    eng = _row_engine("bridge64", 5)
    nid = EA.layout(4, 1)["nid"]
    ids = torch.full((5, eng.A), 4, dtype=torch.int32, device=eng.device)
    assert eng.entity_act_decode(ids, kz=4, kp=1)[..., 0].eq(ACT.ACT_ATTACK_CLOSEST).all()
    assert not eng.overflow() & _abi.OVF_PARAM_RANGE
    for bad in (nid, -1, 2 ** 31 - 1, -2 ** 31):
        ids.fill_(4)
        ids[3, 1] = bad
        out = eng.entity_act_decode(ids, kz=4, kp=1).cpu().numpy()
        assert out[3, 1].tolist() == [0, 0, 0] and (np.delete(out.reshape(-1, 3), 3 * eng.A + 1, axis=0)[:, 0] == ACT.ACT_ATTACK_CLOSEST).all()
        assert eng.overflow(clear=True) & _abi.OVF_PARAM_RANGE, bad
    ids.fill_(nid - 1)  # the last id of the table is inside it
    eng.entity_act_decode(ids, kz=4, kp=1)
    assert not eng.overflow() & _abi.OVF_PARAM_RANGE
    eng.close()


def test_refusals():
    """Before any launch: bad K values, misaligned buffers, null pointers, a bind on a viewer, a generated policy while
    ids are bound."""
    import torch
    eng = _row_engine("wall5x4", 5)
    L, s = eng.L, eng._stream()
    ids = torch.zeros((5, eng.A), dtype=torch.int32, device=eng.device)
    acts = torch.zeros((5, eng.A, 3), dtype=torch.int32, device=eng.device)
    mk = torch.full((5 * eng.A * 24 + 16,), 0x5A, dtype=torch.uint8, device=eng.device)
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)  # noqa: E731
    for kz, kp in ((0, 0), (17, 1), (4, -1), (4, 17)):
        assert L.zs_entity_act_table(eng.h, kz, kp, (C.c_int32 * 8)()) == _abi.ZS_EINVAL
        assert L.zs_entity_act_decode(eng.h, None, kz, kp, p(ids), p(acts), s) == _abi.ZS_EINVAL
        assert L.zs_entity_act_mask(eng.h, None, kz, kp, p(mk), s) == _abi.ZS_EINVAL
        assert L.zs_entity_act_encode(eng.h, None, kz, kp, p(acts), p(ids), s) == _abi.ZS_EINVAL
        assert L.zs_entity_act_bind(eng.h, p(ids), p(mk), kz, kp) == _abi.ZS_EINVAL
        with pytest.raises(ValueError):
            eng.entity_act_mask(kz=kz, kp=kp)
    for off in (1, 2, 4, 7):
        assert L.zs_entity_act_mask(eng.h, None, 4, 1, p(mk, off), s) == _abi.ZS_EINVAL
        assert L.zs_entity_act_bind(eng.h, None, p(mk, off), 4, 1) == _abi.ZS_EINVAL
    assert L.zs_entity_act_mask(eng.h, None, 4, 1, None, s) == _abi.ZS_EINVAL
    assert L.zs_entity_act_decode(eng.h, None, 4, 1, None, p(acts), s) == _abi.ZS_EINVAL
    assert L.zs_entity_act_encode(eng.h, None, 4, 1, p(acts), None, s) == _abi.ZS_EINVAL
    torch.cuda.synchronize()
    assert (mk == 0x5A).all() and not acts.any() and not ids.any()  # nothing was launched
    d = eng.describe()
    assert (d["entity_act_ids_bound"], d["entity_act_mask_bound"]) == (0, 0)
    assert eng.entity_act_layout(4, 1) == dict(EA.layout(4, 1), kz=4, kp=1)
    out = (C.c_int32 * 8)()
    assert L.zs_entity_act_table(eng.h, 16, 16, out) == 0 and list(out) == [47, 48, 7, 11, 15, 31, 47, 0]
    # a generated policy would overwrite the decoded rows
    eng.bind_entity_act(True, None, 4, 1)
    with pytest.raises(ValueError, match="n_discrete"):
        eng.step_graph(1, 7)
    with pytest.raises(ValueError, match="n_discrete"):
        eng.step_graph(1, 7, steps=4)
    eng.step_graph(0, 0)
    eng.bind_entity_act(None, None)
    eng.step_graph(1, 7)
    viewer = _engine(EC.builder("wall5x4", 5, viewer=True))
    assert L.zs_entity_act_bind(viewer.h, p(ids), None, 4, 1) == _abi.ZS_ESTATE
    with pytest.raises(RuntimeError):
        viewer.bind_entity_act(True, True, 4, 1)
    viewer.close()
    eng.close()


# ---- 5. the Python layers ---------------------------------------------------------------------------------------------------
def test_batched_entity_actions(tmp_path):
    """BatchedZombsole(entity_actions=True): step(ids) equals the eager path on a twin; the mask tensor is current after
    reset, a masked reset, steps, restore, clone and load_checkpoint; encode_actions labels the terminator's triples."""
    import torch
    from libzombsole_amd.vector import BatchedZombsole
    n = 13
    kw = dict(agent_ids=["0", "1"], initial_zombies=10, minimum_zombies=4, max_episode_steps=9, base_seed=3, entity_obs=(4, 1),
              autopilot="terminator")
    venv = BatchedZombsole("multi", n, "extermination", [], "bridge", entity_actions=True, **kw)
    twin = BatchedZombsole("multi", n, "extermination", [], "bridge", **kw)
    eng = venv.engine
    static = EO.Static.of_map(eng.builder.map)
    assert venv.n_entity_actions == 20 and twin.n_entity_actions is None and twin.entity_action_masks is None

    def check():
        got = venv.entity_action_masks.cpu().numpy()
        want = np.stack([EA.mask(eng.get_state(k), static, 4, 1)[:, :20] for k in range(n)])
        assert got.shape == (n, 2, 20) and np.array_equal(got, want)
        return got

    venv.reset()
    twin.reset()
    check()
    for t in range(1, 13):
        ids = _ids_for(eng, 20, t)
        if t % 4 == 0:  # the teacher's labels: stepping with them is stepping with its triples
            ids = venv.encode_actions()
            assert int(ids.min()) >= 0 and torch.equal(eng.entity_act_decode(ids), venv.scripted_actions)
        if t % 5 == 0:  # an [N, A, 3] tensor is still taken as triples
            acts = twin.engine.entity_act_decode(ids, kz=4, kp=1)
            venv.step(acts.clone(), graph=bool(t % 2))
        else:
            acts = twin.engine.entity_act_decode(ids, kz=4, kp=1)
            venv.step(ids, graph=bool(t % 2))
        twin.step(acts, graph=False)
        _same(eng, twin.engine, ("batched", t))
        check()
    snap = venv.snapshot()
    ck = str(tmp_path / "ck.pt")
    venv.save_checkpoint(ck)
    at_snap = check()
    for t in range(13, 17):
        venv.step(_ids_for(eng, 20, t))
    venv.restore(snap, src=[0, 1], dst=[4, 5])
    check()
    venv.clone([0], [7], observe=False)
    check()
    venv.load_checkpoint(ck)
    assert np.array_equal(check(), at_snap)
    m = torch.zeros(n, dtype=torch.uint8, device=eng.device)
    m[3] = 1
    venv.reset(m)
    check()
    venv.close()
    twin.close()
    with pytest.raises(ValueError):
        BatchedZombsole("multi", 2, "extermination", [], "bridge", agent_ids=["0", "1"], initial_zombies=3, entity_actions=True)


def test_dropin_helpers():
    """The drop-in envs' entity_action_masks() and entity_action() agree with a one-env batched handle seeded alike."""
    import random

    from libzombsole_amd.gym.multiagent_env import MultiagentZombsoleEnv
    from libzombsole_amd.gym_env import ZombsoleGymEnv
    env = MultiagentZombsoleEnv("extermination", [], "bridge", ["0", "1"], initial_zombies=10, device=0)
    random.seed(11)
    env.reset()
    eng = env._core.engine
    static = EO.Static.of_map(eng.builder.map)
    for t in range(4):
        view = eng.get_state(0)
        want = EA.mask(view, static, 4, 1)[:, :20]
        assert np.array_equal(env.entity_action_masks(), want)
        acts = {}
        for a, aid in enumerate(["0", "1"]):
            j = 15 + (t + a) % 5
            d = env.entity_action(aid, j)
            triple = EA.agent_table(view, static, 4, 1, a)[j][0]
            assert d == {"action_type": {0: None, 2: "attack", 4: "heal"}[triple[0]], "parameter": [triple[1], triple[2]]}
            acts[aid] = d if d["action_type"] else {"action_type": "heal", "parameter": [0, 0]}
        env.step(acts)
    env.close()
    single = ZombsoleGymEnv("extermination", [], "bridge", 0, initial_zombies=5, device=0)
    random.seed(5)
    single.reset()
    view = single.engine.get_state(0)
    assert np.array_equal(single.entity_action_masks(), EA.mask(view, static, 4, 1)[0, :20])
    assert single.entity_action(0, 4) == {"action_type": "attack_closest", "parameter": [0, 0]}
    assert single.entity_action(0, 15)["action_type"] == "attack"
    single.close()
