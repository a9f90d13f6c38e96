"""Observation-state records on one MI355X: pack -> unpack into a viewer handle -> re-encode, bit-identical.

For every shape two source handles with different seeds ("rank 0", "rank 1", m envs each) are reset and stepped
24 steps under the bench policy with max_episode_steps = 5, so autoresets land inside the run.  After the reset
and after steps 1, 2, 7 and 24 their records (zs_obs_state_pack) are unpacked at env0 = 0 and env0 = m into one
viewer handle of 2 m + 3 envs, whose last 3 envs are never written, and the viewer's zs_observe (its own planned
kernel, unmasked and masked) must reproduce the sources' observations bit for bit.  The records' contents are
checked against zs_get_state through the layout's offsets, the pack's writes against guard bands, and the
host-side refusals against their codes.
"""
import ctypes as C
import os

import numpy as np
import pytest

from libzombsole_amd import _abi
from libzombsole_amd.maps import Map

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
I32, I64, I16 = _abi.DTYPE_I32, _abi.DTYPE_I64, _abi.DTYPE_I16
CHECK_AT = (0, 1, 2, 7, 24)
STEPS = 24


def _wall_hp_map():
    with open(os.path.join(HERE, "golden", "maps", "wall_hp.txt")) as f:
        return Map.from_text(f.read(), name="wall_hp")


def _wall_hp(dtype, style="channels"):
    def mk(n, **kw):
        return _abi.multi_env_config(n, "extermination", [], _wall_hp_map(), ["0", "1"], initial_zombies=0,
                                     minimum_zombies=0, observation_position_encoding_style=style,
                                     max_episode_steps=5, obs_dtype=dtype, **kw)
    return mk


def _bridge64(agents, zombies, dtype):
    def mk(n, **kw):
        return _abi.multi_env_config(n, "extermination", [], "bridge64", [str(a) for a in range(agents)],
                                     initial_zombies=zombies, minimum_zombies=0, max_episode_steps=5,
                                     obs_dtype=dtype, **kw)
    return mk


def _bridge_single(n, **kw):  # E = 7: the u8 rows of env e start at byte 7 e
    return _abi.single_env_config(n, "extermination", ["terminator", "sniper"], "bridge", 0, initial_zombies=4,
                                  observation_scope="world", max_episode_steps=5, obs_dtype=I32, **kw)


def _city128(n, **kw):  # the long sections: 512 dead-body words, > 100 obstacle-presence words
    return _abi.multi_env_config(n, "safehouse", [], "city128", ["0", "1", "2", "3"], initial_zombies=50,
                                 minimum_zombies=50, max_episode_steps=5, obs_dtype=I64, **kw)


def _poke_wall_hp(eng):
    """Walls at -32 700 ... -40 000 (either side of the int16 floor), dead bodies under obstacles and on a free
    cell, a removed obstacle."""
    for e in range(eng.N):
        st = eng.get_state(e)
        for i, life in ((5, -32700), (6, -32768), (7, -32769), (8, -40000 + e), (9, -33000)):
            st.obst_life[i] = life
        st.obst_life[3] = -5
        st.obst_present[3] = 0
        dw = st.dead_words.view(np.uint32)
        for cell in (0, 4 + (e % 3), 12, 19):  # (0, 0) and the top row are walls, (2, 2) is free, (4, 3) a wall
            dw[cell >> 5] |= np.uint32(1 << (cell & 31))
        eng.set_state(e, st)


# id -> (config builder, envs per source, policy size, poke)
SHAPES = {
    "bridge64_a2_z10_i64": (_bridge64(2, 10, I64), 37, 7, None),
    "bridge64_a4_z20_i16": (_bridge64(4, 20, I16), 67, 7, None),
    "wall_hp_i16": (_wall_hp(I16), 13, 7, _poke_wall_hp),
    "wall_hp_i32": (_wall_hp(I32), 13, 7, _poke_wall_hp),
    "wall_hp_i16_simple": (_wall_hp(I16, "simple"), 13, 7, _poke_wall_hp),  # the record keeps int32 HP
    "bridge_single_world_i32": (_bridge_single, 13, 6, None),
    "city128_a4_z50_i64": (_city128, 13, 7, None),
}


def _guarded(torch, dev, rows, nb, fill):
    """A [rows, nb] record tensor inside a byte tensor filled with `fill`, 64 guard bytes either side."""
    big = torch.full((64 + rows * nb + 64,), fill, dtype=torch.uint8, device=dev)
    return big, big[64:64 + rows * nb].view(rows, nb)


def _check_content(eng, rec, envs):
    """Record sections, through the layout's offsets, against zs_get_state."""
    L = eng.obs_state_layout()
    E = eng.E
    for e in envs:
        st = eng.get_state(e)
        r = rec[e]

        def sec(name, nbytes, dt):
            return r[L[name]:L[name] + nbytes].copy().view(dt)
        pos = sec("pos", 4 * E, np.int32)
        assert np.array_equal((pos & 0xffff).astype(np.int16).astype(np.int32), st.ent[:, 2]), ("x", e)
        assert np.array_equal(pos >> 16, st.ent[:, 3]), ("y", e)
        assert np.array_equal(sec("life", 4 * E, np.int32), st.ent[:, 4]), ("life", e)
        assert np.array_equal(sec("weapon", E, np.uint8).astype(np.int32), st.ent[:, 5]), ("weapon", e)
        assert np.array_equal(sec("present", E, np.uint8).astype(np.int32), st.ent[:, 1]), ("present", e)
        dw = len(st.dead_words)
        assert np.array_equal(sec("dead", 4 * dw, np.uint32), st.dead_words.view(np.uint32)), ("dead", e)
        ow = (st.O + 31) // 32
        bits = np.unpackbits(sec("obst_present", 4 * ow, np.uint32).view(np.uint8), bitorder="little")[:st.O]
        assert np.array_equal(bits.astype(np.int32), st.obst_present), ("obst_present", e)
        if L["hp_bytes"] == 2:
            hp = sec("obst_hp", 2 * st.O, np.int16).astype(np.int32)
            assert np.array_equal(hp, np.maximum(st.obst_life, -32768)), ("obst_hp", e)
        else:
            assert np.array_equal(sec("obst_hp", 4 * st.O, np.int32), st.obst_life), ("obst_hp", e)
        assert not r[L["pad"]:].any(), ("padding", e)


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_pack_unpack_reencode_is_bit_identical(shape):
    import torch

    from libzombsole_amd.engine import Engine
    mk, m, n_discrete, poke = SHAPES[shape]
    dev = torch.device("cuda", 0)
    srcs = [Engine(mk(m), device=0) for _ in range(2)]
    viewer = Engine(mk(2 * m + 3, viewer=True), device=0)
    V = viewer.N
    L = srcs[0].obs_state_layout()
    nb = L["rec_bytes"]
    assert viewer.obs_state_layout() == L == srcs[0].builder.obs_state_layout() and nb % 16 == 0
    narrow = srcs[0].builder.cfg.obs_dtype == I16 and srcs[0].builder.cfg.obs_encoding == _abi.ENC_CHANNELS
    assert L["hp_bytes"] == (2 if narrow else 4)
    for k, eng in enumerate(srcs):
        eng.seed([1000 * (k + 1) + 7 * i for i in range(m)])
        eng.reset()
        if poke:
            poke(eng)
            eng.observe()
    tail0 = viewer.observe().clone()[2 * m:]  # the 3 envs no unpack writes
    g = torch.Generator().manual_seed(5)
    masks = [(torch.rand(V, generator=g) < p).to(torch.uint8).to(dev) for p in (0.5, 0.15)]
    for mk_ in masks:
        mk_[0] = 1  # never empty
        mk_[2 * m] = 1  # and with an unwritten env
    # the unwritten envs under each masked launch too (never reset, their state is a fresh handle's zeros: the
    # masked and the unmasked kernel need not agree on it, each must keep giving what it gave)
    tail0m = []
    for mask in masks:
        buf = torch.zeros_like(viewer.obs)
        viewer.observe(mask=mask, out=buf)
        tail0m.append(buf[2 * m:].clone())
    for t in range(STEPS + 1):
        if t:
            for eng in srcs:
                eng.gen_actions(t, n_discrete)
                eng.step()
        if t not in CHECK_AT:
            continue
        torch.cuda.synchronize()
        exp = torch.cat([srcs[0].obs, srcs[1].obs], dim=0)
        # guards: the records sit inside 0x5A bytes; a second pack into 0xA5 bytes writes the same bytes
        recs = []
        for k, eng in enumerate(srcs):
            big, rec = _guarded(torch, dev, m, nb, 0x5A)
            assert eng.pack_obs_state(out=rec) is rec
            big2, rec2 = _guarded(torch, dev, m, nb, 0xA5)
            eng.pack_obs_state(out=rec2)
            torch.cuda.synchronize()
            assert bool((big[:64] == 0x5A).all()) and bool((big[-64:] == 0x5A).all()), (shape, t, k)
            assert bool((big2[:64] == 0xA5).all()) and bool((big2[-64:] == 0xA5).all()), (shape, t, k)
            assert torch.equal(rec, rec2), (shape, t, k)  # every byte written, padding included
            assert torch.equal(eng.pack_obs_state(), rec)
            _check_content(eng, rec.cpu().numpy(), (0, m // 2, m - 1))
            recs.append(rec)
        viewer.unpack_obs_state(recs[0])
        viewer.unpack_obs_state(recs[1], env0=m)
        got = viewer.observe()
        torch.cuda.synchronize()
        assert torch.equal(got[:2 * m], exp), (shape, t, "unmasked")
        assert torch.equal(got[2 * m:], tail0), (shape, t, "unwritten envs")
        sentinel = 0x1234
        for j, mask in enumerate(masks):
            buf = torch.full_like(viewer.obs, sentinel)
            viewer.observe(mask=mask, out=buf)
            torch.cuda.synchronize()
            on = mask[:2 * m].bool()
            assert torch.equal(buf[:2 * m][on], exp[on]), (shape, t, "masked", j)
            assert bool((buf[:2 * m][~on] == sentinel).all()), (shape, t, "masked: other rows", j)
            tail_on = mask[2 * m:].bool()
            assert torch.equal(buf[2 * m:][tail_on], tail0m[j][tail_on]), (shape, t, "masked tail", j)
    # the wall_hp runs did cross the int16 floor
    if poke:
        assert srcs[0].overflow() & _abi.OVF_INT16
        assert viewer.overflow() == 0  # the sources' range flags do not travel
    # a partial unpack touches only its envs: rank 1's first two records over envs [1, 3)
    before = viewer.observe().clone()
    viewer.unpack_obs_state(recs[1], env0=1, n=2)
    got = viewer.observe().clone()
    torch.cuda.synchronize()
    assert torch.equal(got[1:3], srcs[1].obs[:2]) and torch.equal(got[0], before[0]) and torch.equal(got[3:], before[3:])
    for eng in srcs + [viewer]:
        eng.close()


def test_refusals_are_host_side():
    """ZS_ESTATE: unpack on a non-viewer; zs_step, zs_reset, zs_seed (and the other state-changing calls) on a
    viewer.  ZS_EINVAL: a wrong rec_bytes, env0 + n > N, a negative env0.  Nothing is launched: the viewer
    observes the same before and after."""
    import torch

    from libzombsole_amd.engine import Engine, EngineError, _ptr
    mk = _bridge64(2, 10, I64)
    src = Engine(mk(9), device=0)
    viewer = Engine(mk(12, viewer=True), device=0)
    src.seed(list(range(40, 49)))
    src.reset()
    rec = src.pack_obs_state()
    viewer.unpack_obs_state(rec, env0=3)
    good = viewer.observe().clone()
    torch.cuda.synchronize()
    assert torch.equal(good[3:12], src.obs)
    Lb, nb = src.L, rec.shape[1]
    # ZS_ESTATE
    assert Lb.zs_obs_state_unpack(src.h, _ptr(rec), nb, 0, 9, None) == _abi.ZS_ESTATE
    assert b"viewer" in Lb.zs_last_error()
    o = viewer.out
    assert Lb.zs_step(viewer.h, _ptr(viewer.actions), _ptr(o.obs), _ptr(o.rewards), _ptr(o.done), _ptr(o.trunc),
                      _ptr(o.listed), _ptr(o.was_reset), None) == _abi.ZS_ESTATE
    assert Lb.zs_step_graph(viewer.h, 1, 7, _ptr(viewer.actions), _ptr(o.obs), _ptr(o.rewards), _ptr(o.done),
                            _ptr(o.trunc), _ptr(o.listed), _ptr(o.was_reset), None) == _abi.ZS_ESTATE
    assert Lb.zs_reset(viewer.h, None, _ptr(o.obs), None) == _abi.ZS_ESTATE
    seeds = (C.c_uint64 * 1)(5)
    assert Lb.zs_seed(viewer.h, 0, 1, seeds, None) == _abi.ZS_ESTATE
    assert Lb.zs_gen_actions(viewer.h, 1, 7, _ptr(viewer.actions), None) == _abi.ZS_ESTATE
    st = viewer.get_state(4)  # zs_get_state works on a viewer ...
    assert np.array_equal(st.ent[:, 4], src.get_state(1).ent[:, 4])
    with pytest.raises(EngineError):  # ... zs_set_state does not
        viewer.set_state(4, st)
    with pytest.raises(EngineError):
        viewer.set_rng(0, src.get_rng(0))
    with pytest.raises(EngineError):
        viewer.host_observe(np.zeros((12, 4096), dtype=np.int32))
    for call in (viewer.step, viewer.reset, lambda: viewer.seed([1])):
        with pytest.raises(EngineError):
            call()
    # ZS_EINVAL
    for args in ((nb + 16, 0, 9), (nb - 16, 0, 9), (nb, 4, 9), (nb, -1, 2), (nb, 0, 13), (nb, 12, 1), (nb, 0, -1)):
        assert Lb.zs_obs_state_unpack(viewer.h, _ptr(rec), args[0], args[1], args[2], None) == _abi.ZS_EINVAL, args
    with pytest.raises(ValueError):
        viewer.unpack_obs_state(rec, env0=4)
    with pytest.raises(ValueError):
        viewer.unpack_obs_state(rec[:, :nb - 16].contiguous())
    with pytest.raises(ValueError):
        src.pack_obs_state(out=torch.empty((8, nb), dtype=torch.uint8, device=src.device))  # fewer rows than envs
    assert viewer.describe()["envs"] == 12 and viewer.overflow() == 0 and viewer.obs_shape == src.obs_shape
    again = viewer.observe()
    torch.cuda.synchronize()
    assert torch.equal(again, good)
    src.close()
    viewer.close()
