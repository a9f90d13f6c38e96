"""StepGather(mode="state") on two gloo ranks (CPU): 25 envs split 13 + 12, stand-in engines as in
test_sharding_gloo.py.

The stand-in's observation-state record is an invertible encoding of its step-tagged observation (the bytes
xor 0xA7, reversed, zero-padded to a multiple of 16) and a stand-in viewer decodes it, so the state mode's
whole path runs without a device: pack into the rank's slice of g_state, the all-gather of g_state and the flat
buffer, unpack of all world * m rows, re-encode into g_obs.  Every step's gathered values must equal those of a
mode="obs" StepGather fed the same steps, and padding rows (rank 1 has one) must never reach them.
"""
import os
import socket

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

TOTAL, STEPS = 25, 5
SHAPE = (2, 3, 5, 5)
OBS_BYTES = 4 * 2 * 3 * 5 * 5
REC_BYTES = (OBS_BYTES + 15) // 16 * 16
POISON = 0x7E7E7E7E  # what a stand-in viewer makes of a zero record's row: never a real observation


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from libzombsole_amd.engine import StepOutputs
        from libzombsole_amd.vector import StepGather, shard_range
        e0, n = shard_range(TOTAL, rank, world)
        gl = torch.arange(e0, e0 + n)

        class Fake(object):
            N, A, multi, obs_shape, obs_dtype, device, torch = n, 2, True, SHAPE, torch.int32, torch.device("cpu"), torch
            packs = 0

            def outputs(self, rows=None, obs=None, flat=None):
                return StepOutputs(self, max(rows or n, n), obs, flat)

            def obs_state_layout(self):
                return {"rec_bytes": REC_BYTES}

            def pack_obs_state(self, out=None):
                assert out.shape == (13, REC_BYTES) and out.dtype == torch.uint8
                b = self.cur.obs[:n].contiguous().view(torch.uint8).view(n, OBS_BYTES)
                out[:n, :OBS_BYTES] = (b ^ 0xA7).flip(1)
                out[:n, OBS_BYTES:] = 0
                self.packs += 1
                return out

        class FakeViewer(object):
            N = world * 13
            unpacks = 0

            def obs_state_layout(self):
                return {"rec_bytes": REC_BYTES}

            def unpack_obs_state(self, rec, env0=0, n=None):
                assert rec.shape == (self.N, REC_BYTES) and env0 == 0 and n is None
                self.rec = rec.clone()
                self.unpacks += 1

            def observe(self, mask=None, out=None):
                assert mask is None and out.shape == (self.N,) + SHAPE
                b = (self.rec[:, :OBS_BYTES].flip(1) ^ 0xA7).contiguous()
                out.copy_(b.view(torch.int32).view((self.N,) + SHAPE))
                zero = (self.rec == 0).all(dim=1)
                out[zero] = POISON
                return out

        def run(eng, t):
            def fill(out):
                out.obs[:n] = 10 * gl.view(-1, 1, 1, 1, 1).int() + 1000 * t + \
                    torch.arange(150, dtype=torch.int32).view(SHAPE)
                out.rewards[:n] = ((gl.double() / 4) + t).view(-1, 1).repeat(1, 2)
                out.done[:n] = ((gl + t) % 2).to(torch.uint8)
                out.trunc[:n] = ((gl + t) % 3 == 0).to(torch.uint8)
                out.listed[:n] = torch.stack([(gl + t) % 5 != 0, (gl + 2 * t) % 7 != 0], 1).to(torch.uint8)
                out.was_reset[:n] = ((gl * 3 + t) % 4 == 0).to(torch.uint8)
                eng.cur = out
            return fill

        fo, fs, viewer = Fake(), Fake(), FakeViewer()
        so = StepGather(fo)
        ss = StepGather(fs, mode="state", viewer=viewer)
        ok = so.mode == "obs" and so.g_state is None and ss.mode == "state" and len(ss.g_state) == 2
        ok = ok and all(g.shape == (world * 13, REC_BYTES) and g.dtype == torch.uint8 for g in ss.g_state)
        # the sets' records are this rank's slices of g_state (in-place collective), their other storage as in mode="obs"
        ok = ok and all(s.state.data_ptr() == ss.g_state[k][13 * rank:].data_ptr() and s.state.shape == (13, REC_BYTES)
                        for k, s in enumerate(ss.sets))
        ok = ok and all(s.obs.data_ptr() == ss.g_obs[k][13 * rank:].data_ptr() for k, s in enumerate(ss.sets))
        ga = torch.arange(TOTAL)
        seen_after = []
        for t in range(STEPS):
            so.step(run(fo, t))
            used = ss.step(run(fs, t), after=seen_after.append)
            ok = ok and used is ss.sets[t % 2] and seen_after[-1] == t % 2
            ok = ok and fs.packs == t + 1 and viewer.unpacks == t + 1 and fo.packs == 0
            for name in ("obs", "rewards", "done", "truncated", "listed", "was_reset"):
                a, b = getattr(so, name)(), getattr(ss, name)()
                ok = ok and a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b)
            ok = ok and ss.obs().shape[0] == TOTAL
            ok = ok and torch.equal(ss.obs()[:, 0, 0, 0, 0], ga.int() * 10 + 1000 * t)
            # rank 1's padding row: a zero record in g_state, the viewer's poison in g_obs, in no result
            k = t % 2
            ok = ok and bool((ss.g_state[k][25] == 0).all()) and bool((ss.g_obs[k][25] == POISON).all())
            ok = ok and not bool((ss.obs() == POISON).any())
            # every rank's records arrived: row 13 is rank 1's first env
            ok = ok and torch.equal(ss.g_state[k][13, :OBS_BYTES],
                                    (ss.g_obs[k][13].contiguous().view(torch.uint8).view(-1) ^ 0xA7).flip(0))
        ss.close()
        q.put((rank, bool(ok)))
    finally:
        dist.destroy_process_group()


def test_state_mode_equals_obs_mode_on_two_ranks():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=240) for _ in range(2))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert res == {0: True, 1: True}
