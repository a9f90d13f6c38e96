"""StepGather(mode="state") on one MI355X, world-size-1 RCCL group (set up as in test_sharding_gpu.py).

The C5 shape with 131 envs on two engines with the same seeds, one under StepGather(mode="obs") and one under
StepGather(mode="state"): the state mode packs the step's records, unpacks them into its viewer and re-encodes
them with the viewer's observation kernel, and every gathered value must equal the obs mode's, every step,
autoresets included (max_episode_steps = 3).
"""
import socket

import pytest

from libzombsole_amd import _abi

pytestmark = pytest.mark.gpu

N = 131


def _c5(n, **kw):
    return _abi.multi_env_config(n, "extermination", [], "bridge64", ["0", "1", "2", "3"], initial_zombies=20,
                                 minimum_zombies=0, max_episode_steps=3, obs_dtype=_abi.DTYPE_I16, **kw)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _engines():
    from libzombsole_amd.engine import Engine
    engs = []
    for _ in range(2):
        eng = Engine(_c5(N), device=0)
        eng.seed([300 + i for i in range(N)])
        eng.reset()
        engs.append(eng)
    return engs


NAMES = ("obs", "rewards", "done", "truncated", "listed", "was_reset")


@pytest.mark.parametrize("self_exchange", [False, True])
def test_state_mode_equals_obs_mode(self_exchange):
    import torch
    import torch.distributed as dist

    from libzombsole_amd.engine import Engine
    from libzombsole_amd.vector import StepGather

    dev = torch.device("cuda", 0)
    dist.init_process_group("nccl", init_method="tcp://127.0.0.1:%d" % _free_port(), rank=0, world_size=1,
                            device_id=dev)
    try:
        ea, eb = _engines()
        ga = StepGather(ea, self_exchange=self_exchange)
        viewer = Engine(_c5(N, viewer=True), device=0) if self_exchange else None  # given, or built by StepGather
        gb = StepGather(eb, self_exchange=self_exchange, mode="state", viewer=viewer)
        assert ga.mode == "obs" and ga.g_state is None and ga.viewer is None
        L = eb.obs_state_layout()
        assert L["rec_bytes"] == 1584 and gb.viewer.N == N and gb.viewer.builder.cfg.flags & _abi.FLAG_VIEWER
        assert all(g.shape == (N, 1584) for g in gb.g_state)
        assert all(s.state.data_ptr() == gb.g_state[k].data_ptr() for k, s in enumerate(gb.sets))
        resets = 0
        for t in range(1, 9):
            ga.step(lambda o: ea.step_graph(t, 7, out=o))
            def run_b(o):  # the step's own observations wiped: what obs() returns can only be the viewer's
                eb.step_graph(t, 7, out=o)
                o.obs.fill_(-7)
            out = gb.step(run_b)
            assert out is gb.sets[(t - 1) % 2]
            torch.cuda.synchronize()
            for name in NAMES:
                assert torch.equal(getattr(ga, name)(), getattr(gb, name)()), (name, t)
            # the gathered observations are the viewer's re-encoding of the records, not the step's own
            assert gb.obs().data_ptr() == gb.g_obs[(t - 1) % 2].data_ptr()
            assert torch.equal(gb.viewer.pack_obs_state(), eb.pack_obs_state())
            resets += int(gb.was_reset().sum())
        assert resets > N  # TimeLimit 3: every env was autoreset at least once
        gb.close()
        for e in (ea, eb) + ((viewer,) if viewer is not None else ()):
            e.close()
    finally:
        dist.destroy_process_group()


def test_state_mode_in_flight():
    """depth = 2 with steps in flight: 8 steps issued back to back with no host sync; a consumer on the
    communication stream (after=) hashes each step's gathered observations and flat buffer there, right after the
    viewer's re-encode.  The hashes equal those of a reference engine stepped alone."""
    import torch
    import torch.distributed as dist

    from libzombsole_amd.vector import StepGather

    dev = torch.device("cuda", 0)
    dist.init_process_group("nccl", init_method="tcp://127.0.0.1:%d" % _free_port(), rank=0, world_size=1,
                            device_id=dev)
    try:
        steps = 8
        eng, ref = _engines()
        g = StepGather(eng, depth=2, self_exchange=True, mode="state")
        assert not g.skip and g.comm is not None
        hashes = torch.zeros((steps, 2), dtype=torch.int64, device=dev)
        wts = torch.arange(1, g.g_obs[0].numel() + 1, dtype=torch.int64, device=dev) % 1000003
        on_comm = []

        def hash_into(t):
            def after(k):
                on_comm.append(torch.cuda.current_stream(dev) == g.comm)
                hashes[t - 1, 0] = (g.g_obs[k].reshape(-1).to(torch.int64) * wts).sum()
                hashes[t - 1, 1] = (g.g_flat[k].to(torch.int64) * wts[:g.g_flat[k].numel()]).sum()
            return after

        for t in range(1, steps + 1):
            g.step(lambda o: eng.step_graph(t, 7, out=o), after=hash_into(t))
        exp = torch.zeros_like(hashes)
        for t in range(1, steps + 1):
            ref.step_graph(t, 7)
            exp[t - 1, 0] = (ref.obs.reshape(-1).to(torch.int64) * wts).sum()
            exp[t - 1, 1] = (ref.out.flat.to(torch.int64) * wts[:ref.out.flat.numel()]).sum()
        torch.cuda.synchronize()
        g.wait()
        torch.cuda.synchronize()
        assert all(on_comm) and len(on_comm) == steps
        assert torch.equal(hashes, exp), (hashes - exp).abs().sum(dim=1).tolist()
        assert torch.equal(g.obs(copy=True), ref.obs)
        g.close()
        eng.close()
        ref.close()
    finally:
        dist.destroy_process_group()
