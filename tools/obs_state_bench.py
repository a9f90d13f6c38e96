#!/usr/bin/env python
"""Times the observation-state record path on one MI355X and writes profiles/obs_state.json.

Per shape (C5: bridge64, 4 agents + 20 zombies, int16; C3: bridge64, 2 agents + 10 zombies, int64) and env count
(8 192 and 65 536): zs_obs_state_pack, zs_obs_state_unpack into a viewer handle of as many envs, and a
Tensor.copy_ of the same byte count as the yardstick; at 65 536 envs also the viewer's re-encode (zs_observe).
Then the C5 8 192-env shard's step under StepGather(mode="obs") and StepGather(mode="state") at world size 1
(collectives skipped: the state mode's cost is its pack + unpack + re-encode).

Method: every timed call is warmed up, then timed `--reps` times between HIP events on the launch stream with
the three kinds of call interleaved; the figure is the median (min and max are kept).  The step loops are timed
as `--steps` steps between two events, the two modes alternating, `--loops` times each.

    python tools/obs_state_bench.py [--out profiles/obs_state.json] [--reps 50] [--steps 200] [--loops 5]
"""
import argparse
import json
import os
import socket
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import libzombsole_amd  # noqa: E402

libzombsole_amd.plain_graph_dispatch()  # the graph dispatch bench.py times, before the first HIP call
from libzombsole_amd import _abi  # noqa: E402


def c5(n, **kw):
    return _abi.multi_env_config(n, "extermination", [], "bridge64", ["0", "1", "2", "3"], initial_zombies=20,
                                 minimum_zombies=0, max_episode_steps=1000, obs_dtype=_abi.DTYPE_I16, **kw)


def c3(n, **kw):
    return _abi.multi_env_config(n, "extermination", [], "bridge64", ["0", "1"], initial_zombies=10,
                                 minimum_zombies=0, max_episode_steps=1000, **kw)


def stats(us):
    return {"median_us": round(statistics.median(us), 2), "min_us": round(min(us), 2), "max_us": round(max(us), 2),
            "reps": len(us)}


def time_calls(torch, calls, reps, warmup=5):
    """{name: [us]}: the calls interleaved, each between two events on the current stream."""
    for _ in range(warmup):
        for fn in calls.values():
            fn()
    torch.cuda.synchronize()
    ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
          for k in calls}
    for r in range(reps):
        for k, fn in calls.items():
            ev[k][r][0].record()
            fn()
            ev[k][r][1].record()
    torch.cuda.synchronize()
    return {k: [1000.0 * a.elapsed_time(b) for a, b in ev[k]] for k in calls}


def records(torch, mk, name, n, reps, with_observe):
    from libzombsole_amd.engine import Engine
    src = Engine(mk(n), device=0)
    src.seed(list(range(n)))
    src.reset()
    for t in range(1, 21):  # a played state: bodies, damaged obstacles
        src.step_graph(t, 7)
    viewer = Engine(mk(n, viewer=True), device=0)
    nb = src.obs_state_layout()["rec_bytes"]
    rec = src.pack_obs_state()
    dst = torch.empty_like(rec)
    calls = {"pack": lambda: src.pack_obs_state(out=rec), "unpack": lambda: viewer.unpack_obs_state(rec),
             "copy": lambda: dst.copy_(rec)}
    if with_observe:
        out = torch.empty_like(viewer.obs)
        calls["viewer_observe"] = lambda: viewer.observe(out=out)
    us = time_calls(torch, calls, reps)
    torch.cuda.synchronize()
    viewer.observe()
    torch.cuda.synchronize()
    assert torch.equal(viewer.obs, src.obs), "re-encoded observations differ"
    obs_bytes = src.obs[0].numel() * src.obs.element_size()
    row = {"shape": name, "envs": n, "rec_bytes": nb, "obs_bytes_per_env": obs_bytes, "bytes": n * nb,
           "obs_kernel": viewer.describe()["obs_kernel"]}
    for k in calls:
        row[k] = stats(us[k])
    for k in ("pack", "unpack"):
        row[k + "_over_copy"] = round(row[k]["median_us"] / row["copy"]["median_us"], 2)
        # bytes read + bytes written over the median
        row[k + "_GBps"] = round(2 * n * nb / row[k]["median_us"] / 1e3, 1)
    row["copy_GBps"] = round(2 * n * nb / row["copy"]["median_us"] / 1e3, 1)
    src.close()
    viewer.close()
    return row


def step_modes(torch, n, steps, loops):
    import torch.distributed as dist

    from libzombsole_amd.engine import Engine
    from libzombsole_amd.vector import StepGather
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    dist.init_process_group("nccl", init_method="tcp://127.0.0.1:%d" % port, rank=0, world_size=1,
                            device_id=torch.device("cuda", 0))
    try:
        g, eng, t0 = {}, {}, {}
        for mode in ("obs", "state"):
            eng[mode] = Engine(c5(n), device=0)
            eng[mode].seed(list(range(n)))
            eng[mode].reset()
            g[mode] = StepGather(eng[mode], mode=mode)
            t0[mode] = 1
        us = {"obs": [], "state": []}

        def loop(mode, k):
            e = eng[mode]
            for _ in range(k):
                t = t0[mode]
                g[mode].step(lambda o: e.step_graph(t, 7, out=o))
                t0[mode] += 1

        for mode in us:
            loop(mode, 20)
        torch.cuda.synchronize()
        for _ in range(loops):
            for mode in us:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                loop(mode, steps)
                b.record()
                torch.cuda.synchronize()
                us[mode].append(1000.0 * a.elapsed_time(b) / steps)
        assert torch.equal(g["obs"].obs(), g["state"].obs()), "the two modes' observations differ"
        row = {"shape": "c5", "envs": n, "world": 1, "steps_per_loop": steps,
               "step_obs_mode": stats(us["obs"]), "step_state_mode": stats(us["state"])}
        g["state"].close()
        for e in eng.values():
            e.close()
        return row
    finally:
        dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "obs_state.json"))
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--loops", type=int, default=5)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("obs_state_bench: no HIP device; nothing is measured without one")
    res = {"device": torch.cuda.get_device_name(0), "method": "HIP events on the launch stream, medians; see the "
           "module docstring of tools/obs_state_bench.py", "records": [], "step": None}
    for name, mk in (("c5", c5), ("c3", c3)):
        for n in (8192, 65536):
            res["records"].append(records(torch, mk, name, n, a.reps, n == 65536))
            print(json.dumps(res["records"][-1]), flush=True)
    res["step"] = step_modes(torch, 8192, a.steps, a.loops)
    print(json.dumps(res["step"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
