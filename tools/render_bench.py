#!/usr/bin/env python3
"""Measure zs_render and the body-colour tracker (ZS_FLAG_RENDER) and write profiles/render_bench.json.

HIP events around each call, 50 interleaved repetitions after a warm-up, medians.
  * k_render for 64 and 1 024 envs of C3 (bridge64) and 64 envs of C4 (city128), against a Tensor.copy_ of the same
    number of bytes in the same process (the yardstick of the snapshot work);
  * the tracker's cost: the graphed step of a flagged handle, of one with the death log alone and of an unflagged one,
    at C3 with 65 536 envs and at the 8 192-env shard (flag_us: flagged - unflagged; tracker_us: flagged - logs).

    python tools/render_bench.py [--reps 50] [--out profiles/render_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from libzombsole_amd import _abi  # noqa: E402
from libzombsole_amd.engine import Engine  # noqa: E402


def c3(n, render):
    return _abi.multi_env_config(n, "extermination", [], "bridge64", ["0", "1"], initial_zombies=10, minimum_zombies=0,
                                 max_episode_steps=1000, render=render)


def c4(n, render):
    return _abi.multi_env_config(n, "safehouse", [], "city128", ["0", "1", "2", "3"], initial_zombies=50,
                                 minimum_zombies=50, max_episode_steps=1000, render=render)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3  # us


def interleaved(fns, reps, warmup=5):
    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            out[k].append(timed(f))
    return {k: statistics.median(v) for k, v in out.items()}


def render_row(name, builder, n_total, n_frames, reps):
    eng = Engine(builder(n_total, True))
    eng.reset()
    for t in range(1, 31):  # some bodies and destroyed obstacles
        eng.step_graph(t, eng.n_discrete)
    envs = torch.arange(n_frames, dtype=torch.int32, device=eng.device)
    out = eng.render(envs)
    nbytes = out.numel()
    # the yardstick rotates over enough buffer pairs that no copy finds its bytes in the 256 MB cache the one before left
    pairs = max(2, -(-(1 << 30) // (2 * nbytes)))
    bufs = [(torch.empty_like(out), out.clone()) for _ in range(pairs)]
    turn = [0]

    def copy():
        dst, src = bufs[turn[0] % pairs]
        turn[0] += 1
        dst.copy_(src)
    med = interleaved({"render_us": lambda: eng.render(envs, out=out), "copy_us": copy}, reps)
    eng.close()
    return dict(name=name, frames=n_frames, bytes=nbytes, ratio=med["render_us"] / med["copy_us"],
                render_gb_s=nbytes / med["render_us"] / 1e3, copy_gb_s=nbytes / med["copy_us"] / 1e3, **med)


def tracker_row(n, reps):
    engs = {}
    for key, flag in (("unflagged_us", False), ("logs_us", None), ("flagged_us", True)):
        b = c3(n, bool(flag))
        if flag is None:  # the death and action logs alone: what the flag costs in the tick, without k_render_track
            b.cfg.flags |= _abi.FLAG_DEATH_LOG
        e = Engine(b)
        e.reset()
        engs[key] = e
    step = {k: [20] for k in engs}

    def stepper(k):
        def f():
            step[k][0] += 1
            engs[k].step_graph(step[k][0], 7)
        return f
    for k in engs:
        for t in range(1, 21):
            engs[k].step_graph(t, 7)
    med = interleaved({k: stepper(k) for k in engs}, reps)
    for e in engs.values():
        e.close()
    return dict(envs=n, flag_us=med["flagged_us"] - med["unflagged_us"], tracker_us=med["flagged_us"] - med["logs_us"], **med)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_bench.json"))
    a = ap.parse_args()
    res = {"reps": a.reps, "device": torch.cuda.get_device_name(0),
           "render": [render_row("C3 bridge64", c3, 1024, 64, a.reps), render_row("C3 bridge64", c3, 1024, 1024, a.reps),
                      render_row("C4 city128", c4, 64, 64, a.reps)],
           "tracker": [tracker_row(65536, a.reps), tracker_row(8192, a.reps)]}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
