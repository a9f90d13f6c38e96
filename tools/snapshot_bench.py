#!/usr/bin/env python
"""Times snapshot, restore and clone of all envs on one MI355X and writes profiles/snapshot_bench.json.

Shapes: C3 (bridge64, 2 agents + 10 zombies) at 65 536 envs and at the 8 192-env shard, C5 (bridge64, 4 agents + 20
zombies, int16) at 65 536, C4 (city128, 4 agents + 50 zombies kept at 50) at 16 384.  Per shape: Engine.snapshot
of all envs, Engine.restore of all envs (check=False: the copy launch and the pending-list launch), clone of all
envs onto themselves shifted by one (snapshot + restore through a scratch tensor), and as the yardstick a
device-to-device Tensor.copy_ of n * rec_bytes bytes in the same process.  Also the per-env route this replaces
(get_state + get_rng, set_state + set_rng) over 256 envs, wall-clock, scaled to n and labelled as scaled.

Method: every timed call is warmed up, then timed `--reps` times between HIP events on the launch stream with the
kinds of call interleaved; the figure is the median (min and max are kept).

    python tools/snapshot_bench.py [--out profiles/snapshot_bench.json] [--reps 50] [--only c3_65536,...]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from libzombsole_amd import _abi  # noqa: E402


def c3(n):
    return _abi.multi_env_config(n, "extermination", [], "bridge64", ["0", "1"], initial_zombies=10,
                                 minimum_zombies=0, max_episode_steps=1000)


def c5(n):
    return _abi.multi_env_config(n, "extermination", [], "bridge64", ["0", "1", "2", "3"], initial_zombies=20,
                                 minimum_zombies=0, max_episode_steps=1000, obs_dtype=_abi.DTYPE_I16)


def c4(n):
    return _abi.multi_env_config(n, "safehouse", [], "city128", ["0", "1", "2", "3"], initial_zombies=50,
                                 minimum_zombies=50, max_episode_steps=1000)


CASES = {"c3_65536": (c3, 65536), "c3_8192": (c3, 8192), "c5_65536": (c5, 65536), "c4_16384": (c4, 16384)}


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


def case(torch, name, mk, n, reps):
    from libzombsole_amd.engine import Engine
    eng = Engine(mk(n), device=0)
    eng.seed(list(range(n)))
    eng.reset()
    for t in range(1, 21):  # a played state: bodies, damaged obstacles, advanced streams
        eng.step_graph(t, 7)
    nb = eng.snapshot_layout()["rec_bytes"]
    rec = eng.snapshot()
    scratch, dst = torch.empty_like(rec), torch.empty_like(rec)
    shifted = torch.roll(torch.arange(n, dtype=torch.int32, device=eng.device), 1)
    ident = torch.arange(n, dtype=torch.int32, device=eng.device)

    def clone():
        eng.snapshot(envs=ident, out=scratch)
        eng.restore(scratch, dst=shifted, check=False)

    calls = {"snapshot": lambda: eng.snapshot(out=scratch), "restore": lambda: eng.restore(rec, check=False),
             "clone": clone, "copy": lambda: dst.copy_(rec)}
    us = time_calls(torch, calls, reps)
    eng.restore(rec, check=False)
    torch.cuda.synchronize()
    assert torch.equal(eng.snapshot(), rec), "restore + snapshot is not the identity"
    row = {"case": name, "envs": n, "rec_bytes": nb, "bytes": n * nb}
    for k in calls:
        row[k] = stats(us[k])
    for k in ("snapshot", "restore", "clone"):
        row[k + "_over_copy"] = round(row[k]["median_us"] / row["copy"]["median_us"], 2)
    for k in ("snapshot", "restore", "copy"):  # bytes read + bytes written over the median
        row[k + "_GBps"] = round(2 * n * nb / row[k]["median_us"] / 1e3, 1)
    # the per-env route, wall-clock over 256 envs (each call synchronises), scaled to n
    m = min(256, n)
    t0 = time.perf_counter()
    got = [(eng.get_state(e), eng.get_rng(e)) for e in range(m)]
    t1 = time.perf_counter()
    for e, (st, rng) in enumerate(got):
        eng.set_state(e, st)
        eng.set_rng(e, rng)
    t2 = time.perf_counter()
    row["per_env_route"] = {"envs_timed": m, "get_us_per_env": round(1e6 * (t1 - t0) / m, 1),
                            "set_us_per_env": round(1e6 * (t2 - t1) / m, 1),
                            "get_us_scaled_to_n": round(1e6 * (t1 - t0) / m * n), "set_us_scaled_to_n": round(1e6 * (t2 - t1) / m * n),
                            "note": "scaled: measured over envs_timed envs, multiplied up to n"}
    eng.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "snapshot_bench.json"))
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    import torch
    names = [s for s in a.only.split(",") if s] or list(CASES)
    rows = []
    for name in names:
        mk, n = CASES[name]
        rows.append(case(torch, name, mk, n, max(50, a.reps)))
        print(json.dumps(rows[-1]), flush=True)
    with open(a.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "method": "HIP events on the launch stream, median of reps, "
                   "calls interleaved; copy = Tensor.copy_ of n * rec_bytes bytes", "cases": rows}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
