#!/usr/bin/env python
"""What ZS_FLAG_EPISODE_STATS costs a step, and whether an unflagged handle is the parent's: writes
profiles/episode_stats_ab.log.

Shapes: C3 (bridge64, 2 agents + 10 zombies, 65 536 envs), C5 (4 agents + 20 zombies, int16, 65 536) and the
8 192-env C3 shard.  Per shape, handles stepped through step_graph (the on-device policy, one step per graph launch),
200 timed steps each after a warm-up, their launches interleaved step by step on one stream in one process (the same
box, the same minute), each step between two HIP events:

  plain     this build, no flag
  flagged   this build, ZS_FLAG_EPISODE_STATS: the step ends with k_episode_stats
  parent    --parent-lib: a library built from the parent commit's sources (no flag exists there), twice (parent_a,
            parent_b), so the parent measured against itself gives the run-to-run spread a difference is read against

The figure is the median step time; min and max are kept.

    python tools/episode_stats_ab.py [--parent-lib PATH] [--steps 200] [--only c3,c5,shard]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from libzombsole_amd import _abi, engine  # noqa: E402


def c3(n, **kw):
    return _abi.multi_env_config(n, "extermination", [], "bridge64", ["0", "1"], initial_zombies=10,
                                 minimum_zombies=0, max_episode_steps=1000, **kw)


def c5(n, **kw):
    return _abi.multi_env_config(n, "extermination", [], "bridge64", ["0", "1", "2", "3"], initial_zombies=20,
                                 minimum_zombies=0, max_episode_steps=1000, obs_dtype=_abi.DTYPE_I16, **kw)


CASES = {"c3": (c3, 65536), "c5": (c5, 65536), "shard": (c3, 8192)}


def bind(path):
    """The library at `path` with the binding's prototypes; a parent build lacks the newest entry points."""
    import ctypes as C
    ref = engine.load_library(engine.LIB_PATH)
    if path == engine.LIB_PATH:
        return ref
    L = C.CDLL(path)
    for s in engine.SYMBOLS:
        if hasattr(L, s):
            getattr(L, s).argtypes, getattr(L, s).restype = getattr(ref, s).argtypes, getattr(ref, s).restype
    return L


def handle(lib, mk, n, flagged):
    engine._lib = bind(lib)  # an Engine binds the library current at its construction
    eng = engine.Engine(mk(n, episode_stats=True) if flagged else mk(n), device=0)
    eng.seed(list(range(n)))
    eng.reset()
    return eng


def run(torch, engines, steps, warmup=30):
    t = {k: 1 for k in engines}

    def step(k):
        engines[k].step_graph(t[k], 7)
        t[k] += 1
    for _ in range(warmup):
        for k in engines:
            step(k)
    torch.cuda.synchronize()
    ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
          for k in engines}
    for r in range(steps):
        for k in engines:
            ev[k][r][0].record()
            step(k)
            ev[k][r][1].record()
    torch.cuda.synchronize()
    return {k: [1000.0 * a.elapsed_time(b) for a, b in ev[k]] for k in engines}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "episode_stats_ab.log"))
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    import torch
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("# %s; step_graph, one step per launch, %d timed steps per handle, handles interleaved\n"
                % (torch.cuda.get_device_name(0), a.steps))
        for name in [s for s in a.only.split(",") if s] or list(CASES):
            mk, n = CASES[name]
            engines = {"plain": handle(engine.LIB_PATH, mk, n, False), "flagged": handle(engine.LIB_PATH, mk, n, True)}
            if a.parent_lib:
                engines["parent_a"] = handle(a.parent_lib, mk, n, False)
                engines["parent_b"] = handle(a.parent_lib, mk, n, False)
            us = run(torch, engines, a.steps)
            row = {"case": name, "envs": n}
            for k, v in us.items():
                row[k] = {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)}
            row["flag_cost_us"] = round(row["flagged"]["median_us"] - row["plain"]["median_us"], 2)
            if a.parent_lib:
                row["plain_minus_parent_us"] = round(row["plain"]["median_us"] - row["parent_a"]["median_us"], 2)
                row["parent_spread_us"] = round(abs(row["parent_a"]["median_us"] - row["parent_b"]["median_us"]), 2)
            line = json.dumps(row)
            print(line, flush=True)
            f.write(line + "\n")
            for e in engines.values():
                e.close()


if __name__ == "__main__":
    main()
