#!/usr/bin/env python
"""Times the action-mask kernel (k_action_mask) on one MI355X and writes profiles/mask_bench.json.

Shapes: C3 (bridge64, 2 agents + 10 zombies) at 65 536 envs and at the 8 192-env shard, C2 (the same at 4 096) and
C5 (bridge64, 4 agents + 20 zombies, int16) at 65 536.  Two results per shape:

  standalone   Engine.action_mask of all envs, beside Engine.observe of all envs in the same interleaved run, and
               the mask kernel's algorithmic bytes (an env's pos, present and weapon rows, its obstacle-present
               words, the masks written) over the HBM peak
  step         env-steps/s of step_graph, one step per graph launch, on one handle with a bound mask buffer and
               on one without, the two handles' launches interleaved

Method: every timed call is warmed up, then timed `--reps` times between HIP events on the launch stream with the
kinds of call interleaved; the figure is the median (min and max are kept).

    python tools/mask_bench.py [--out profiles/mask_bench.json] [--reps 50] [--only c3_65536,...]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from libzombsole_amd import _abi  # noqa: E402

HBM_PEAK_GBPS = 8000.0


def c3(n):
    return _abi.multi_env_config(n, "extermination", [], "bridge64", ["0", "1"], initial_zombies=10,
                                 minimum_zombies=0, max_episode_steps=1000)


def c5(n):
    return _abi.multi_env_config(n, "extermination", [], "bridge64", ["0", "1", "2", "3"], initial_zombies=20,
                                 minimum_zombies=0, max_episode_steps=1000, obs_dtype=_abi.DTYPE_I16)


CASES = {"c3_65536": (c3, 65536), "c3_8192": (c3, 8192), "c2_4096": (c3, 4096), "c5_65536": (c5, 65536)}


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


def played(mk, n, bind):
    from libzombsole_amd.engine import Engine
    eng = Engine(mk(n), device=0)
    eng.seed(list(range(n)))
    eng.reset()
    if bind:
        eng.bind_action_masks()
    for t in range(1, 21):  # a played state: bodies, moved zombies, some envs reset
        eng.step_graph(t, 7)
    return eng


def case(torch, name, mk, n, reps):
    plain, bound = played(mk, n, False), played(mk, n, True)
    out = torch.zeros((n, plain.A, 8), dtype=torch.uint8, device=plain.device)
    us = time_calls(torch, {"mask": lambda: plain.action_mask(out=out), "observe": plain.observe}, reps)
    assert torch.equal(out, bound.action_mask(out=torch.zeros_like(out))), "the two handles ran the same envs"
    b = plain.builder
    ow = (len(b.map.obstacles) + 31) // 32
    per_env = 6 * plain.E + 4 * ow + 8 * plain.A  # pos i32 + present u8 + weapon u8 per slot, obstacle words, masks
    row = {"case": name, "envs": n, "entities": plain.E, "agents": plain.A, "mask": stats(us["mask"]),
           "observe": stats(us["observe"]), "obs_kernel": plain.describe()["obs_kernel"],
           "mask_bytes_per_env": per_env, "mask_bytes": n * per_env}
    row["mask_GBps"] = round(n * per_env / row["mask"]["median_us"] / 1e3, 1)
    row["mask_fraction_of_hbm_peak"] = round(row["mask_GBps"] / HBM_PEAK_GBPS, 4)
    row["mask_us_at_hbm_peak"] = round(n * per_env / HBM_PEAK_GBPS / 1e3, 2)
    row["mask_over_observe"] = round(row["mask"]["median_us"] / row["observe"]["median_us"], 4)
    ctr = {"plain": 21, "bound": 21}

    def stepper(key, eng):
        def fn():
            eng.step_graph(ctr[key], 7)
            ctr[key] += 1
        return fn

    us = time_calls(torch, {"step_unbound": stepper("plain", plain), "step_bound": stepper("bound", bound)}, reps)
    for k in ("step_unbound", "step_bound"):
        row[k] = stats(us[k])
        row[k + "_env_steps_per_s"] = round(n / row[k]["median_us"] * 1e6)
    row["bound_step_cost_us"] = round(row["step_bound"]["median_us"] - row["step_unbound"]["median_us"], 2)
    row["bound_step_cost_fraction"] = round(row["bound_step_cost_us"] / row["step_unbound"]["median_us"], 4)
    plain.close()
    bound.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mask_bench.json"))
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
                   "calls interleaved; step = step_graph with the on-device policy, one step per graph launch",
                   "hbm_peak_GBps": HBM_PEAK_GBPS, "cases": rows}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
