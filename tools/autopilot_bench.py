#!/usr/bin/env python
"""Times the scripted-policy kernel (k_autopilot) on one MI355X and writes profiles/autopilot_bench.json.

Shapes: C3 (bridge64, 2 agents + 10 zombies) and C5 (bridge64, 4 agents + 20 zombies, int16) at 65 536 envs.  Two
results per shape:

  standalone   Engine.autopilot of all envs under the terminator policy (the one that reduces over the zombies), beside
               Engine.action_mask of all envs in the same interleaved run: the yardstick, a kernel of the same mapping
               over the same rows.  The autopilot adds the order row and one cell lookup per agent.  Also its
               algorithmic bytes (an env's pos, present, weapon and order rows, its obstacle-present words, its dict
               length, the policy codes read and the triples written) over the HBM peak
  step         env-steps/s of step_graph, one step per graph launch, on one handle with a bound autopilot and on one
               without, the two handles' launches interleaved; and the spread of the unbound step over `--runs`
               repeats of that measurement

Method: every timed call is warmed up, then timed `--reps` times between HIP events on the launch stream with the
kinds of call interleaved; the figure is the median (min and max are kept).

    python tools/autopilot_bench.py [--out profiles/autopilot_bench.json] [--reps 50] [--runs 5] [--only c3_65536,...]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from mask_bench import HBM_PEAK_GBPS, c3, c5, stats, time_calls  # noqa: E402

CASES = {"c3_65536": (c3, 65536), "c5_65536": (c5, 65536)}


def played(mk, n, bind):
    from libzombsole_amd.engine import Engine
    eng = Engine(mk(n), device=0)
    eng.seed(list(range(n)))
    eng.reset()
    if bind:
        eng.bind_autopilot("terminator")
    for t in range(1, 21):  # a played state: bodies, moved zombies, some envs reset
        eng.step_graph(t, 7)
    return eng


def case(torch, name, mk, n, reps, runs):
    plain, bound = played(mk, n, False), played(mk, n, True)
    pol = plain.policy_tensor("terminator")
    out = torch.zeros((n, plain.A, 3), dtype=torch.int32, device=plain.device)
    masks = torch.zeros((n, plain.A, 8), dtype=torch.uint8, device=plain.device)
    us = time_calls(torch, {"autopilot": lambda: plain.autopilot(pol, out=out),
                            "mask": lambda: plain.action_mask(out=masks)}, reps)
    assert torch.equal(out, bound.pilot), "the two handles ran the same envs"
    ow = (len(plain.builder.map.obstacles) + 31) // 32
    per_env = 7 * plain.E + 4 * ow + 4 + 13 * plain.A  # pos i32 + present, weapon, order u8 per slot; codes + triples
    row = {"case": name, "envs": n, "entities": plain.E, "agents": plain.A, "autopilot": stats(us["autopilot"]),
           "mask": stats(us["mask"]), "autopilot_bytes_per_env": per_env, "autopilot_bytes": n * per_env}
    row["autopilot_over_mask"] = round(row["autopilot"]["median_us"] / row["mask"]["median_us"], 4)
    row["autopilot_GBps"] = round(n * per_env / row["autopilot"]["median_us"] / 1e3, 1)
    row["autopilot_fraction_of_hbm_peak"] = round(row["autopilot_GBps"] / HBM_PEAK_GBPS, 4)
    row["autopilot_us_at_hbm_peak"] = round(n * per_env / HBM_PEAK_GBPS / 1e3, 2)
    ctr = {"plain": 21, "bound": 21}

    def stepper(key, eng):
        def fn():
            eng.step_graph(ctr[key], 7)
            ctr[key] += 1
        return fn

    meds = {"step_unbound": [], "step_bound": []}
    for _ in range(runs):
        us = time_calls(torch, {"step_unbound": stepper("plain", plain), "step_bound": stepper("bound", bound)}, reps)
        for k in meds:
            meds[k].append(stats(us[k])["median_us"])
    for k in meds:
        row[k] = stats(us[k])
        row[k + "_run_medians_us"] = meds[k]
        row[k + "_env_steps_per_s"] = round(n / min(meds[k]) * 1e6)
    row["step_unbound_run_spread"] = round((max(meds["step_unbound"]) - min(meds["step_unbound"])) / min(meds["step_unbound"]), 4)
    row["bound_step_cost_us"] = round(min(meds["step_bound"]) - min(meds["step_unbound"]), 2)
    row["bound_step_cost_fraction"] = round(row["bound_step_cost_us"] / min(meds["step_unbound"]), 4)
    plain.close()
    bound.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "autopilot_bench.json"))
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    import torch
    names = [s for s in a.only.split(",") if s] or list(CASES)
    rows = []
    for name in names:
        mk, n = CASES[name]
        rows.append(case(torch, name, mk, n, max(50, a.reps), max(1, a.runs)))
        print(json.dumps(rows[-1]), flush=True)
    with open(a.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "method": "HIP events on the launch stream, median of reps, "
                   "calls interleaved; step = step_graph with the on-device policy, one step per graph launch; the "
                   "unbound step's spread over repeated runs of the measurement", "hbm_peak_GBps": HBM_PEAK_GBPS,
                   "cases": rows}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
