#!/usr/bin/env python3
"""The head of the step from a rocprofv3 --kernel-trace CSV of a bench run (diagnostic): per step, the gap from the
end of the previous step's observation kernel to the start of the tick, the gap from the start of the policy launch
(k_gen_actions_ctr, when the graph has one) to the start of the tick, and the step period (tick start to tick start);
medians over the last K steps.
    python tools/trace_head.py <dir with *kernel_trace.csv> [K]"""
import csv
import glob
import os
import sys


def short(n):
    return n.split("(")[0].replace("void ", "").split("<")[0].strip()


def median(v):
    v = sorted(v)
    return v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])


def head_gaps(rows, K):
    """rows: (start ns, end ns, kernel) sorted by start.  {name: (median us, n)}"""
    obs_end = pol_start = None
    tick_starts, obs_gap, pol_gap, tick_dur, obs_dur = [], [], [], [], []
    for st, en, nm in rows:
        if nm == "k_gen_actions_ctr":
            pol_start = st
        elif nm in ("k_tick", "k_step"):
            if obs_end is not None:
                obs_gap.append((st - obs_end) / 1e3)
                if pol_start is not None:
                    pol_gap.append((st - pol_start) / 1e3)
            tick_starts.append(st)
            tick_dur.append((en - st) / 1e3)
            pol_start = None
        elif nm.startswith("k_obs"):
            obs_end = en
            obs_dur.append((en - st) / 1e3)
    period = [(b - a) / 1e3 for a, b in zip(tick_starts, tick_starts[1:])]
    out = {}
    for name, v in (("obs_end_to_tick_start_us", obs_gap), ("policy_start_to_tick_start_us", pol_gap),
                    ("tick_us", tick_dur), ("obs_us", obs_dur), ("step_period_us", period)):
        v = v[-K:]
        out[name] = (round(median(v), 2), len(v)) if v else (None, 0)
    return out


def main():
    src = sys.argv[1]
    K = int(sys.argv[2]) if len(sys.argv) > 2 else 100
    rows = []
    for f in glob.glob(os.path.join(src, "**", "*kernel_trace.csv"), recursive=True):
        with open(f) as fh:
            for r in csv.DictReader(fh):
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short(r["Kernel_Name"])))
    rows.sort()
    for name, (m, n) in head_gaps(rows, K).items():
        print("%-32s median %s over %d" % (name, m, n))


if __name__ == "__main__":
    main()
