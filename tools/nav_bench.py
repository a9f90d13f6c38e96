#!/usr/bin/env python
"""Times the path-distance kernel (k_nav) on one MI355X and writes profiles/nav_bench.json (and a .log of its lines).

Shapes: C3 (bridge64, 2 agents + 10 zombies) at 65 536 envs and at the 8 192-env shard, C4 (city128, safehouse, 4 agents
+ 50 zombies) at 16 384 envs, and maze_for_safehouse (2 agents + 10 zombies, 16 384 envs) for the cap.  Per shape:

  standalone   Engine.nav_obs of all envs for the objective field, the zombie field and both, and Engine.nav_field of
               64 envs, between HIP events, the calls interleaved
  step         step_graph, one step per graph launch, on four handles played alike: nothing bound, the objective field
               bound, the zombie field bound, both bound; the handles' launches interleaved, `--runs` repeats of the
               measurement (min / median / max of the runs' medians)
  levels       the distribution, over 64 envs' states read back, of the levels a full search of each field runs
               (libzombsole_amd/nav.py levels) and of the level at which the last query of the rows is answered
  max_dist     (maze only) the both-fields bound step at max_dist 16, 64 and 32766

    python tools/nav_bench.py [--out profiles/nav_bench.json] [--reps 50] [--runs 5] [--only c3_65536,...]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from libzombsole_amd import _abi  # noqa: E402
from mask_bench import c3, stats, time_calls  # noqa: E402


def c4(n):
    return _abi.multi_env_config(n, "safehouse", [], "city128", ["0", "1", "2", "3"], initial_zombies=50,
                                 minimum_zombies=50, max_episode_steps=1000)


def maze(n):
    return _abi.multi_env_config(n, "safehouse", [], "maze_for_safehouse", ["0", "1"], initial_zombies=10,
                                 minimum_zombies=10, max_episode_steps=1000)


CASES = {"c3_65536": (c3, 65536, False), "c3_8192": (c3, 8192, False), "c4_16384": (c4, 16384, False),
         "maze_16384": (maze, 16384, True)}
BINDS = {"unbound": None, "objective": 1, "zombies": 2, "both": 3}


def played(mk, n, fields, max_dist=None):
    from libzombsole_amd.engine import Engine
    eng = Engine(mk(n), device=0)
    eng.seed(list(range(n)))
    eng.reset()
    if fields:
        eng.nav_bind(True, fields, max_dist)
    for t in range(1, 21):  # a played state: moved zombies, some envs reset
        eng.step_graph(t, 7)
    return eng


def level_stats(eng, envs=64):
    from libzombsole_amd import nav
    from libzombsole_amd.entity_obs import Static
    static = Static.of_map(eng.builder.map)
    out = {}
    views = [eng.get_state(k) for k in range(min(envs, eng.N))]
    for name, bit in (("objective", 1), ("zombies", 2)):
        full = [nav.levels(v, static, bit) for v in views]
        rows = [nav.encode(v, static, bit)[:, 0, :5].astype(int) for v in views]
        last = [int(r[r >= 0].max()) if (r >= 0).any() else 0 for r in rows]
        out[name] = {"full_search_levels": {"min": min(full), "median": statistics.median(full), "max": max(full)},
                     "last_query_answered_at": {"min": min(last), "median": statistics.median(last), "max": max(last)}}
    return out


def steppers(engs):
    ctr = {k: 21 for k in engs}

    def mk(key):
        def fn():
            engs[key].step_graph(ctr[key], 7)
            ctr[key] += 1
        return fn
    return {"step_" + k: mk(k) for k in engs}


def run_steps(torch, engs, reps, runs):
    calls = steppers(engs)
    meds = {k: [] for k in calls}
    for _ in range(runs):
        us = time_calls(torch, calls, reps)
        for k in meds:
            meds[k].append(stats(us[k])["median_us"])
    return {k: {"run_medians_us": v, "min_us": min(v), "median_us": round(statistics.median(v), 2), "max_us": max(v)}
            for k, v in meds.items()}


def case(torch, name, mk, n, caps, reps, runs):
    engs = {k: played(mk, n, f) for k, f in BINDS.items()}
    plain = engs["unbound"]
    row = {"case": name, "envs": n, "entities": plain.E, "agents": plain.A, "map": list(plain.builder.map.size),
           "plan": plain.nav_layout(3), "levels": level_stats(plain)}
    outs = {f: torch.zeros((n, plain.A, bin(f).count("1"), 8), dtype=torch.int16, device=plain.device) for f in (1, 2, 3)}
    W, H = plain.builder.map.size
    frames = torch.zeros((64, H, W), dtype=torch.int16, device=plain.device).view(torch.uint16)
    idx = torch.arange(64, dtype=torch.int32, device=plain.device)
    us = time_calls(torch, {"nav_objective": lambda: plain.nav_obs(out=outs[1], fields=1),
                            "nav_zombies": lambda: plain.nav_obs(out=outs[2], fields=2),
                            "nav_both": lambda: plain.nav_obs(out=outs[3], fields=3),
                            "nav_field_64_envs": lambda: plain.nav_field(1, idx, out=frames)}, reps)
    assert torch.equal(outs[3], engs["both"].nav), "the handles ran the same envs"
    row["standalone"] = {k: stats(v) for k, v in us.items()}
    row["step"] = run_steps(torch, engs, reps, runs)
    base = row["step"]["step_unbound"]["median_us"]
    row["bound_step_cost_us"] = {k: round(row["step"]["step_" + k]["median_us"] - base, 2) for k in BINDS if k != "unbound"}
    row["env_steps_per_s"] = {k: round(n / row["step"]["step_" + k]["median_us"] * 1e6) for k in BINDS}
    for e in engs.values():
        e.close()
    if caps:
        capped = {"cap%d" % c: played(mk, n, 3, c) for c in (16, 64, 32766)}
        row["max_dist"] = run_steps(torch, capped, reps, runs)
        for e in capped.values():
            e.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nav_bench.json"))
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    import torch
    names = [s for s in a.only.split(",") if s] or list(CASES)
    rows = []
    with open(os.path.splitext(a.out)[0] + ".log", "w") as log:
        for name in names:
            mk, n, caps = CASES[name]
            rows.append(case(torch, name, mk, n, caps, max(20, a.reps), max(1, a.runs)))
            line = json.dumps(rows[-1])
            print(line, flush=True)
            log.write(line + "\n")
    with open(a.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "method": "HIP events on the launch stream, median of reps, "
                   "calls interleaved; step = step_graph with the on-device policy, one step per graph launch, four "
                   "handles played alike; min / median / max over repeated runs of the measurement", "cases": rows}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
