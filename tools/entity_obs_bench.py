#!/usr/bin/env python
"""Times the entity-observation kernel (k_entity_obs) and the step without grid observations on one MI355X and writes
profiles/entity_obs_bench.json.

  kernel   Engine.entity_obs of all envs at (KZ, KP) = (4, 1) and (16, 16), beside a Tensor.copy_ of the same bytes and
           Engine.observe of all envs, at the C3 (bridge64, 65 536 envs), C4 (city128, 16 384) and C5 (bridge64 int16,
           65 536) shapes
  step     step_graph with the on-device policy, one step per graph launch, on three handles seeded alike: grid only (as
           today), grid plus a bound entity tensor, and entities with grid_obs=False; at C3, C5 and the 8 192-env shard.
           The tick's own time (zs_profile, eager steps of the grid-free handle) stands beside the third form: the gap
           between the two is the launch and tail cost

Method: every timed call is warmed up, then timed `--reps` times between HIP events on the launch stream with the kinds
of call interleaved; the figure is the median (min and max are kept).

    python tools/entity_obs_bench.py [--out profiles/entity_obs_bench.json] [--reps 50] [--only c3_65536,...]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from libzombsole_amd import _abi  # noqa: E402


def c3(n):
    return _abi.multi_env_config(n, "extermination", [], "bridge64", ["0", "1"], initial_zombies=10,
                                 minimum_zombies=0, max_episode_steps=1000)


def c4(n):
    return _abi.multi_env_config(n, "safehouse", [], "city128", ["0", "1", "2", "3"], initial_zombies=50,
                                 minimum_zombies=50, max_episode_steps=1000)


def c5(n):
    return _abi.multi_env_config(n, "extermination", [], "bridge64", ["0", "1", "2", "3"], initial_zombies=20,
                                 minimum_zombies=0, max_episode_steps=1000, obs_dtype=_abi.DTYPE_I16)


# name -> (config, envs, time the kernel, time the step)
CASES = {"c3_65536": (c3, 65536, True, True), "c4_16384": (c4, 16384, True, False), "c5_65536": (c5, 65536, True, True),
         "c3_8192": (c3, 8192, False, True)}
KS = ((4, 1), (16, 16))


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


def played(mk, n, bind, grid=True):
    from libzombsole_amd.engine import Engine
    eng = Engine(mk(n), device=0, grid_obs=grid)
    eng.seed(list(range(n)))
    eng.reset()
    if bind:
        eng.bind_entity_obs(True, *bind)
    for t in range(1, 21):  # a played state: bodies, moved zombies, some envs reset
        eng.step_graph(t, 7)
    return eng


def kernel_rows(torch, plain, reps):
    n, row = plain.N, {}
    calls = {"observe": plain.observe}
    bufs = {}
    for kz, kp in KS:
        words = _abi.entity_layout(kz, kp)["row_words"]
        out = torch.zeros((n, plain.A, words), dtype=torch.int16, device=plain.device)
        src = torch.ones_like(out)
        dst = torch.zeros_like(out)
        bufs[(kz, kp)] = out
        calls["entity_%d_%d" % (kz, kp)] = (lambda o=out, a=kz, b=kp: plain.entity_obs(out=o, kz=a, kp=b))
        calls["copy_%d_%d" % (kz, kp)] = (lambda s=src, d=dst: d.copy_(s))
    us = time_calls(torch, calls, reps)
    row["observe"] = stats(us["observe"])
    row["obs_kernel"] = plain.describe()["obs_kernel"]
    row["grid_bytes_per_env"] = plain.obs[0].numel() * plain.obs.element_size()
    for kz, kp in KS:
        k = "%d_%d" % (kz, kp)
        row["entity_" + k] = stats(us["entity_" + k])
        row["copy_" + k] = stats(us["copy_" + k])
        row["entity_bytes_per_env_" + k] = plain.A * _abi.entity_layout(kz, kp)["row_bytes"]
    return row


def step_rows(torch, mk, n, plain, reps):
    bound, nogrid = played(mk, n, (4, 1)), played(mk, n, (4, 1), grid=False)
    assert torch.equal(bound.entities, nogrid.entities), "the handles ran the same envs"
    ctr = {}

    def stepper(key, eng):
        ctr[key] = 21

        def fn():
            eng.step_graph(ctr[key], 7)
            ctr[key] += 1
        return fn

    us = time_calls(torch, {"step_grid": stepper("g", plain), "step_grid_entities": stepper("b", bound),
                            "step_entities_only": stepper("n", nogrid)}, reps)
    row = {}
    for k, v in us.items():
        row[k] = stats(v)
        row[k + "_env_steps_per_s"] = round(n / row[k]["median_us"] * 1e6)
    # the tick's own time: eager steps of the grid-free handle under zs_profile
    nogrid.profile(True)
    for t in range(ctr["n"], ctr["n"] + reps):
        nogrid.gen_actions(t, 7)
        nogrid.step()
    pr = nogrid.profile_read()
    nogrid.profile(False)
    row["tick_us"] = round(1000.0 * pr["tick_ms"] / max(pr["tick_n"], 1), 2)
    row["entities_only_minus_tick_us"] = round(row["step_entities_only"]["median_us"] - row["tick_us"], 2)
    row["describe_entities_only"] = {k: nogrid.describe()[k] for k in ("step_kernel", "obs_kernel", "respawn", "reset_side_stream")}
    bound.close()
    nogrid.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "entity_obs_bench.json"))
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    import torch
    names = [s for s in a.only.split(",") if s] or list(CASES)
    rows = []
    for name in names:
        mk, n, do_kernel, do_step = CASES[name]
        plain = played(mk, n, None)
        row = {"case": name, "envs": n, "entities": plain.E, "agents": plain.A}
        if do_kernel:
            row.update(kernel_rows(torch, plain, a.reps))
        if do_step:
            row.update(step_rows(torch, mk, n, plain, a.reps))
        plain.close()
        rows.append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "method": "HIP events on the launch stream, median of reps, "
                   "calls interleaved; step = step_graph with the on-device policy, one step per graph launch; tick_us = "
                   "zs_profile over eager steps", "cases": rows}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
