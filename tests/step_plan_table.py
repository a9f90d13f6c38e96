"""The (shape, overrides) matrix of the step plan (libzombsole_amd/csrc/zs_step_plan.hpp), the table of what every
pair resolved to before the plan existed (tests/step_plan_expected.json, one row per pair) and the compiled plan
itself (tests/step_plan_dump.cpp built with the host compiler, once per process).  test_step_plan.py checks the
plan against the table on the CPU; the GPU test of the step instantiations compares describe() with the table.

How the table's fields were obtained.  Every row was printed by a host program that wrapped the text of
choose_layout() and create_step_layout() of the commit before the plan, unmodified, round a stub handle (the HIP
calls stubbed to succeed, tick_layout() and reset_lds_bytes() copied from that commit's zs_tick.hpp / zs_reset.hpp),
never by step_plan():
  * G, fused, lds, resident, want, rw_cap, rw_step, cand_cap, lists_cap, rlists_cap, reset_lds: the handle's and
    Dev's fields after create_step_layout();
  * tick_waves: zs_describe()'s expression of that commit, fused ? ZS_FUSED_WAVES : h->tick_waves;
  * side_stream: reset_side after create_step_layout() with stream and event creation succeeding;
  * n_reset, reset_grid_list, reset_grid_mask, respawn_grid: the expressions of that commit's launch_tick(),
    launch_reset() and launch_respawn(), copied into the program;
  * defer_respawn: the rule inline in that commit's zs_create(), copied into the program;
  * obs_bytes (an input): obs_plan()'s fobs ? step image + 4 * obs_stat : 0, from tests/obs_plan_dump.cpp (the
    observation plan is not touched by the step plan).
The env counts of FLIPS were found by running the same program over every env count from 1 to 300 000 and
printing each count at which its result or its sequence of choose_layout() calls differed from the count before.
"""
import json
import os
import subprocess
import tempfile

import obs_plan_table
from libzombsole_amd import _abi

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FIELDS = ("G", "fused", "tick_waves", "lds", "resident", "want", "rw_cap", "rw_step", "cand_cap", "lists_cap",
          "rlists_cap", "reset_lds", "side_stream", "n_reset", "reset_grid_list", "reset_grid_mask", "respawn_grid",
          "defer_respawn")

# -- the compiled plans --------------------------------------------------------------------------------------------
_exes, _tmp = {}, None


def dump(program, lines):
    """tests/<program>.cpp, compiled once per process with the host compiler: one parsed JSON row per input line."""
    global _tmp
    if program not in _exes:
        _tmp = _tmp or tempfile.TemporaryDirectory(prefix="zs_plan_")
        exe = os.path.join(_tmp.name, program)
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "libzombsole_amd", "csrc"),
                               "-o", exe, os.path.join(HERE, program + ".cpp")])
        _exes[program] = exe
    out = subprocess.run([_exes[program]], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True)
    rows = [json.loads(l) for l in out.stdout.splitlines()]
    assert len(rows) == len(lines), (program, len(rows), len(lines))
    return rows


def launch_ints(lo):
    return [int((lo or {}).get(f, 0)) for f in _abi.LAUNCH_FIELDS]


def step_ints(builder, obs_bytes):
    """The StepShape of a config (zs_create's arithmetic on the config's integers), in the struct's order."""
    c, m = builder.cfg, builder.cfg.map
    cells = m.width * m.height
    E = c.num_agents + c.num_bots + max(c.initial_zombies, c.minimum_zombies)
    return [c.num_envs, m.width, m.height, E, c.num_agents, (cells + 31) // 32,
            max(m.n_player_spawns or cells, m.n_zombie_spawns or cells), m.n_player_spawns, m.n_zombie_spawns,
            c.minimum_zombies, c.lanes_per_env, obs_bytes]


def plans(pairs):
    """The compiled step plan of every (builder, zs_launch overrides) pair: the observation plan first (its step
    image is an input), then the step plan; each row carries its "obs_bytes"."""
    if not pairs:
        return []
    obs = dump("obs_plan_dump", [" ".join(str(v) for v in [0] + obs_plan_table.shape_ints(b, lo) + launch_ints(lo))
                                 for b, lo in pairs])
    nbytes = [r["step_img_bytes"] + 4 * r["obs_stat"] if r["fobs"] else 0 for r in obs]
    rows = dump("step_plan_dump", ["P " + " ".join(str(v) for v in step_ints(b, nb) + launch_ints(lo))
                                   for (b, lo), nb in zip(pairs, nbytes)])
    for r, nb in zip(rows, nbytes):
        r["obs_bytes"] = nb
    return rows


_defer = {}


def defer_respawn(builder, lo):
    """step_defer_respawn() of the config under the overrides, from the compiled plan."""
    ints = step_ints(builder, 0) + launch_ints(lo)
    key = (ints[1] * ints[2], ints[8], ints[9], int((lo or {}).get("defer_respawn", 0)))
    if key not in _defer:
        _defer[key] = dump("step_plan_dump", ["P " + " ".join(str(v) for v in ints)])[0]["defer_respawn"]
    return _defer[key]


def images(args):
    """step_plan_dump's image mode: per (fused, ne, E, DW, rw_cap, cand_cap, lists_cap, A, ncand, obs_bytes) the row
    {"tick": tick_layout().bytes, "reset": reset_lds_bytes(), "bytes": the launch's image}."""
    return dump("step_plan_dump", ["I " + " ".join(str(int(v)) for v in a) for a in args])


# -- the matrix ------------------------------------------------------------------------------------------------------
# "lanes_per_env" in a set of overrides is zs_config.lanes_per_env, not a zs_launch field
def split(lo):
    lo = dict(lo or {})
    return lo.pop("lanes_per_env", 0), lo


def ov_key(lo):
    return json.dumps(sorted((k, v) for k, v in (lo or {}).items() if v))


# env counts on either side of each point where a decision flips (defaults; see the module docstring)
FLIPS = {
    # c3: RNG window 512 -> 256 (9217); the fused "8 instead of 16" retry taken (11265), window shrinking under it
    # (14337, 18433, 20481), its fallback to 16 (22529), taken again (23553); automatic G 16 -> 8 (24577);
    # fused -> unfused, want at its cap with G = 16 (47105); automatic G 16 -> 8 unfused, tick_waves 6 -> 5 (49153);
    # want reaching 32 at G = 8 (63489)
    "c3": (9217, 11265, 14337, 18433, 20481, 22529, 23553, 24577, 47105, 49153, 63489),
    # c5: window (9217); fused -> unfused (23553); tick_waves 6 -> 5 (24577), want reaching 32 (31745), tick_waves
    # 5 -> 6 -> 5 -> 6 (40961, 49153, 61441)
    "c5": (9217, 23553, 24577, 31745, 40961, 49153, 61441),
    # c4: window (5121); fused -> unfused (11777); want reaching 32 (15873)
    "c4": (5121, 11777, 15873),
}


def _shapes():
    import step_instantiations as S
    import test_fullsize_parity as F
    sh = {}
    for name, (mk, n) in obs_plan_table.SHAPES.items():
        sh[name] = (lambda mk=mk, n=n: mk(n))
    for r in S.ROWS + S.SMALL_ROWS:  # with the row's lanes per env
        sh["row:" + r.id] = (lambda r=r: r.builder().set_launch(None))
    for n in (8192, 12288, 16384, 24576, 32768, 49152, 65536):
        sh["c3@%d" % n] = (lambda n=n: F.c3(n))
    for cfg, mk in (("c3", F.c3), ("c5", F.c5), ("c4", F.c4)):
        for first in FLIPS[cfg]:
            for n in (first - 1, first):
                sh["%s@%d" % (cfg, n)] = (lambda mk=mk, n=n: mk(n))
    sh["pen_quad@37"] = lambda: S.pen_quad(37)
    return sh


# the shapes every set of overrides goes with
CORE = ("c3@8192", "c3@16384", "c3@65536", "c5@4097", "c5@65536", "c4@24", "c4@16384", "pen_quad@37", "cityfs_world@16",
        "wall_hp_i64@64", "easy_exit_surr9@32")

OVERRIDES = [{}, {"fused": 1}, {"fused": -1}, {"tick_waves": 5}, {"tick_waves": 6}, {"fused": -1, "tick_waves": 5},
             {"fused": -1, "tick_waves": 6}, {"lds_budget": -1}, {"rw_need": 16}, {"rw_need": 64}, {"rw_need": 1000},
             {"reset_wgs": 1}, {"reset_wgs": 3}, {"fused": 1, "reset_wgs": 3}, {"reset_lists": -1},
             {"fused": -1, "reset_lists": -1}, {"reset_stream": -1}, {"fused": -1, "reset_stream": -1},
             {"reset_grid": 1}, {"reset_grid": 3}, {"respawn_grid": 1}, {"respawn_grid": 3}, {"defer_respawn": 1},
             {"defer_respawn": -1}, {"fobs": 1}, {"fobs": -1}, {"fobs": 1, "fused": -1}] + \
            [{"lanes_per_env": g} for g in (0, 1, 2, 4, 8, 16, 32, 64)]


def pairs():
    """[(shape name, overrides)]: every shape with no override, every row of step_instantiations with its own,
    every set of OVERRIDES with the CORE shapes; one entry per distinct pair."""
    import step_instantiations as S
    shapes = _shapes()
    out = [(name, {}) for name in shapes]
    out += [("row:" + r.id, dict(r.launch)) for r in S.ROWS + S.SMALL_ROWS]
    out += [(name, lo) for lo in OVERRIDES for name in CORE]
    seen, uniq = set(), []
    for name, lo in out:
        if (name, ov_key(lo)) not in seen:
            seen.add((name, ov_key(lo)))
            uniq.append((name, lo))
    return uniq


def resolve(pair_list):
    """The compiled plan's row of every (shape name, overrides) pair."""
    shapes = _shapes()
    built = []
    for name, lo in pair_list:
        lanes, launch = split(lo)
        b = shapes[name]()
        if lanes:
            b.cfg.lanes_per_env = lanes
        built.append((b, launch))
    return plans(built)


_rows = None


def expected(shape, lo):
    """The table's row for the shape under the overrides."""
    global _rows
    if _rows is None:
        with open(os.path.join(HERE, "step_plan_expected.json")) as f:
            _rows = {(r["shape"], ov_key(r["ov"])): r for r in json.load(f)}
    return _rows[(shape, ov_key(lo))]
