"""The snapshot record and fingerprint (libzombsole_amd/csrc/zs_snapshot.hpp) on the CPU: the header compiled with
the host compiler into tests/snapshot_layout_dump.cpp, against the engine arrays' per-env sizes written out by hand,
the pure-Python mirrors in _abi, and the checkpoint file helpers of vector.py on CPU tensors."""
import copy
import os
import re

import pytest

import step_plan_table as T
from libzombsole_amd import _abi, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (E, O, DW, OW, A)
SHAPES = {
    "E7_A1_O0": (7, 0, 47, 0, 1),                 # odd E: the byte rows start at odd offsets; no obstacle
    "bridge64_E12_A2": (12, 384, 128, 12, 2),     # C2 / C3
    "city128_a4_z50": (54, 3640, 512, 114, 4),    # C4
    "A_plus_P_65": (70, 16, 1, 1, 3),             # 3 agents + 62 bots + 5 zombies
    "O4200": (12, 4200, 512, 132, 2),
}


@pytest.fixture(scope="module")
def rows():
    return dict(zip(SHAPES, T.dump("snapshot_layout_dump", ["L %d %d %d %d %d" % s for s in SHAPES.values()])))


def by_hand(E, O, DW, OW, A):
    """Per-env bytes of every engine array a record copies (zs_device.hpp Dev; create_env_arrays), in record order."""
    return [("ring", 4 * 2 * 624),      # uint32 ring[N][2][624]
            ("dead", 4 * DW),           # uint32 dead[N][DW]
            ("obst_hp", 4 * O),         # int32 obst_hp[N][O]
            ("obst_present", 4 * OW),   # uint32 obst_present[N][OW]
            ("obst_nonpos", 4 * OW),    # uint32 obst_nonpos[N][OW]
            ("pos", 4 * E),             # int32 pos[N][E]
            ("life", 4 * E),            # int32 life[N][E]
            ("serial", 4 * E),          # uint32 serial[N][E]
            ("scal", 4 * 9),            # int32 scal[S_NSCAL = 9][N]
            ("hp_dirty", 4),            # uint32 hp_dirty[N]
            ("dead_dirty", 4),          # uint32 dead_dirty[N]
            ("rngst", 4),               # uint32 rngst[N]
            ("prev_life", 4 * A),       # int32 prev_life[A][N]
            ("weapon", E),              # uint8 weapon[N][E]
            ("present", E),             # uint8 present[N][E]
            ("order", E),               # uint8 order[N][E]
            ("listed", A)]              # uint8 listed[A][N]


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_sections_tile_the_record(rows, shape):
    r, sizes = rows[shape], by_hand(*SHAPES[shape])
    assert [n for n, _ in sizes] == list(_abi.SNAPSHOT_SECTIONS) and r["nsec"] == len(sizes) == 17
    o = 0
    for name, nb in sizes:  # disjoint, in order, no gap: every section starts where the one before ends
        assert r[name] == o, (name, r)
        o += nb
    assert r["pad"] == o  # the sections cover [0, pad)
    assert r["rec_bytes"] % 16 == 0 and 0 <= r["rec_bytes"] - r["pad"] < 16
    for name, _ in sizes[:13]:  # the 4-byte sections
        assert r[name] % 4 == 0, name
    assert [n for n, _ in sizes[13:]] == ["weapon", "present", "order", "listed"]  # the byte rows come last
    assert r["nscal"] == _abi.SNAPSHOT_NSCAL == 9 and r["ring_words"] == _abi.SNAPSHOT_RING == 1248


def test_header_equals_the_python_mirror(rows):
    for shape, s in SHAPES.items():
        exp = _abi.snapshot_layout(*s)
        assert {k: rows[shape][k] for k in exp} == exp, shape
        assert [b for _, b in by_hand(*s)] == list(_abi.snapshot_section_bytes(*s))


def test_scalar_rows_match_the_device_header():
    src = open(os.path.join(ROOT, "libzombsole_amd", "csrc", "zs_device.hpp")).read()
    body = re.search(r"enum \{\s*S_T = 0,(.*?)S_NSCAL", src, re.S).group(1)
    assert 1 + len(re.findall(r"^\s*S_\w+,", body, re.M)) == _abi.SNAPSHOT_NSCAL


# -- the fingerprint ---------------------------------------------------------------------------------------------
def base_cfg():
    """A config's covered fields and tables as a dict (bridge64, 2 agents and a bot; tables shortened so each entry
    can be changed in turn) plus the three fields the fingerprint leaves out."""
    return {"num_envs": 37, "obs_dtype": _abi.DTYPE_I64, "lanes_per_env": 0,
            "W": 64, "H": 64, "rules": _abi.RULES_EXTERMINATION, "reward_mode": _abi.REWARD_MULTI, "max_episode_steps": 5,
            "initial_zombies": 10, "minimum_zombies": 2,
            "agent_weapons": [_abi.WEAPON_RIFLE, _abi.WEAPON_GUN], "bot_types": [_abi.BOT_SNIPER],
            "obstacle_xy": [3, 4, 5, 6, 7, 8], "obstacle_kind": [_abi.THING_BOX, _abi.THING_WALL, _abi.THING_WALL],
            "objective_xy": [1, 1, 2, 2], "player_spawn_xy": [10, 10, 11, 10], "zombie_spawn_xy": [40, 40, 41, 40, 42, 40]}


def fp_line(c):
    head = [c["num_envs"], c["obs_dtype"], c["lanes_per_env"], c["W"], c["H"], c["rules"], c["reward_mode"],
            c["max_episode_steps"], c["initial_zombies"], c["minimum_zombies"], len(c["agent_weapons"]), len(c["bot_types"]),
            len(c["obstacle_kind"]), len(c["objective_xy"]) // 2, len(c["player_spawn_xy"]) // 2, len(c["zombie_spawn_xy"]) // 2]
    assert len(c["obstacle_xy"]) == 2 * len(c["obstacle_kind"])
    tabs = c["obstacle_xy"] + c["obstacle_kind"] + c["player_spawn_xy"] + c["zombie_spawn_xy"] + c["objective_xy"] + \
        c["agent_weapons"] + c["bot_types"]
    return "F " + " ".join(str(int(v)) for v in head + tabs)


def fingerprints(cfgs):
    return [r["fp_lo"] | (r["fp_hi"] << 32) for r in T.dump("snapshot_layout_dump", [fp_line(c) for c in cfgs])]


def test_fingerprint_changes_with_every_covered_field_and_entry():
    base = base_cfg()
    variants, names = [], []
    for k in ("W", "H", "rules", "reward_mode", "max_episode_steps", "initial_zombies", "minimum_zombies"):
        c = copy.deepcopy(base)
        c[k] += 1
        variants.append(c), names.append(k)
    # minimum above initial changes Z and E as well; initial_zombies alone changed both above
    for k in ("agent_weapons", "bot_types", "obstacle_xy", "obstacle_kind", "objective_xy", "player_spawn_xy",
              "zombie_spawn_xy"):
        for i in range(len(base[k])):  # every entry of every table
            c = copy.deepcopy(base)
            c[k][i] += 1
            variants.append(c), names.append("%s[%d]" % (k, i))
    # the counts: one agent more (A, E), one bot more (P, E), one obstacle / spawn / objective fewer
    c = copy.deepcopy(base); c["agent_weapons"].append(_abi.WEAPON_AXE); variants.append(c); names.append("A")
    c = copy.deepcopy(base); c["bot_types"].append(_abi.BOT_TROLL); variants.append(c); names.append("P")
    c = copy.deepcopy(base); c["obstacle_xy"] = c["obstacle_xy"][:4]; c["obstacle_kind"] = c["obstacle_kind"][:2]
    variants.append(c); names.append("O")
    for k in ("objective_xy", "player_spawn_xy", "zombie_spawn_xy"):
        c = copy.deepcopy(base); c[k] = c[k][:-2]; variants.append(c); names.append("n " + k)
    # an entry moved from one table to the next is another config too
    c = copy.deepcopy(base); c["player_spawn_xy"] = base["player_spawn_xy"][:2]
    c["zombie_spawn_xy"] = base["player_spawn_xy"][2:] + base["zombie_spawn_xy"]; variants.append(c); names.append("moved")
    fps = fingerprints([base] + variants)
    for name, fp in zip(names, fps[1:]):
        assert fp != fps[0], name
    assert len(set(fps)) == len(fps)


def test_fingerprint_ignores_env_count_dtype_and_lanes():
    base = base_cfg()
    variants = []
    for k, v in (("num_envs", 65536), ("obs_dtype", _abi.DTYPE_I16), ("lanes_per_env", 8)):
        c = copy.deepcopy(base)
        c[k] = v
        variants.append(c)
    fps = fingerprints([base] + variants)
    assert fps[1:] == [fps[0]] * 3


def _builder_line(b):
    c, m = b.cfg, b.cfg.map
    return fp_line({"num_envs": c.num_envs, "obs_dtype": c.obs_dtype, "lanes_per_env": c.lanes_per_env, "W": m.width,
                    "H": m.height, "rules": c.rules, "reward_mode": c.reward_mode, "max_episode_steps": c.max_episode_steps,
                    "initial_zombies": c.initial_zombies, "minimum_zombies": c.minimum_zombies,
                    "agent_weapons": list(c.agent_weapons[:c.num_agents]), "bot_types": list(c.bot_types[:c.num_bots]),
                    "obstacle_xy": list(m.obstacle_xy[:2 * m.n_obstacles]), "obstacle_kind": list(m.obstacle_kind[:m.n_obstacles]),
                    "objective_xy": list(m.objective_xy[:2 * m.n_objectives]),
                    "player_spawn_xy": list(m.player_spawn_xy[:2 * m.n_player_spawns]),
                    "zombie_spawn_xy": list(m.zombie_spawn_xy[:2 * m.n_zombie_spawns])})


def test_builder_layout_and_fingerprint_mirror():
    """ConfigBuilder.snapshot_layout(): the header's layout and fingerprint of real configs; handles that differ in
    env count, observation dtype, lanes per env, launch overrides or the viewer flag share a fingerprint."""
    mk = lambda n, **kw: _abi.multi_env_config(n, "extermination", [], "bridge64", ["0", "1"], initial_zombies=10,  # noqa: E731
                                               max_episode_steps=5, **kw)
    a, b = mk(13), mk(21, obs_dtype=_abi.DTYPE_I16, lanes_per_env=8, viewer=True).set_launch({"fused": -1})
    s = _abi.single_env_config(13, "extermination", ["terminator", "sniper"], "bridge", 0, initial_zombies=4,
                               max_episode_steps=5)
    La, Lb, Ls = a.snapshot_layout(), b.snapshot_layout(), s.snapshot_layout()
    assert La == Lb and La["fingerprint"] != Ls["fingerprint"]
    assert {k: v for k, v in La.items() if k != "fingerprint"} == _abi.snapshot_layout(*SHAPES["bridge64_E12_A2"])
    assert La["rec_bytes"] == 7376
    got = T.dump("snapshot_layout_dump", [_builder_line(x) for x in (a, b, s)])
    assert [r["fp_lo"] | (r["fp_hi"] << 32) for r in got] == [La["fingerprint"], Lb["fingerprint"], Ls["fingerprint"]]
    other = mk(13, minimum_zombies=3)
    assert other.snapshot_layout()["fingerprint"] != La["fingerprint"]


def test_symbols():
    for name in ("zs_snapshot_layout", "zs_snapshot", "zs_restore"):
        assert name in engine.SYMBOLS


# -- checkpoint files (vector.write_checkpoint / read_checkpoint) on CPU tensors -----------------------------------
@pytest.fixture()
def ckpt(tmp_path):
    import torch

    from libzombsole_amd import vector
    rec = (torch.arange(5 * 48, dtype=torch.int64) % 251).to(torch.uint8).view(5, 48)
    path = str(tmp_path / "run.ckpt")
    vector.write_checkpoint(path, rec, 0xFEDCBA9876543210, 5, env0=8192, base_seed=7)
    return vector, path, rec


def test_checkpoint_round_trip(ckpt):
    import torch
    vector, path, rec = ckpt
    ck = vector.read_checkpoint(path, 0xFEDCBA9876543210, 48, 5)
    assert sorted(ck) == sorted(vector.CHECKPOINT_KEYS)
    assert torch.equal(ck["records"], rec) and ck["records"].dtype == torch.uint8
    assert (ck["fingerprint"], ck["rec_bytes"], ck["num_envs"], ck["env0"], ck["base_seed"]) == \
        (0xFEDCBA9876543210, 48, 5, 8192, 7)


def test_checkpoint_refusals(ckpt, tmp_path):
    import torch
    vector, path, rec = ckpt
    with pytest.raises(ValueError, match="fingerprint"):
        vector.read_checkpoint(path, 0xFEDCBA9876543211, 48, 5)
    with pytest.raises(ValueError, match="bytes"):
        vector.read_checkpoint(path, 0xFEDCBA9876543210, 64, 5)
    with pytest.raises(ValueError, match="envs"):
        vector.read_checkpoint(path, 0xFEDCBA9876543210, 48, 6)
    with pytest.raises(ValueError):
        vector.write_checkpoint(str(tmp_path / "bad.ckpt"), rec, 1, 6)  # records of another env count
    other = str(tmp_path / "other.pt")
    torch.save({"records": rec}, other)
    with pytest.raises(ValueError, match="not a checkpoint"):
        vector.read_checkpoint(other, 1, 48, 5)
