"""Every step-kernel instantiation (step_instantiations.py: lanes per env x k_step / k_tick at 5 / 6 waves) on the
GPU against the C oracle, every env at every step, at env counts that leave a partial last workgroup, with guard
bands round every buffer zs_step writes; then the grid-stride loops of the reset and respawn work (k_reset, the
reset role of a fused k_step, k_respawn) with fewer workgroups than envs to rebuild, so that one workgroup's LDS
image serves several envs in one launch.

Guard bands: rewards, done, truncated, listed, the reset flag and the actions each lie inside a byte tensor
filled with 0x5A, 64 B before and after.  Before every step the payloads are filled with 0x5A too: 0x5A is no
value done, truncated, listed or the reset flag can hold, so after the step every such byte of every env must
have been written, and every guard byte must still be 0x5A (a partial workgroup's idle lanes are where a store
past the last env would come from).
"""
import pytest

import step_instantiations as S
import step_plan_table as T
from libzombsole_amd import _abi
from step_runner import Band, GuardedStep, run_engines  # noqa: F401

pytestmark = pytest.mark.gpu


ALL_ROWS = S.ROWS + S.SMALL_ROWS


def plan_describe(row):
    """The describe() fields that the step plan decides, from the plan's table row of the row's config and overrides
    (test_step_plan.py and test_step_instantiations_plan.py hold the compiled plan to that row on the CPU)."""
    p = T.expected("row:" + row.id, row.launch)
    return {"step_lds": p["lds"], "step_wgs_per_cu": p["resident"], "rng_window": p["rw_cap"], "rng_step": p["rw_step"],
            "reset_lds": p["reset_lds"], "reset_side_stream": p["side_stream"]}


@pytest.mark.parametrize("row", ALL_ROWS, ids=[r.id for r in ALL_ROWS])
def test_instantiation(row):
    """One instantiation, with the lanes' execution (par_exec 1) and with the leader's serial loop (par_exec -1):
    describe() names the requested lanes per env, the kernel and its wave budget, and the LDS sizes, resident
    workgroups, RNG window and side stream of the step plan's row; 24 steps of episodes of five,
    every env of both engines against the oracle at every step, the state at steps 12 and 24."""
    pars = (1, -1)
    resets, _ = run_engines([row.builder(par_exec=p) for p in pars], row.make, row.seeds(), S.STEPS, row,
                            states_at=(S.STEPS // 2, S.STEPS),
                            expect=[dict(row.describe(p), **plan_describe(row)) for p in pars])
    assert sum(resets) >= 4 * row.n  # every env went through four autoresets or more


@pytest.mark.parametrize("lanes", [3, 6, 48, 65, 128, -1])
def test_bad_lanes_per_env_is_refused(lanes):
    """zs_create refuses a lanes_per_env that no step kernel is compiled for (it used to size the launch for
    64 / G envs per workgroup and run the G = 64 kernel, leaving most envs unstepped): ValueError naming the
    field, and no handle.  Nothing is stepped here."""
    from libzombsole_amd.engine import Engine
    b = S.c2(8)
    b.cfg.lanes_per_env = lanes
    with pytest.raises(ValueError, match="lanes_per_env"):
        Engine(b)


# -- work-list loops ---------------------------------------------------------------------------------------------
class Stream(object):
    """The action stream of a work-list case (Row.actions without a table row)."""

    def __init__(self, stream):
        self.stream = stream

    actions = S.Row.actions


def c2_short(n):
    """C2 with episodes of four steps: every env is pending at the same steps."""
    return _abi.multi_env_config(n, "extermination", [], "bridge64", ["0", "1"], initial_zombies=10,
                                 minimum_zombies=0, max_episode_steps=4)


def mixed_reset(n):
    """Consecutive resets leave different things in the reset image: random weapons (a draw per agent), a bot,
    and a zombie spawn list of every free cell of the map (city_for_safehouse lists none), whose candidate list
    changes with every env's player positions."""
    return _abi.multi_env_config(n, "extermination", ["terminator"], "city_for_safehouse", ["0", "1"],
                                 initial_zombies=6, minimum_zombies=0, agent_weapons="random", max_episode_steps=3)


RESET_LOOPS = {
    # the reset role of a fused k_step over 1 and 3 workgroups
    "fused_wgs1": ({"fused": 1, "reset_wgs": 1}, 1, "k_step", 0),
    "fused_wgs3": ({"fused": 1, "reset_wgs": 3}, 3, "k_step", 0),
    # k_reset in list mode over 1 and 3 workgroups, on the side stream and on the caller's
    "k_reset_grid1_side": ({"fused": -1, "reset_grid": 1}, 1, "k_tick", 1),
    "k_reset_grid3_side": ({"fused": -1, "reset_grid": 3}, 3, "k_tick", 1),
    "k_reset_grid1_serial": ({"fused": -1, "reset_grid": 1, "reset_stream": -1}, 1, "k_tick", 0),
    "k_reset_grid3_serial": ({"fused": -1, "reset_grid": 3, "reset_stream": -1}, 3, "k_tick", 0),
    # ... reading the spawn lists from HBM instead of its LDS copy
    "k_reset_grid3_hbm_lists": ({"fused": -1, "reset_grid": 3, "reset_lists": -1}, 3, "k_tick", 1),
}


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("path", sorted(RESET_LOOPS))
def test_reset_loop(path, graph):
    """37 C2 envs with episodes of four steps: all 37 are pending at once, and the reset work has 1 or 3
    workgroups, so every workgroup rebuilds 12 envs or more through one LDS image in one launch (reset_role's
    grid-stride loop).  The oracle's count of envs reset at a step states it: 37 > 3.  Eager launches and the
    replayed step graphs (both pending-list parities: resets fall on odd and on even steps)."""
    launch, wgs, kernel, side = RESET_LOOPS[path]
    n, steps = 37, 21
    b = c2_short(n).set_launch(dict(launch, fobs=-1))
    expect = {"envs": n, "step_kernel": kernel, "reset_side_stream": side, "respawn": "tick"}
    resets, _ = run_engines([b], c2_short, [300 + i for i in range(n)], steps, Stream("discrete"), graph=graph,
                            states_at=(10, steps), expect=[expect])
    assert max(resets) == n > wgs  # one launch rebuilt more envs than it had workgroups
    assert {t % 2 for t in range(steps + 1) if resets[t] == n} == {0, 1}


@pytest.mark.parametrize("path", ["fused_wgs1", "k_reset_grid1_side", "k_reset_grid3_hbm_lists"])
def test_reset_loop_stale_lds(path):
    """13 envs whose consecutive resets differ in what they leave in the image (mixed_reset), episodes of three
    steps, one or three workgroups for all of them."""
    launch, wgs, kernel, side = RESET_LOOPS[path]
    n, steps = 13, 20
    b = mixed_reset(n).set_launch(dict(launch, fobs=-1))
    expect = {"envs": n, "step_kernel": kernel, "reset_side_stream": side}
    resets, _ = run_engines([b], mixed_reset, [500 + i for i in range(n)], steps, Stream("rich"),
                            states_at=(steps,), expect=[expect])
    assert max(resets) == n > wgs


def boxed(n):
    """The one-zombie extermination config of test_respawn_paths, as a multi-agent env."""
    return _abi.multi_env_config(n, "extermination", ["terminator"], "boxed", ["0"], initial_zombies=1,
                                 minimum_zombies=1, agent_weapons="shotgun", max_episode_steps=60)


def c4_long(n):
    """city128, 4 agents, 50 zombies kept at 50, episodes without a time limit: the agents' rifles kill often."""
    return _abi.multi_env_config(n, "safehouse", [], "city128", ["0", "1", "2", "3"], initial_zombies=50,
                                 minimum_zombies=50)


# config -> (builder, envs, steps, action stream, first seed).  The seeds and step counts are chosen so that the
# oracle alone shows a step at which more envs respawn than the larger grid has workgroups (four of the nine
# city128 envs at step 31; five or more of the 37 boxed envs at every step but the first).
RESPAWN_LOOPS = {"c4": (c4_long, 9, 32, "discrete", 1800), "boxed": (boxed, 37, 24, "rich", 800)}


@pytest.mark.parametrize("fused", [1, -1], ids=["fused", "unfused"])
@pytest.mark.parametrize("grid", [1, 3])
@pytest.mark.parametrize("config", sorted(RESPAWN_LOOPS))
def test_respawn_loop(config, grid, fused):
    """k_respawn over 1 or 3 workgroups: city128 with 50 zombies kept at 50 (9 envs) and the boxed one-zombie
    config (37 envs), fused and unfused step launches.  The oracle's count of envs that respawned at one step is
    larger than the grid at some step: a workgroup placed zombies in two envs or more through one image."""
    make, n, steps, stream, seed0 = RESPAWN_LOOPS[config]
    b = make(n).set_launch({"defer_respawn": 1, "respawn_grid": grid, "fused": fused, "fobs": -1})
    expect = {"envs": n, "respawn": "k_respawn", "step_kernel": "k_step" if fused > 0 else "k_tick",
              "reset_side_stream": 1 if fused < 0 else 0}
    _, respawns = run_engines([b], make, [seed0 + i for i in range(n)], steps, Stream(stream),
                              states_at=(steps // 2, steps), expect=[expect])
    assert max(respawns) > grid, respawns
