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
import numpy as np
import pytest

import step_instantiations as S
import step_plan_table as T
from libzombsole_amd import _abi
from test_obs_instantiations import FILL, GUARD

pytestmark = pytest.mark.gpu


class Band(object):
    """A tensor of `shape` and `dtype` at byte GUARD of a 0x5A-filled byte tensor with GUARD bytes after it."""

    def __init__(self, eng, shape, dtype):
        torch = eng.torch
        self.nbytes = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        self.raw = torch.full((GUARD + self.nbytes + GUARD,), FILL, dtype=torch.uint8, device=eng.device)
        assert self.raw.data_ptr() % 16 == 0 and GUARD >= 64 and GUARD % 8 == 0
        self.view = self.raw[GUARD:GUARD + self.nbytes].view(dtype).view(shape)
        assert self.view.data_ptr() == self.raw.data_ptr() + GUARD

    def guards_hold(self):
        raw = self.raw.cpu().numpy()
        return bool((raw[:GUARD] == FILL).all() and (raw[GUARD + self.nbytes:] == FILL).all())


class GuardedStep(object):
    """The output set of Engine.step / step_graph (obs, rewards, done, trunc, listed, was_reset) and the action
    tensor, each but the observations (test_obs_instantiations.py guards those) inside its own Band."""
    FLAGS = ("done", "trunc", "listed", "was_reset")

    def __init__(self, eng):
        torch = eng.torch
        n, a = eng.N, eng.A
        self.bands = {"rewards": Band(eng, (n, a if eng.multi else 1), torch.float64),
                      "done": Band(eng, (n,), torch.uint8), "trunc": Band(eng, (n,), torch.uint8),
                      "listed": Band(eng, (n, a), torch.uint8), "was_reset": Band(eng, (n,), torch.uint8),
                      "actions": Band(eng, (n, a, 3), torch.int32)}
        for k, b in self.bands.items():
            setattr(self, k, b.view)
        self.obs = eng.obs

    def clear(self):
        """0x5A over every output payload (not the actions, which the step reads)."""
        for k, b in self.bands.items():
            if k != "actions":
                b.raw.fill_(FILL)

    def check(self, what):
        for k, b in self.bands.items():
            assert b.guards_hold(), ("guard bytes written", k, what)
        for k in self.FLAGS:  # every env's flags were stored
            v = getattr(self, k).cpu().numpy()
            assert (v != FILL).all(), ("flag bytes never written", k, what, np.argwhere(v == FILL)[:8].tolist())


def run_engines(builders, make_oracle, seeds, steps, stream_row, graph=False, states_at=(), expect=None):
    """One engine per builder (the same config and seeds under different launch overrides), stepped in lock step
    and each compared with one OracleEnv per env at every step: the reset observation; observations, rewards
    (bit-exact, the listed ones), done, truncated, the autoreset flag and `listed`; the canonical state of every
    env at the steps `states_at`.  expect: per builder, the describe() fields it must report.  Returns per step
    (1-based; index 0 unused) the number of envs the oracle reset and the number it respawned zombies in."""
    import torch
    from libzombsole_amd.engine import Engine
    from oracle.oracle import OracleEnv

    n = len(seeds)
    engs, outs = [], []
    for i, b in enumerate(builders):
        eng = Engine(b)
        if expect:
            desc = eng.describe()
            assert {k: desc[k] for k in expect[i]} == expect[i], (i, desc)
        eng.seed(seeds)
        engs.append(eng)
        outs.append(GuardedStep(eng))
    kinds = [o[2] for o in engs[0].builder.map.obstacles]
    A = engs[0].A
    refs = []
    obs0 = [eng.reset().cpu().numpy() for eng in engs]
    for k, s in enumerate(seeds):
        o = OracleEnv(make_oracle(1))
        o.seed(s)
        exp = o.reset()
        for i in range(len(engs)):
            assert np.array_equal(obs0[i][k], exp), ("reset obs", i, k)
        refs.append(o)
    need = [False] * n
    resets, respawns, respawned = [0] * (steps + 1), [0] * (steps + 1), [0] * n
    for t in range(1, steps + 1):
        got = []
        for i, (eng, out) in enumerate(zip(engs, outs)):
            out.clear()
            if graph:  # the policy's actions are generated inside the replayed graph, into the guarded tensor
                eng.step_graph(t, 7, out=out, actions=out.actions)
            else:
                if stream_row.stream == "discrete":
                    eng.gen_actions(t, 7, out=out.actions)
                else:
                    out.actions.copy_(torch.from_numpy(stream_row.actions(seeds, t, A)))
                eng.step(actions=out.actions, out=out)
            torch.cuda.synchronize()
            out.check((i, t))
            got.append({k: getattr(out, k).cpu().numpy() for k in
                        ("obs", "rewards", "done", "trunc", "listed", "was_reset", "actions")})
        acts = got[0]["actions"]
        for g in got[1:]:
            assert np.array_equal(g["actions"], acts)
        if stream_row.stream == "discrete":  # zs_gen_actions' stream is the oracle's (run_hashes, the CPU census)
            assert np.array_equal(acts[::max(1, n // 3)], stream_row.actions(seeds[::max(1, n // 3)], t, A))
        for k, o in enumerate(refs):
            if need[k]:
                exp, r, d, tr, lb = o.reset(), None, False, False, np.ones(A, bool)
                need[k] = False
                resets[t] += 1
            else:
                exp, r, d, tr, lb = o.step(acts[k])
                need[k] = d or tr
                c = o.census()["respawns"]
                respawns[t] += c != respawned[k]
                respawned[k] = c
            for i, g in enumerate(got):
                assert bool(g["was_reset"][k]) == (r is None), ("autoreset flag", i, k, t)
                assert bool(g["done"][k]) == d and bool(g["trunc"][k]) == tr, ("flags", i, k, t)
                assert np.array_equal(g["listed"][k].astype(bool), lb), ("listed", i, k, t)
                if r is None:
                    assert not g["rewards"][k].any(), ("rewards of a reset", i, k, t)
                else:
                    assert np.array_equal(g["rewards"][k][lb].view(np.uint64), r[:A][lb].view(np.uint64)), \
                        ("rew", i, k, t, g["rewards"][k], r)
                assert np.array_equal(g["obs"][k], exp), ("obs", i, k, t)
        if t in states_at:
            for i, eng in enumerate(engs):
                for k, o in enumerate(refs):
                    assert eng.get_state(k).canonical(kinds) == o.state(), ("state", i, k, t)
    for eng in engs:
        eng.close()
    return resets, respawns


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
