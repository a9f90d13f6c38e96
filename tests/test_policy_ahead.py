"""The step graph's policy kept one step ahead (zs_step_graph on an unfused, side-stream step that ends in k_obs_ring
or k_obs_pbring): the observation kernel of step t leaves step t + 1's triples in the handle's own rows with a stamp,
and step t + 1's tick copies them out instead of a policy launch (csrc/zs_device.hpp policy_ahead, GS_*).

Every case runs the graphed engine beside a second handle with the same seeds that takes the eager path
(zs_gen_actions(t), zs_step) and compares, bit for bit, after every call: the caller's action buffer, observations,
rewards, done, truncated, listed, was_reset; and at the end the state record of every env.  A TimeLimit of 7 steps
keeps autoresets (the side-stream reset work) in every run.

The shapes: C3's (bridge64, 2 agents + 10 zombies, int64) at 5 envs (fewer than the encoder waves: waves
without an item still produce), 64, 70 and 600 (workgroups of two and three envs), forced onto k_tick + k_obs_ring by
launch overrides; C4's (city128, k_obs_pbring) at 6.
"""
import numpy as np
import pytest

from libzombsole_amd import _abi

pytestmark = pytest.mark.gpu

STEPS = 30
RING = {"fused": -1, "fobs": -1, "obs_lds": 1, "obs_ring": 1}
PBRING = {"fused": -1, "fobs": -1}


def c3(n):
    return _abi.multi_env_config(n, "extermination", [], "bridge64", ["0", "1"], initial_zombies=10,
                                 minimum_zombies=0, max_episode_steps=7)


def c4(n):
    return _abi.multi_env_config(n, "safehouse", [], "city128", ["0", "1", "2", "3"], initial_zombies=50,
                                 minimum_zombies=50, max_episode_steps=7)


# name -> (config, envs, launch overrides, describe()'s obs_kernel)
SHAPES = {"c3@5": (c3, 5, RING, "k_obs_ring"), "c3@64": (c3, 64, RING, "k_obs_ring"),
          "c3@70": (c3, 70, RING, "k_obs_ring"), "c3@600": (c3, 600, RING, "k_obs_ring"),
          "c4@6": (c4, 6, PBRING, "k_obs_pbring")}
C3_SMALL = ["c3@5", "c3@64", "c3@70"]
ALL = C3_SMALL + ["c4@6"]


class Pair(object):
    """The graphed engine `g` and its eager twin `e`, driven alike; `t` is the policy's next step number."""

    def __init__(self, shape, t0=1, seed0=500):
        from libzombsole_amd.engine import Engine
        make, n, launch, self.obs_kernel = SHAPES[shape]
        self.g, self.e = Engine(make(n).set_launch(launch)), Engine(make(n).set_launch(launch))
        self.n, self.t, self.calls, self.resets = n, t0, 0, 0
        d = self.g.describe()
        assert (d["step_kernel"], d["obs_kernel"], d["reset_side_stream"]) == ("k_tick", self.obs_kernel, 1), d
        self.seed(seed0)
        for x in (self.g, self.e):
            x.reset()
        self.same("reset", outputs=False)

    def seed(self, seed0):
        for x in (self.g, self.e):
            x.seed([seed0 + 3 * i for i in range(self.n)])

    def same(self, what, outputs=True):
        import torch
        g, e = self.g, self.e
        fields = [("obs", g.obs, e.obs)]
        if outputs:
            fields += [("actions", g.actions, e.actions), ("rewards", g.rewards.view(torch.int64), e.rewards.view(torch.int64)),
                       ("done", g.done, e.done), ("truncated", g.trunc, e.trunc), ("listed", g.listed, e.listed),
                       ("was_reset", g.was_reset, e.was_reset)]
        for name, a, b in fields:
            assert torch.equal(a, b), (what, self.calls, self.t, name)
        if outputs:
            self.resets += int(g.was_reset.sum())

    def replay(self, nd=7, steps=1):
        """One graph launch of `steps` policy steps; the twin generates and steps eagerly."""
        self.g.step_graph(self.t, nd, steps=steps)
        for k in range(steps):
            self.e.gen_actions(self.t + k, nd)
            self.e.step()
        self.t += steps
        self.calls += 1
        d = self.g.describe()
        assert (d["step_policy"], d["step_tail_launch"]) == ("ahead", self.obs_kernel), d  # no policy launch in the graph
        self.same("replay")

    def eager(self, acts):
        """An eager step of both on the caller's own triples, written into the graph's action tensor."""
        for x in (self.g, self.e):
            x.actions.copy_(acts)
            x.step()
        self.calls += 1
        self.same("eager")

    def finish(self):
        for k in range(self.n):
            assert np.array_equal(self.g.get_state(k).buf, self.e.get_state(k).buf), ("state", k)
        assert self.resets >= self.n  # the TimeLimit's autoresets were in the run
        self.g.close()
        self.e.close()


def own_actions(p, salt):
    """A caller's triples: the policy's stream of another step number and table."""
    return p.e.gen_actions(1000 + salt, 5).clone()


# 1, 8: plain replays; the stamp starts invalid (the first replay generates in the tick), at step0 = 1 and at a large one
@pytest.mark.parametrize("shape,t0", [(s, 1) for s in ALL + ["c3@600"]] + [(s, (1 << 40) + 12345) for s in ALL])
def test_plain_replays(shape, t0):
    p = Pair(shape, t0=t0)
    for _ in range(STEPS):
        p.replay()
    p.finish()


# 2: an eager zs_step on the caller's own actions between replays: the rows kept ahead are still the next policy step's
@pytest.mark.parametrize("shape", ALL)
def test_eager_step_between_replays(shape):
    p = Pair(shape)
    for k in range(STEPS):
        p.replay()
        if k % 5 == 2:
            p.eager(own_actions(p, k))
        if k == 11:  # two in a row (both pending-list parities)
            p.eager(own_actions(p, 100))
            p.eager(own_actions(p, 101))
    p.finish()


# 3: the caller overwrites its action buffer between replays: the tick reads the handle's own rows
@pytest.mark.parametrize("shape", ALL)
def test_caller_garbage_in_actions(shape):
    import torch
    p = Pair(shape)
    gen = torch.Generator(device="cpu").manual_seed(3)
    for _ in range(STEPS):
        junk = torch.randint(-2 ** 31, 2 ** 31 - 1, tuple(p.g.actions.shape), generator=gen, dtype=torch.int64)
        p.g.actions.copy_(junk.to(torch.int32))
        p.replay()
    p.finish()


# 4: zs_seed between replays: the next step generates from the new seeds in the tick, the one after reads ahead again
@pytest.mark.parametrize("shape", ALL)
def test_seed_between_replays(shape):
    p = Pair(shape)
    for k in range(STEPS):
        if k in (4, 5, 17):
            p.seed(9000 + 100 * k)
        p.replay()
    p.g.seed([77], env0=p.n - 1)  # one env's seed alone invalidates as well
    p.e.seed([77], env0=p.n - 1)
    for _ in range(3):
        p.replay()
    p.finish()


# 5: two graph sets that differ in n_discrete on the same buffers: neither reads the other's rows
@pytest.mark.parametrize("shape", ALL)
def test_alternating_n_discrete(shape):
    p = Pair(shape)
    for k in range(STEPS):
        p.replay(nd=7 if (k // 2) % 2 == 0 else 5)  # 7 7 5 5 7 7 ...: a set follows itself and the other one
    for k in range(6):
        p.replay(nd=7 if k % 2 == 0 else 5)
    p.finish()


# 6: three steps per graph launch: every captured step produces and consumes
@pytest.mark.parametrize("shape", ALL)
def test_three_steps_per_launch(shape):
    p = Pair(shape)
    for _ in range(STEPS // 3):
        p.replay(steps=3)
    p.replay(steps=1)  # another set continues from the counter and the rows the last launch left
    p.replay(steps=3)
    p.finish()


# 7: zs_reset of a masked subset between replays
@pytest.mark.parametrize("shape", ALL)
def test_masked_reset_between_replays(shape):
    import torch
    p = Pair(shape)
    mask = (torch.arange(p.n, device=p.g.device) % 3 == 1).to(torch.uint8)
    for k in range(STEPS):
        if k % 6 == 4:
            for x in (p.g, p.e):
                x.reset(mask)
            p.same("masked reset", outputs=False)
        p.replay()
    p.finish()
