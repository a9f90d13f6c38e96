"""Seeds of 2**32 and above: random.seed(int) keys MT19937 with abs(n) in 32-bit little-endian words, two of them
from 2**32 on.  Both the oracle's mt_seed (oracle/zs_oracle.c) and the engine's k_seed (csrc/k_state.hip) take
that branch; every other test seeds below 2**16."""
import random

import numpy as np
import pytest

from libzombsole_amd import _abi

SEEDS = [0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 63, 2 ** 64 - 1]
# WeaponFactory.create_player_weapon's choice([Knife(), Axe(), Gun(), Rifle(), Shotgun()]) (weapons.py:28-45)
WEAPONS = ["knife", "axe", "gun", "rifle", "shotgun"]
ZOMBIES = 6


def _builder():
    return _abi.multi_env_config(1, "extermination", [], "bridge64", ["0", "1", "2", "3"], initial_zombies=ZOMBIES,
                                 minimum_zombies=0, agent_weapons="random")


def _expected_reset(seed, m):
    """Game.__initialize_world__ (game.py:141-187) drawn from CPython's own generator: the agents' random
    weapons, World.spawn_in_random (core.py:40-66: shuffle the free spawn cells, pop from the end) for the
    players (none here: the shuffle alone) and the agents, then Zombie() lives (randint(50, 100)) and the
    zombies' spawn_in_random.  bridge64's spawn cells are free of obstacles."""
    rnd = random.Random()
    rnd.seed(seed)
    weapons = [_abi.weapon_id(WEAPONS[rnd.randrange(5)]) for _ in range(4)]
    cand = list(m.player_spawns)
    rnd.shuffle(cand)
    cand = list(m.player_spawns)
    rnd.shuffle(cand)
    agents = [cand.pop() for _ in range(4)]
    lives = [rnd.randint(50, 100) for _ in range(ZOMBIES)]
    cand = [c for c in m.zombie_spawns if c not in agents]
    rnd.shuffle(cand)
    zombies = [cand.pop() for _ in range(ZOMBIES)]
    return ([[x, y, 100, w] for (x, y), w in zip(agents, weapons)],
            [[x, y, life] for (x, y), life in zip(zombies, lives)])


@pytest.mark.parametrize("seed", SEEDS)
def test_oracle_seed_is_cpythons(seed):
    """The oracle's first draws after seed(s) (a reset's: about 480 of them) are random.seed(s)'s stream."""
    from oracle.oracle import OracleEnv
    b = _builder()
    obstacles = {(x, y) for x, y, _ in b.map.obstacles}
    assert not obstacles & (set(b.map.player_spawns) | set(b.map.zombie_spawns))
    o = OracleEnv(b)
    o.seed(seed)
    o.reset()
    st = o.state()
    agents, zombies = _expected_reset(seed, b.map)
    assert st["agents"] == agents
    assert [[r[1], r[2], r[3]] for r in st["dyn"] if r[0] == _abi.THING_ZOMBIE] == zombies


def test_oracle_seeds_differ():
    """The high word is part of the key: 2**32 and 2**32 + 1 are neither 0's nor 1's stream."""
    from oracle.oracle import OracleEnv
    states = []
    for s in SEEDS:
        o = OracleEnv(_builder())
        o.seed(s)
        o.reset()
        states.append(str(o.state()))
    assert len(set(states)) == len(SEEDS)


@pytest.mark.gpu
def test_engine_seed_is_cpythons():
    """eng.seed(s) leaves the env's stream where random.seed(s) leaves CPython's.  zs_get_rng's record is in
    getstate() form, but k_seed has already made the first twist (index 0 of the twisted block) where CPython
    holds index 624 of the block before it: the same point of the same stream, so the record is loaded into a
    random.Random and the two are compared by their draws (two twists' worth) and then by their states, which
    are equal word for word once both have twisted."""
    from libzombsole_amd.engine import Engine
    eng = Engine(_abi.multi_env_config(len(SEEDS), "extermination", [], "bridge64", ["0", "1", "2", "3"],
                                       initial_zombies=ZOMBIES, minimum_zombies=0, agent_weapons="random"))
    eng.seed(SEEDS)
    for e, s in enumerate(SEEDS):
        want, got = random.Random(), random.Random()
        want.seed(s)
        rec = eng.get_rng(e)
        assert int(rec[624]) in (0, 624), (e, s, int(rec[624]))  # nothing drawn yet
        got.setstate((3, tuple(int(v) for v in rec), None))
        assert [got.getrandbits(32) for _ in range(1300)] == [want.getrandbits(32) for _ in range(1300)], (e, s)
        assert got.getstate() == want.getstate(), (e, s)
    eng.close()
