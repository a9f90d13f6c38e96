"""The oracle takes and returns a stream state (zo_set_rng / zo_get_rng, random.setstate() / getstate() form: the
raw 624-word block and the index 0..624 of its next word), so that a test can start it anywhere in a block.

Streams are compared as streams (stream_util.py).
"""
import random

import numpy as np
import pytest

from libzombsole_amd import _abi
from stream_util import WORDS, at_index, record, stream_words


def _builder(zombies=6):
    return _abi.multi_env_config(1, "extermination", ["hamster"], "bridge64", ["0", "1"], initial_zombies=zombies,
                                 minimum_zombies=0, agent_weapons="random")


def oracle_words(o, n=WORDS):
    """The stream zo_get_rng's record holds (nothing consumed)."""
    return stream_words(o.get_rng(), n)


@pytest.mark.parametrize("index,blocks", [(0, 0), (1, 0), (623, 0), (624, 0), (311, 5)],
                         ids=["i0", "i1", "i623", "i624", "block5"])
def test_set_rng_is_setstate(index, blocks):
    """setstate into random.Random and zo_set_rng give the same next 1 300 words, drawn by the oracle's own
    generator (zo_rng_words: two twists or more); the record reads straight back; after the draws the oracle's
    record is the stream 1 300 words on; and a reset from the set state leaves the stream its draws on."""
    from oracle.oracle import OracleEnv
    rec = at_index(1234 + index, index, blocks)
    want = stream_words(rec, 2 * WORDS)
    o = OracleEnv(_builder())
    o.seed(99)
    o.set_rng(rec)
    assert np.array_equal(o.get_rng(), rec)
    assert oracle_words(o) == want[:WORDS]
    d0 = o.rng_draws()
    assert o.rng_words(WORDS) == want[:WORDS]
    assert o.rng_draws() == d0 + WORDS
    assert oracle_words(o, WORDS) == want[WORDS:]
    o.set_rng(rec)
    o.reset()
    d = o.rng_draws() - d0 - WORDS
    assert 0 < d < WORDS
    assert oracle_words(o) == want[d:d + WORDS]


def test_set_rng_refuses_a_bad_index():
    from oracle.oracle import OracleEnv
    o = OracleEnv(_builder())
    o.seed(5)
    before = o.get_rng().copy()
    rec = at_index(1, 0)
    rec[624] = 625
    with pytest.raises(ValueError):
        o.set_rng(rec)
    assert np.array_equal(o.get_rng(), before)


def test_draw_count_runs_on_over_a_set():
    """zo_rng_draws keeps counting from the moment of the set."""
    from oracle.oracle import OracleEnv
    o = OracleEnv(_builder())
    o.seed(5)
    o.reset()
    d1 = o.rng_draws()
    assert d1 > 0
    o.set_rng(at_index(8, 17))
    assert o.rng_draws() == d1
    o.reset()
    assert o.rng_draws() > d1


@pytest.mark.parametrize("seed", [0, 7, 2 ** 32 + 1])
def test_get_rng_after_a_reset_is_the_seeded_stream(seed):
    """zo_get_rng after zo_seed + zo_reset loads into random.Random as random.seed(seed)'s stream, the reset's
    draws on."""
    from oracle.oracle import OracleEnv
    o = OracleEnv(_builder())
    o.seed(seed)
    o.reset()
    d = o.rng_draws()
    r = random.Random()
    r.seed(seed)
    for _ in range(d):
        r.getrandbits(32)
    assert oracle_words(o) == [r.getrandbits(32) for _ in range(WORDS)]


def test_set_rng_equals_seed():
    """An env started from random.seed(s)'s getstate() runs as one started with zo_seed(s): observations,
    rewards and state over 30 steps with respawns."""
    from oracle.oracle import OracleEnv
    b = lambda: _abi.multi_env_config(1, "extermination", ["randoman"], "boxed", ["0"], initial_zombies=2,  # noqa: E731
                                      minimum_zombies=2, agent_weapons="random", max_episode_steps=0)
    a, c = OracleEnv(b()), OracleEnv(b())
    a.seed(31)
    r = random.Random()
    r.seed(31)
    c.seed(1)
    c.set_rng(record(r))
    assert np.array_equal(a.reset(), c.reset())
    for t in range(30):
        act = [[3, 0, 0]]
        ra, rc = a.step(act), c.step(act)
        assert np.array_equal(ra[0], rc[0]) and np.array_equal(ra[1], rc[1]) and ra[2:4] == rc[2:4]
        if ra[2] or ra[3]:
            break
    assert a.state() == c.state()
    assert oracle_words(a) == oracle_words(c)
