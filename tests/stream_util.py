"""MT19937 stream records for the tests (random.getstate() form: the raw 624-word block, then the index 0..624 of
its next word).  Streams are compared as streams: two records of one point of one stream need not be equal word
for word (index 624 of a block is index 0 of the next one, see test_seed64.py), so a record is loaded into a
random.Random and its next 1 300 getrandbits(32) taken, two blocks' worth."""
import random

import numpy as np

WORDS = 1300


def stream_words(rec, n=WORDS):
    """The next n getrandbits(32) of the stream a 625-word record holds."""
    r = random.Random()
    r.setstate((3, tuple(int(v) for v in rec), None))
    return [r.getrandbits(32) for _ in range(n)]


def record(rnd):
    """random.getstate() of `rnd` as 625 uint32 words."""
    return np.asarray(rnd.getstate()[1], dtype=np.uint64).astype(np.uint32)


def at_index(seed, index, blocks=0):
    """A record with the given index: random.Random(seed) advanced `blocks` whole blocks (a draw first, so that
    the block is a twisted one), its index then set to `index`."""
    r = random.Random(seed)
    r.getrandbits(32)
    for _ in range(624 * blocks):
        r.getrandbits(32)
    rec = record(r)
    rec[624] = index
    return rec


def same_stream(a, b, words=WORDS):
    """Two records hold the same point of the same stream: equal word for word, or equal in their next `words`
    words."""
    return bool(np.array_equal(a, b)) or stream_words(a, words) == stream_words(b, words)
