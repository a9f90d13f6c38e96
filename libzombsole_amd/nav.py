"""Path-distance fields in numpy: the second statement of their rules (the first is csrc/zs_nav.hpp).

    field(state, static, which, max_dist)   -> uint16 [H, W]      (UNREACHED = 0xFFFF)
    encode(state, static, fields, max_dist) -> int16  [A, F, 8]

A cell is free when it is inside the map and holds no present obstacle, whatever the obstacle's life; entities never
block.  A field is the 4-connected breadth-first distance over free cells from its source cells, in moves; a source
cell that is not free is not a source.  OBJECTIVE (bit 0): the map's objective cells.  ZOMBIES (bit 1): the cells of
the present zombie slots (s >= A + P).  `fields` is a bitmask of the two (or their names), F its popcount, the fields
in ascending bit order.  The search stops after max_dist (1..MAX_DIST) levels; a cell not reached by then is
unreachable, as blocked cells and cells outside the map are.

A row, in int16 words: 0 the distance at the agent's cell; 1..4 the distances at the cells the moves DIRS lead to, -1
where unreachable, blocked or outside the map; 5 the smallest k whose neighbour distance is the minimum over the
reachable neighbours, 6 the smallest k at their maximum (both -1 when no neighbour is reachable); 7 flags: PRESENT,
ON_SOURCE (the agent's own cell is a source).  An agent that is not present has an all-zero row.

`state` is an engine.StateView (Engine.get_state) or anything with its fields: `ent` [E][>= 4] rows of (kind, present,
x, y, ...), slots agents [0, A), bots [A, A + P), zombies after them; `obst_present` [O]; `A`; `P`.  `static` is an
entity_obs.Static: the map's size, obstacle cells and objective cells in map-file order.

A shaping potential is -rows[..., f, 0] where it is >= 0; a greedy path follower takes move rows[..., f, 5].
"""
import numpy as np

from .entity_obs import Static  # noqa: F401  (what `static` is)

OBJECTIVE, ZOMBIES = 1, 2
FIELD_NAMES = {"objective": OBJECTIVE, "zombies": ZOMBIES}
MAX_DIST = 32766
UNREACHED = 0xFFFF
ROW_WORDS = 8
PRESENT, ON_SOURCE = 1, 2
DIRS = ((0, 1), (-1, 0), (0, -1), (1, 0))


def fields_mask(fields):
    """A bitmask, a field's name, or a sequence of names as the bitmask; ValueError for anything else."""
    if isinstance(fields, str):
        fields = (fields,)
    if isinstance(fields, (tuple, list, set, frozenset)):
        try:
            m = 0
            for f in fields:
                m |= FIELD_NAMES[f]
        except (KeyError, TypeError):
            raise ValueError("path distances: fields are 'objective' and 'zombies'") from None
        fields = m
    fields = int(fields)
    if not 1 <= fields <= (OBJECTIVE | ZOMBIES):
        raise ValueError("path distances: fields must be a non-empty mask of OBJECTIVE | ZOMBIES")
    return fields


def field_bits(fields):
    """The single-field masks of `fields`, in the order they are emitted."""
    fields = fields_mask(fields)
    return [b for b in (OBJECTIVE, ZOMBIES) if fields & b]


def _check_max_dist(max_dist):
    if not 1 <= int(max_dist) <= MAX_DIST:
        raise ValueError("path distances: max_dist must be in 1..%d" % MAX_DIST)
    return int(max_dist)


def free_cells(state, static):
    """bool [H, W]: the cells that hold no present obstacle."""
    free = np.ones((static.H, static.W), dtype=bool)
    for i, (x, y) in enumerate(static.obstacles):
        if int(state.obst_present[i]):
            free[y, x] = False
    return free


def sources(state, static, which):
    """bool [H, W]: the source cells of the one field `which`, free or not."""
    src = np.zeros((static.H, static.W), dtype=bool)
    if which == OBJECTIVE:
        cells = static.objectives
    else:
        first = int(state.A) + int(state.P)
        cells = [(int(e[2]), int(e[3])) for e in list(state.ent)[first:] if int(e[1])]
    for x, y in cells:
        if 0 <= x < static.W and 0 <= y < static.H:
            src[y, x] = True
    return src


def field(state, static, which, max_dist=MAX_DIST):
    """The full field of the one field `which` (a mask with one bit, or its name), level by level on boolean arrays."""
    which = fields_mask(which)
    if which not in (OBJECTIVE, ZOMBIES):
        raise ValueError("path distances: field must be OBJECTIVE or ZOMBIES")
    max_dist = _check_max_dist(max_dist)
    free = free_cells(state, static)
    frontier = sources(state, static, which) & free
    visited = frontier.copy()
    out = np.full((static.H, static.W), UNREACHED, dtype=np.uint16)
    out[frontier] = 0
    level = 0
    while frontier.any() and level < max_dist:
        level += 1
        grown = np.zeros_like(frontier)
        grown[1:, :] |= frontier[:-1, :]
        grown[:-1, :] |= frontier[1:, :]
        grown[:, 1:] |= frontier[:, :-1]
        grown[:, :-1] |= frontier[:, 1:]
        frontier = grown & free & ~visited
        visited |= frontier
        out[frontier] = level
    return out


def row(dist, present, x, y):
    """The eight words of one agent's row from the full field `dist`."""
    if not present:
        return [0] * ROW_WORDS
    H, W = dist.shape

    def at(cx, cy):
        if not (0 <= cx < W and 0 <= cy < H) or dist[cy, cx] == UNREACHED:
            return -1
        return int(dist[cy, cx])

    d0 = at(x, y)
    d = [at(x + dx, y + dy) for dx, dy in DIRS]
    reach = [v for v in d if v >= 0]
    lo = d.index(min(reach)) if reach else -1
    hi = d.index(max(reach)) if reach else -1
    return [d0] + d + [lo, hi, PRESENT | (ON_SOURCE if d0 == 0 else 0)]


def encode(state, static, fields, max_dist=MAX_DIST):
    bits = field_bits(fields)
    A = int(state.A)
    out = np.zeros((A, len(bits), ROW_WORDS), dtype=np.int16)
    for f, b in enumerate(bits):
        dist = field(state, static, b, max_dist)
        for a in range(A):
            e = state.ent[a]
            out[a, f] = row(dist, int(e[1]), int(e[2]), int(e[3]))
    return out


def levels(state, static, which, max_dist=MAX_DIST):
    """The number of levels a full search of the field runs: its largest finite distance (0 with no reachable cell)."""
    d = field(state, static, which, max_dist)
    r = d[d != UNREACHED]
    return int(r.max()) if r.size else 0
