"""The envs' picture on the host: the default sprite atlas and `compose`, a numpy model of the frame the engine draws
(zs_render; csrc/zs_render.hpp), for a host picture from `get_state` output and as the tests' statement of the rules.

A frame is uint8 [10 H, 10 W, 3], RGB: the map area of the reference's OpencvRenderer.render (renderer.py:235-277).
Every drawn cell paints a one-colour 11 x 11 mask at (10 x, 10 y), the cells in x-outer, y-inner order, so a later cell
wins the pixel row or column it shares with an earlier neighbour; the frame clips the last row's and column's overhang.

Pure host code: importable without torch or a GPU.
"""
import numpy as np

from . import _abi

CELL, MASK = 10, 11
SHAPES = ("solid", "box", "disc", "frame", "body")  # the atlas's masks, in order: wall, box, zombie / player, objective, body
# palette entries; a body colour of 0 is "none recorded" and is drawn green, the zombies' own colour
GREEN, BLUE, CYAN, YELLOW, WHITE, RED = 0, 1, 2, 3, 4, 5
COLOR_NAMES = ("green", "blue", "cyan", "yellow", "white", "red")
_CSS = {"green": (0, 128, 0), "blue": (0, 0, 255), "cyan": (0, 255, 255), "yellow": (255, 255, 0),
        "white": (255, 255, 255), "red": (255, 0, 0)}
BOT_COLOR = {_abi.BOT_TERMINATOR: CYAN, _abi.BOT_SNIPER: YELLOW, _abi.BOT_HAMSTER: WHITE, _abi.BOT_RANDOMAN: RED,
             _abi.BOT_TROLL: BLUE}  # players/*.py


def _disc(x, y):
    return 0 <= x <= 10 and 0 <= y <= 10 and (x - 5) ** 2 + (y - 5) ** 2 <= 30  # radius 5.5 around the centre pixel


def rasterise(shape):
    """bool [11, 11] (row oy, column ox): the project's own drawing of one of SHAPES: a filled square, a 2-pixel frame
    with both diagonals, a disc, a 2-pixel frame, a disc's outline with both diagonals."""
    m = np.zeros((MASK, MASK), dtype=bool)
    for y in range(MASK):
        for x in range(MASK):
            frame = x < 2 or x > 8 or y < 2 or y > 8
            diag = x == y or x + y == 10
            ring = _disc(x, y) and not (_disc(x - 1, y) and _disc(x + 1, y) and _disc(x, y - 1) and _disc(x, y + 1))
            m[y, x] = {"solid": True, "frame": frame, "box": frame or diag, "disc": _disc(x, y), "body": ring or diag}[shape]
    return m


def pack_mask(m):
    """uint32 [4]: bit oy * 11 + ox of a bool [11, 11] mask (zs_render_sprites' form)."""
    bits = np.zeros(128, dtype=np.uint8)
    bits[:MASK * MASK] = np.asarray(m, dtype=np.uint8).reshape(-1)
    return np.packbits(bits, bitorder="little").view("<u4").astype(np.uint32)


def unpack_mask(words):
    w = np.ascontiguousarray(np.asarray(words, dtype="<u4"))
    return np.unpackbits(w.view(np.uint8), bitorder="little")[:MASK * MASK].reshape(MASK, MASK).astype(bool)


def default_atlas():
    """(masks uint32 [5, 4], palette uint8 [8, 3]): the five shapes and the CSS values of the six colour names; palette
    entries 6 and 7 are unused (black)."""
    masks = np.stack([pack_mask(rasterise(s)) for s in SHAPES])
    palette = np.zeros((8, 3), dtype=np.uint8)
    for i, name in enumerate(COLOR_NAMES):
        palette[i] = _CSS[name]
    return masks, palette


def slot_colors(A, bot_types, Z):
    """The palette index of every entity slot: agents blue, bots by type, zombies green."""
    return [BLUE] * A + [BOT_COLOR[int(b)] for b in bot_types] + [GREEN] * Z


def compose(W, H, entities=(), obstacles=(), bodies=(), objectives=(), atlas=None):
    """The frame of one world, uint8 [10 H, 10 W, 3].
    entities: (x, y, palette index) of every present zombie, bot and agent; obstacles: (x, y, kind) of every present
    wall (_abi.THING_WALL) and box (_abi.THING_BOX), whatever its life; bodies: (x, y, palette index) of every cell
    with a body; objectives: (x, y).  Per cell an entity hides an obstacle, which hides a body, which replaces an
    objective.  atlas: (masks, palette) as default_atlas() gives."""
    masks, palette = default_atlas() if atlas is None else atlas
    shape_of = {s: unpack_mask(masks[i]) for i, s in enumerate(SHAPES)}
    cell = {}
    for x, y in objectives:
        cell[(int(x), int(y))] = ("frame", BLUE)
    for x, y, c in bodies:
        cell[(int(x), int(y))] = ("body", int(c))
    for x, y, kind in obstacles:
        cell[(int(x), int(y))] = ("box", YELLOW) if kind == _abi.THING_BOX else ("solid", WHITE)
    for x, y, c in entities:
        cell[(int(x), int(y))] = ("disc", int(c))
    img = np.zeros((CELL * H + 1, CELL * W + 1, 3), dtype=np.uint8)  # one pixel more each way: the overhang, clipped below
    for (x, y) in sorted(cell):  # x outer, y inner
        if not (0 <= x < W and 0 <= y < H):
            continue
        shape, c = cell[(x, y)]
        img[CELL * y:CELL * y + MASK, CELL * x:CELL * x + MASK][shape_of[shape]] = palette[c & 7]
    return np.ascontiguousarray(img[:CELL * H, :CELL * W])


def compose_state(map_, st, colors, body_col=None, atlas=None):
    """The frame of an env from its zs_get_state record: map_ the config's maps.Map, st the engine.StateView, colors
    slot_colors(...) of the config, body_col the env's recorded body colours by cell (a sequence of W * H palette
    indices, or a dict cell -> index; default: every body green)."""
    W, H = map_.size
    ents = [(int(r[2]), int(r[3]), colors[s]) for s, r in enumerate(st.ent) if r[1]]
    obst = [(o[0], o[1], o[2]) for i, o in enumerate(map_.obstacles) if st.obst_present[i]]
    get = (lambda c: 0) if body_col is None else (body_col.get if isinstance(body_col, dict) else (lambda c: body_col[c]))
    bodies = [(c % W, c // W, int(get(c) or 0)) for c in st.dead_cells()]
    return compose(W, H, ents, obst, bodies, map_.objectives, atlas)
