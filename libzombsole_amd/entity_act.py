"""The entity action table in numpy: the second statement of its rules (the first is csrc/zs_entity_act.hpp).

    layout(kz, kp)                                 -> the table's blocks
    agent_table(state_view, static, kz, kp, a)     -> [(triple, mask bit)] of every id for agent a
    decode(state_view, static, kz, kp, ids)        -> int32 [A, 3]
    mask(state_view, static, kz, kp)               -> uint8 [A, row_bytes]
    encode(state_view, static, kz, kp, triples)    -> int32 [A]

NID = 15 + kz + kp ids per agent, kz and kp those of the entity observation (entity_obs.py):
  id                   triple                            mask bit is 1 exactly when
  0..3                 (MOVE, dir k)                     the destination is inside the map and World.things holds nothing there
  4                    (ATTACK_CLOSEST, 0, 0)            a present zombie stands within the agent's weapon range
  5                    (HEAL, 0, 0)                      always
  6                    (HEAL_CLOSEST, 0, 0)              no other agent or bot is present, or one stands within HEALING_RANGE
  7..10                (ATTACK, dir k)                   the adjacent cell is inside the map and holds a thing: a present
                                                         obstacle whatever its life, or a present zombie, bot or agent
  11..14               (HEAL, dir k)                     the adjacent cell holds a present agent or bot or a present obstacle
  15 + j, j < kz       (ATTACK, dx_j, dy_j)              zombie row j of the entity observation is valid and in weapon range
  15 + kz + j, j < kp  (HEAL, dx_j, dy_j)                player row j is valid and d2 <= 9
dir k = (0,1), (-1,0), (0,-1), (1,0); row j is the j-th present zombie, or the j-th other present agent or bot, by
(d2, slot).  A valid row decodes to its triple whatever its mask bit; a row past the present slots, an id outside
[0, NID) and every id of an agent that is not present decode to (IDLE, 0, 0) (the kernel also raises OVF_PARAM_RANGE
for an id outside the table); an agent that is not present has an all-zero mask row.  encode gives the smallest id
whose decoded triple equals the given one word for word, else -1.

`state_view` and `static` are entity_obs.encode's: an engine.StateView (or anything with `ent`, `obst_present`, `A`,
`P`) and an entity_obs.Static.
"""
import numpy as np

from . import actions as ACT
from .entity_obs import HEAL_R2, RAY_DIRS as DIRS, _nearest, weapon_r2

FIXED, ATTACK_DIR, HEAL_DIR = 15, 7, 11
MOVE, ATTACK_CLOSEST, HEAL_SELF, HEAL_CLOSEST = 0, 4, 5, 6
IDLE_TRIPLE = (ACT.ACT_IDLE, 0, 0)
LAYOUT_KEYS = ("nid", "row_bytes", "attack_dir", "heal_dir", "zombie_rows", "player_rows", "end")


def layout(kz, kp):
    """zs_entity_act_table on the host: "nid", "row_bytes" (nid rounded up to 8) and the first id of the blocks
    "attack_dir", "heal_dir", "zombie_rows", "player_rows", "end"."""
    kz, kp = int(kz), int(kp)
    if not (1 <= kz <= 16 and 0 <= kp <= 16):
        raise ValueError("entity actions: kz must be in 1..16 and kp in 0..16")
    nid = FIXED + kz + kp
    return dict(zip(LAYOUT_KEYS, (nid, (nid + 7) // 8 * 8, ATTACK_DIR, HEAL_DIR, FIXED, FIXED + kz, nid)))


def fixed_triple(i):
    """The triple of a fixed id (0..14)."""
    if i < 4:
        return (ACT.ACT_MOVE,) + DIRS[i]
    if i < ATTACK_DIR:
        return ((ACT.ACT_ATTACK_CLOSEST, ACT.ACT_HEAL, ACT.ACT_HEAL_CLOSEST)[i - 4], 0, 0)
    if i < HEAL_DIR:
        return (ACT.ACT_ATTACK,) + DIRS[i - ATTACK_DIR]
    return (ACT.ACT_HEAL,) + DIRS[i - HEAL_DIR]


def _rows(view, a, kz, kp):
    """(zombie rows, player rows) of present agent a: [(dx, dy, d2, slot)], at most kz and kp."""
    ent, A, P = view.ent, int(view.A), int(view.P)
    ax, ay = int(ent[a][2]), int(ent[a][3])
    return (_nearest(range(A + P, len(ent)), ent, ax, ay, kz),
            _nearest([s for s in range(A + P) if s != a], ent, ax, ay, kp))


def agent_table(view, static, kz, kp, a):
    """[(triple, mask bit)] of every id for agent a."""
    L = layout(kz, kp)
    ent, A, P = view.ent, int(view.A), int(view.P)
    if not int(ent[a][1]):
        return [(IDLE_TRIPLE, 0)] * L["nid"]
    ax, ay = int(ent[a][2]), int(ent[a][3])
    r2 = weapon_r2(ent[a][5])
    at = {(int(ent[s][2]), int(ent[s][3])): s for s in range(len(ent)) if int(ent[s][1]) and s != a}
    zrows, prows = _rows(view, a, len(ent), len(ent))  # every present slot of the two classes
    inside, obstacle, slot = [], [], []
    for dx, dy in DIRS:
        c = (ax + dx, ay + dy)
        o = static.obstacle_at.get(c)
        inside.append(0 <= c[0] < static.W and 0 <= c[1] < static.H)
        obstacle.append(inside[-1] and o is not None and bool(int(view.obst_present[o])))
        slot.append(at.get(c))
    bits = []
    for k in range(4):
        bits.append(inside[k] and not obstacle[k] and slot[k] is None)
    bits.append(any(d2 <= r2 for _dx, _dy, d2, _s in zrows))
    bits.append(True)
    bits.append(not prows or any(d2 <= HEAL_R2 for _dx, _dy, d2, _s in prows))
    for k in range(4):
        bits.append(inside[k] and (obstacle[k] or slot[k] is not None))
    for k in range(4):
        bits.append(inside[k] and (obstacle[k] or (slot[k] is not None and slot[k] < A + P)))
    table = [(fixed_triple(i), int(b)) for i, b in enumerate(bits)]
    for rows, K, kind, rr in ((zrows, kz, ACT.ACT_ATTACK, r2), (prows, kp, ACT.ACT_HEAL, HEAL_R2)):
        for j in range(K):
            if j < len(rows):
                dx, dy, d2, _s = rows[j]
                table.append(((kind, dx, dy), int(d2 <= rr)))
            else:
                table.append((IDLE_TRIPLE, 0))
    return table


def decode(view, static, kz, kp, ids):
    """The triples of `ids` ([A] integers), int32 [A, 3]."""
    A = int(view.A)
    out = np.zeros((A, 3), dtype=np.int32)
    for a in range(A):
        table = agent_table(view, static, kz, kp, a)
        i = int(ids[a])
        out[a] = table[i][0] if 0 <= i < len(table) else IDLE_TRIPLE
    return out


def decode_all(view, static, kz, kp):
    """The triple of every id, int32 [A, NID, 3]."""
    return np.array([[t for t, _b in agent_table(view, static, kz, kp, a)] for a in range(int(view.A))], dtype=np.int32)


def mask(view, static, kz, kp):
    """The mask rows, uint8 [A, row_bytes] (bytes past NID are 0)."""
    L = layout(kz, kp)
    out = np.zeros((int(view.A), L["row_bytes"]), dtype=np.uint8)
    for a in range(int(view.A)):
        out[a, :L["nid"]] = [b for _t, b in agent_table(view, static, kz, kp, a)]
    return out


def encode(view, static, kz, kp, triples):
    """The smallest id whose decoded triple is the agent's row of `triples` ([A, 3]), else -1; int32 [A]."""
    A = int(view.A)
    out = np.full(A, -1, dtype=np.int32)
    for a in range(A):
        want = tuple(int(v) for v in triples[a])
        for i, (t, _b) in enumerate(agent_table(view, static, kz, kp, a)):
            if tuple(t) == want:
                out[a] = i
                break
    return out
