"""A plain observation encoder written for the tests: gym/observation.py's rules over the oracle's canonical state
(OracleEnv.state()), in numpy.  It is neither the oracle's encoder (oracle/zs_oracle.c encode_window) nor the
engine's (csrc/zs_obs.hpp): test_obs_shapes_plan.py holds the oracle's observations to it at every env and step of
obs_shapes.py's rows and over the reference fixtures, which pins the oracle where no reference fixture exists
(per-agent simple blocks on the multi surface, where the reference itself raises).

The rules: a cell off the map is a Wall of life 200; on the map a thing comes first, then an obstacle that is
still in the world, then a dead body, then an objective, then nothing (code 0, life 0, weapon 0).  channels is
(code, life, weapon) with an agent's code 8 + agent_id; simple is 256 * code + 16 * weapon + (15 * min(life, 100))
// 100 in Python ints (floor division), an agent's code staying 7.  int16 saturation comes last: it is the
engine's documented lossy form (include/zombsole_mi355x.h ZS_OVF_INT16), not the reference's.
"""
import numpy as np

from libzombsole_amd import _abi

MAX_LIFE = {_abi.THING_BOX: 10, _abi.THING_WALL: 200}


def planes(builder, state):
    """(code, life, weapon) of every map cell, int64 [H][W]; an agent's code is 7 here, `who` its agent index + 1."""
    W, H = builder.map.size
    code, life, weapon, who = (np.zeros((H, W), dtype=np.int64) for _ in range(4))
    for x, y in builder.map.objectives:
        code[y, x] = _abi.THING_OBJECTIVE
    for c in state["dead"]:
        code[c // W, c % W] = _abi.THING_DEADBODY
    changed = {i: (lf, present) for i, lf, present in state["obst"]}
    for i, (x, y, kind) in enumerate(builder.map.obstacles):
        lf, present = changed.get(i, (MAX_LIFE[kind], 1))
        if present:
            code[y, x], life[y, x] = kind, lf
    for kind, x, y, lf, wp, extra in state["dyn"]:
        code[y, x], life[y, x], weapon[y, x] = kind, lf, wp
        who[y, x] = extra + 1 if kind == _abi.THING_AGENT else 0
    return code, life, weapon, who


def _window(p, x0, y0, w, h, fill):
    """p[y0:y0 + h, x0:x0 + w] with `fill` where that leaves the map."""
    H, W = p.shape
    out = np.full((h, w), fill, dtype=np.int64)
    xa, xb, ya, yb = max(x0, 0), min(x0 + w, W), max(y0, 0), min(y0 + h, H)
    if xa < xb and ya < yb:
        out[ya - y0:yb - y0, xa - x0:xb - x0] = p[ya:yb, xa:xb]
    return out


def _simple(code, life, weapon):
    vals, inv = np.unique(life, return_inverse=True)
    f = np.array([(15 * min(int(v), 100)) // 100 for v in vals], dtype=np.int64)  # Python ints: floor division
    return 256 * code + 16 * weapon + f[inv].reshape(life.shape)


def observe(builder, state, agent_ids):
    """The observation of one env, in the shape and dtype the config asks for (builder.obs_shape()).  agent_ids: the
    ids the config's agents were created with, in order; an agent's channels code is 8 + int(agent_id)."""
    c = builder.cfg
    W, H = builder.map.size
    code, life, weapon, who = planes(builder, state)
    channels = c.obs_encoding == _abi.ENC_CHANNELS
    if channels:
        code = np.where(who > 0, 8 + np.array([int(v) for v in agent_ids], dtype=np.int64)[who - 1], code)
    if c.obs_scope == _abi.OBS_WORLD:
        views = [(0, 0, W, H)]
    else:
        n = c.num_agents if c.reward_mode == _abi.REWARD_MULTI else 1
        views = [(a[0] - c.obs_width // 2, a[1] - c.obs_width // 2, c.obs_width, c.obs_width) for a in state["agents"][:n]]
    out = []
    for x0, y0, w, h in views:
        k, lf, wp = (_window(p, x0, y0, w, h, fill) for p, fill in ((code, _abi.THING_WALL), (life, 200), (weapon, 0)))
        out.append(np.stack([k, lf, wp]) if channels else _simple(k, lf, wp)[None])
    out = np.stack(out)
    if c.obs_dtype == _abi.DTYPE_I16:
        out = np.clip(out, -32768, 32767)
    return out.astype(_abi.DTYPE_NP[c.obs_dtype])
