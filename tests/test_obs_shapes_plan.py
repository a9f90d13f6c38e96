"""obs_shapes.py on the CPU: every row against the compiled observation and step plans (tests/obs_plan_dump.cpp,
tests/step_plan_dump.cpp), the table's coverage, the oracle's own run of every row held to the plain encoder of
obs_model.py at every env and step, the content the rows' windows must show, and the model over the reference
fixtures that hold observations."""
import numpy as np
import pytest

import obs_model
import obs_shapes as S
import obs_plan_table as T
import step_plan_table
from libzombsole_amd import _abi


@pytest.fixture(scope="module")
def plans():
    rows = step_plan_table.dump("obs_plan_dump", [
        " ".join(str(v) for v in [0] + T.shape_ints(r.builder(), r.launch) + step_plan_table.launch_ints(r.launch))
        for r in S.ROWS])
    return dict(zip((r.id for r in S.ROWS), rows))


def function_of(p, row):
    """The function of obs_stream() (csrc/zs_obs.hpp) the compiled plan's fields lead to, or the store stream."""
    name = p["full"]["name"]
    if name in ("k_obs_pipe", "k_obs_gather"):
        return name[len("k_obs_"):]
    assert name == "k_obs"
    c = row.builder(1).cfg
    if p["obs_stat"] and p["step_hp_cap"] and p["step_win"] and c.map.n_obstacles > 0:
        return "fast21" if c.obs_scope != _abi.OBS_WORLD and c.obs_width == 21 else "fast0"
    return "gen_scan" if not p["step_win"] else "gen_hbm" if not p["step_hp_cap"] else "gen_win"


def test_rows_resolve_as_claimed(plans):
    bad = []
    for r in S.ROWS:
        p = plans[r.id]
        assert "error" not in p, r.id
        full = p["full"]
        got = (S.STEP if p["fobs"] else full["name"], p["masked"]["name"], full["win"] != 0, full["hp_cap"] != 0,
               p["obs_stat"] != 0, full["envs_per_wg"], p["fobs"])
        if got != r.plan:
            bad.append((r.id, "plan", got, r.plan))
        if function_of(p, r) != r.func:
            bad.append((r.id, "function", function_of(p, r), r.func))
        if full["name"] == "k_obs":  # the step launch's image is k_obs's
            assert (p["step_win"], p["step_hp_cap"], p["step_img_bytes"]) == (full["win"], full["hp_cap"], full["img_bytes"])
    assert not bad, bad


def test_where_rows_resolve_in_the_step_plan():
    """The lanes per env the tick rows ask for stand, `fused` and `unfused` are what the step plan launches."""
    rows = step_plan_table.plans([(r.builder(), r.launch) for r in S.WHERE_ROWS])
    for r, p in zip(S.WHERE_ROWS, rows):
        if r.lanes:
            assert p["G"] == r.lanes, (r.id, p)
        if r.step_kernel:
            assert p["fused"] == (r.step_kernel == "k_step"), (r.id, p)
        assert (p["obs_bytes"] != 0) == bool(r.plan[6]), (r.id, p)


def test_table_covers_what_it_claims():
    combos = {(r.func, r.dt, r.enc) for r in S.SHAPE_ROWS}
    assert combos >= {(f, dt, enc) for f in S.FUNCS for dt in S.DTS for enc in S.ENCS}
    # the 18 simple store-stream instantiations, and the three overrides that ask for a staged kernel
    stream = {(r.func, r.dt, r.builder(1).num_agents) for r in S.STREAM_ROWS if "_asked" not in r.id}
    assert stream == {(v, dt, nobs) for v in ("pipe", "gather") for dt in S.DTS for nobs in (1, 2, 4)}
    assert all(r.enc == "simple" and r.builder(1).cfg.obs_encoding == _abi.ENC_SIMPLE for r in S.STREAM_ROWS)
    assert sum("_asked" in r.id for r in S.STREAM_ROWS) == 3
    # every listed width on both maps under both encodings, every listed world size
    ids = set(S.BY_ID)
    for m in ("small", "bridge64"):
        for w in S.SURR_WIDTHS:
            for enc in S.ENCS:
                assert any(i.startswith("surr%d-%s-%s-" % (w, m, enc)) for i in ids), (m, w, enc)
    for w, h in S.WORLD_SIZES:
        b = S.single("field%dx%d" % (w, h), "world", "simple", "i32")(1)
        assert b.obs_shape() == (1, 1, h, w)
        for enc in S.ENCS:
            assert any(i.startswith("world-field%dx%d-%s-" % (w, h, enc)) for i in ids)
    # 3 and 5 agents at width 21, env counts odd and no multiple of 4
    assert {r.builder(1).num_agents for r in S.ROWS if r.func == "fast21"} == {3, 5}
    assert all(r.n % 2 == 1 and r.n in (13, 37, 67) for r in S.ROWS)


def _plan_of(make, lo=None):
    b = make(13)
    return step_plan_table.dump("obs_plan_dump", [" ".join(str(v) for v in [0] + T.shape_ints(b, lo or {}) +
                                                            step_plan_table.launch_ints(lo))])[0]


def test_tier_boundaries_on_both_sides():
    """Each boundary of the module docstring: the two odd widths either side of it differ in exactly that field."""
    def fields(make):
        p = _plan_of(make)
        return {"win": p["full"]["win"] != 0, "hp": p["full"]["hp_cap"] != 0, "wpg": p["full"]["envs_per_wg"], "fobs": p["fobs"]}
    one = lambda w: S.single("small", "surroundings:%d" % w, "channels", "i64")  # noqa: E731
    assert (fields(one(179))["win"], fields(one(181))["win"]) == (True, False)
    four = lambda w: S.multi("small", 4, w, "channels", "i64")  # noqa: E731
    assert (fields(four(89))["win"], fields(four(91))["win"]) == (True, False)
    city = lambda w: S.single("city128", "surroundings:%d" % w, "channels", "i64", zombies=20)  # noqa: E731
    a, b = fields(city(123)), fields(city(125))
    assert (a["win"], a["hp"], b["win"], b["hp"]) == (True, True, True, False)
    a, b = fields(one(127)), fields(one(129))
    assert (a["wpg"], a["fobs"], b["wpg"], b["fobs"]) == (4, 1, 1, 0)
    for prefix in ("win179-", "scan181-", "a4win89-", "a4scan91-", "hp123-", "hbm125-", "surr127-small-", "wpg129-"):
        assert any(i.startswith(prefix) for i in S.BY_ID), prefix  # both sides of every boundary are rows


def test_refusal_is_the_plans(plans):
    make, msg, which = S.REFUSED
    assert which == "obs" and _plan_of(make) == {"error": msg}


# -- the oracle's run of every row -------------------------------------------------------------------------------------
CLASSES = ("top", "bottom", "left", "right", "off_top", "off_bottom", "off_left", "off_right", "second",
           "body_under_obstacle", "damaged", "cleaned_up")


def oracle_run(row, n):
    """The oracle alone over the row's first n envs: yields (env, step, observation, state, the env) at the reset
    and after every step, autoresets as the engine does them."""
    from oracle.oracle import OracleEnv
    for k, s in enumerate(row.seeds(n)):
        o = OracleEnv(row.builder(1))
        o.seed(s)
        yield k, 0, o.reset(), o.state(), o
        need = False
        for t in range(1, row.steps + 1):
            if need:
                obs, need = o.reset(), False
            else:
                obs, _, d, tr, _ = o.step(S.actions([s], t, o.A)[0])
                need = d or tr
            yield k, t, obs, o.state(), o


def _codes(obs, row):
    """The code plane(s) of an observation: [observations][h][w]."""
    return obs[:, 0] if row.enc == "channels" else obs[:, 0].astype(np.int64) >> 8


def census(row):
    """The oracle's run of the row, every observation held to the model, then the pokes of S.poke_plan (the ones
    test_obs_shapes.py applies to the engine) and the poked observation held to the model too.  Returns class ->
    the number of envs that show it: a thing (zombie, player, agent) in the first / last row / column of what an
    observation shows of the map (the window's own edge where that lies on the map, the map's edge where the window
    hangs over it); an off-map cell on each side; a second living agent inside the first one's window; after the
    pokes, inside an observation, an obstacle in the world with a body under it, a damaged obstacle in the world,
    and the cell of a cleaned-up obstacle."""
    b = row.builder(1)
    W, H = b.map.size
    world = b.cfg.obs_scope == _abi.OBS_WORLD
    half = b.cfg.obs_width // 2
    ids = row.agent_ids()
    seen = {k: np.zeros((row.n,), bool) for k in CLASSES}
    envs = {}
    for k, t, obs, st, o in oracle_run(row, row.n):
        envs[k] = o
        assert np.array_equal(obs, obs_model.observe(b, st, ids)), ("model != oracle", row.id, k, t)
        thing = _codes(obs, row) >= _abi.THING_ZOMBIE  # off-map cells are Wall (4): things on the map only
        for a in range(obs.shape[0]):
            x0, y0 = (0, 0) if world else (st["agents"][a][0] - half, st["agents"][a][1] - half)
            h, w = thing.shape[1:]
            r0, r1, c0, c1 = max(0, -y0), min(h, H - y0) - 1, max(0, -x0), min(w, W - x0) - 1
            seen["top"][k] |= thing[a, r0, :].any()
            seen["bottom"][k] |= thing[a, r1, :].any()
            seen["left"][k] |= thing[a, :, c0].any()
            seen["right"][k] |= thing[a, :, c1].any()
            seen["off_top"][k] |= r0 > 0
            seen["off_left"][k] |= c0 > 0
            seen["off_bottom"][k] |= r1 < h - 1
            seen["off_right"][k] |= c1 < w - 1
        if not world and obs.shape[0] > 1:
            (ax, ay), (bx, by) = st["agents"][0][:2], st["agents"][1][:2]
            seen["second"][k] |= abs(ax - bx) <= half and abs(ay - by) <= half and st["agents"][1][2] > 0
    rng = np.random.default_rng(57)
    for k in range(row.n):
        o = envs[k]
        S.poke_oracle(o, S.poke_plan(b, o.state(), rng, k), W)
        st = o.state()
        obs = o.obs()
        assert np.array_equal(obs, obs_model.observe(b, st, ids)), ("model != oracle after the pokes", row.id, k)
        changed = {i: (life, present) for i, life, present in st["obst"]}
        things = {(d[1], d[2]) for d in st["dyn"]}
        for a in range(obs.shape[0]):
            x0, y0, x1, y1 = S.view_rect(b, st, a)
            for i, (x, y, kind) in enumerate(b.map.obstacles):
                if not (x0 <= x <= x1 and y0 <= y <= y1) or i not in changed or (x, y) in things:
                    continue
                life, present = changed[i]
                seen["cleaned_up"][k] |= not present
                seen["damaged"][k] |= bool(present)  # listed in the state and in the world: its life is not the full one
                seen["body_under_obstacle"][k] |= bool(present) and (y * W + x) in st["dead"]
    return {k: int(v.sum()) for k, v in seen.items()}


@pytest.mark.parametrize("row", S.ROWS, ids=[r.id for r in S.ROWS])
def test_model_equals_oracle_and_rows_show_their_content(row):
    """Every env and step of the row, and its poked states: the model equals the oracle's observation, bit for bit.
    And every class S.required(row) names is in view in three envs or more."""
    got = census(row)
    for key in S.required(row):
        assert got[key] >= 3, (row.id, key, got)


def test_model_equals_reference_fixtures():
    """The model over every reference fixture: at every call, the model's observation of the state the reference
    recorded has the hash of the observation the reference recorded there (int32 on the single surface, int64 per
    listed agent on the multi surface), and equals the full observation where the fixture holds one.  The oracle
    meets the same records in test_oracle_golden.py, so the model and the oracle both mean the reference."""
    import golden_util as G
    calls = 0
    for name in G.fixture_names():
        fx = G.load_fixture(name)
        b = G.builder_for(fx)
        ids = fx["kwargs"]["agent_ids"] if fx["surface"] == "multi" else [fx["kwargs"]["agent_id"]]
        for run in fx["runs"]:
            for i, rec in enumerate(run["calls"]):
                if "obs_sha" not in rec or "raised" in rec:
                    continue
                obs = obs_model.observe(b, rec["state"], ids)
                listed = None
                if fx["surface"] == "multi":
                    listed = [j in rec["obs_keys"] for j in range(b.num_agents)]
                assert G.obs_sha(fx, obs, listed) == rec["obs_sha"], (name, run["seed"], i)
                if "obs" in rec and fx["surface"] == "single":
                    assert obs.ravel().tolist() == rec["obs"], (name, run["seed"], i)
                calls += 1
    assert calls > 1000
