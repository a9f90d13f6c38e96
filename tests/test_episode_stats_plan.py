"""Episode statistics (ZS_FLAG_EPISODE_STATS) on the CPU: the update rule of csrc/zs_episode.hpp, compiled into a
stand-alone host program (tests/episode_plan_host.cpp, host compiler, -fsanitize=address,undefined) and replayed over
recorded oracle traces, must equal episode_model.py bit for bit; the snapshot record's ep_run section for all four
flag combinations; the table of episode_cases.py shown by the oracle alone; the ABI's new symbols."""
import json
import os
import re
import subprocess

import pytest

import episode_cases as EC
import episode_model as EM
import step_plan_table as T
from libzombsole_amd import _abi, engine
from test_snapshot_layout import SHAPES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """The sanitized host program: lines in, one parsed JSON row per line out."""
    exe = str(tmp_path_factory.mktemp("episode_plan") / "episode_plan_host")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "libzombsole_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "episode_plan_host.cpp")])

    def run(lines):
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert out.returncode == 0, out.stderr[-2000:]
        rows = [json.loads(l) for l in out.stdout.splitlines()]
        assert len(rows) == len(lines)
        return rows
    return run


def _norm(xs):
    return [float.fromhex(x).hex() for x in xs]


# -- the shared update function against the model ---------------------------------------------------------------------
@pytest.mark.parametrize("row", EC.ROWS[::2], ids=lambda r: r.id)
def test_host_replay_equals_the_model(host, row):
    """Envs 0..12 of the row: the oracle's trace through episode_update() (host store) and through EnvModel."""
    cfg = row.make(1).cfg
    n_players = cfg.num_agents + cfg.num_bots
    for s in row.seeds()[:13]:
        k = EC.Track(row, s)
        lines, want = ["E %d %d %d" % (row.R, cfg.rules, n_players)], [None]
        for t in range(1, EC.STEPS + 1):
            o = k.o
            need = k.need
            if need:
                k.step(t)
                lines.append("S 1 0 0 0 0 0 0 0 0 0 0 " + " ".join(["0x0p+0"] * row.R))
            else:
                a = row.actions([s], t, o.A)[0]
                _, rew, d, tr, _ = o.step(a)
                cur = o.state()
                k.m.step(rew, d, tr, cur, row.triple())
                k.need = d or tr
                team = cur["agents"] + cur["players"]
                lines.append("S 0 %d %d %d %d %d %d %d %d %d %d " % (
                    (d, tr, k.m.length, cur["ctr"][2], cur["ctr"][1], sum(p[2] > 0 for p in team),
                     sum(p[2] > 0 for p in cur["agents"])) + row.triple()) + " ".join(float(rew[r]).hex() for r in range(row.R)))
            want.append(EM.snapshot([k.m]))
        if s == row.seeds()[0]:  # and the clear, once
            lines.append("C")
            k.m.clear()
            want.append(EM.snapshot([k.m]))
        got = host(lines)
        for g, w in zip(got[1:], want[1:]):
            assert _norm(g["run"]) == w["run_ret"][0] and _norm(g["last_ret"]) == w["last_ret"][0]
            assert _norm(g["sum_ret"]) == w["sum_ret"][0] and g["last"] == w["last"][0] and g["tot"] == w["tot"][0]
            assert g["closed"] == w["closed"][0]


def test_a_closed_env_is_not_counted_again(host):
    """Without autoreset an ended env keeps ticking and reporting done: one episode, until the reset."""
    term = "S 0 1 0 3 2 1 0 0 4 2 6 0x1p+0"
    rows = host(["E 1 1 2", "S 0 0 0 0 0 0 0 0 0 0 0 0x1p-1", term, term, term, "S 1 0 0 0 0 0 0 0 0 0 0 0x0p+0", term])
    assert rows[2]["tot"] == rows[3]["tot"] == rows[4]["tot"] == [1, 0, 1, 0, 0, 3, 2, 1] and rows[2]["closed"] == 1
    assert rows[2]["last"] == rows[4]["last"] == [3, 2, 2, 1, 4, 2, 6, 1] and _norm(rows[4]["run"]) == [(1.5).hex()]
    assert rows[5]["closed"] == 0 and _norm(rows[5]["run"]) == [(0.0).hex()] and rows[5]["tot"] == rows[4]["tot"]
    assert rows[6]["tot"][0] == 2 and rows[6]["last"][7] == 2 and _norm(rows[6]["sum_ret"]) == [(2.5).hex()]


# -- the record ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_layout_for_the_four_flag_combinations(host, shape):
    E, O, DW, OW, A = SHAPES[shape]
    for R in (1, A):
        rows = host(["L %d %d %d %d %d %d %d" % (E, O, DW, OW, A, envp, ep) for envp in (0, 1) for ep in (0, R)])
        L = {(envp, ep): rows[2 * envp + (ep != 0)] for envp in (0, 1) for ep in (0, R)}
        # the unflagged layouts are the parent's: the existing host programs, unchanged
        old = T.dump("env_params_layout_dump", ["L %d %d %d %d %d %d" % (E, O, DW, OW, A, f) for f in (0, 1)])
        for envp in (0, 1):
            r = L[(envp, 0)]
            assert {k: r[k] for k in old[envp]} == old[envp] and r["ep_run"] == r["ep_bytes"] == r["ep_gap"] == 0
            assert {k: r[k] for k in _abi.snapshot_layout(E, O, DW, OW, A, bool(envp))} == _abi.snapshot_layout(E, O, DW, OW, A, bool(envp))
            f = L[(envp, R)]
            end = r["weapon"]  # where the 4-byte sections (env_params included) end
            assert f["ep_run"] % 8 == 0 and f["ep_run"] - end == f["ep_gap"] == end % 8 and f["ep_bytes"] == 8 * R + 8
            assert f["weapon"] == f["ep_run"] + f["ep_bytes"] and f["rec_bytes"] % 16 == 0
            assert f["rec_bytes"] == (f["pad"] + 15) // 16 * 16 and f["pad"] == r["pad"] + f["ep_gap"] + f["ep_bytes"]
            for name in _abi.SNAPSHOT_SECTIONS[:13]:
                assert f[name] == r[name], name
            assert f["env_params"] == r["env_params"]
            for name in _abi.SNAPSHOT_SECTIONS[13:]:
                assert f[name] - r[name] == f["ep_gap"] + f["ep_bytes"], name
            mirror = _abi.snapshot_layout(E, O, DW, OW, A, bool(envp), R)
            assert {k: f[k] for k in mirror} == mirror
            w = host(["W %d %d %d %d %d %d %d 5" % (E, O, DW, OW, A, envp, R)])[0]
            assert w.get("ok"), w
            assert w["rec_bytes"] == f["rec_bytes"] and w["nsec"] == 18 + envp - (O == 0) * 3


def test_both_gap_parities_occur():
    gaps = {_abi.snapshot_layout(*SHAPES[s], env_params=e)["weapon"] % 8 for s in SHAPES for e in (False, True)}
    assert gaps == {0, 4}


def test_fingerprint_hashes_the_flag_last_and_only_when_set():
    mk = lambda **kw: _abi.multi_env_config(13, "extermination", [], "bridge64", ["0", "1"], initial_zombies=6,  # noqa: E731
                                            minimum_zombies=3, max_episode_steps=5, **kw)
    L = {(e, s): mk(env_params=e, episode_stats=s).snapshot_layout() for e in (False, True) for s in (False, True)}
    assert len({v["fingerprint"] for v in L.values()}) == 4
    from test_snapshot_layout import _builder_line
    got = T.dump("snapshot_layout_dump", [_builder_line(mk())])[0]  # the existing program: the parent's value
    assert got["fp_lo"] | (got["fp_hi"] << 32) == L[(False, False)]["fingerprint"]
    assert L[(False, True)]["fingerprint"] == _abi._fp_add(L[(False, False)]["fingerprint"], 32)
    assert L[(True, True)]["fingerprint"] == _abi._fp_add(L[(True, False)]["fingerprint"], 32)
    assert "ep_run" not in L[(True, False)] and L[(True, True)]["ep_run"] % 8 == 0


def test_header_constants_and_symbols():
    src = open(os.path.join(ROOT, "include", "zombsole_mi355x.h")).read()
    assert int(re.search(r"#define ZS_FLAG_EPISODE_STATS (\d+)u", src).group(1)) == _abi.FLAG_EPISODE_STATS == 32
    declared = set(re.findall(r"^\s*(?:const\s+)?\w+\*?\s+\*?(zs_\w+)\s*\(", src, re.M))
    L = engine.load_library()
    for name in ("zs_episode_stats_layout", "zs_episode_stats_get", "zs_episode_stats_clear"):
        assert name in engine.SYMBOLS and name in declared and hasattr(L, name)
    assert declared == set(engine.SYMBOLS)
    hdr = open(os.path.join(ROOT, "libzombsole_amd", "csrc", "zs_episode.hpp")).read()
    for name, v in (("ZS_EP_WON", 1), ("ZS_EP_LOST", 2), ("ZS_EP_AGENTS_DEAD", 3), ("ZS_EP_TIMELIMIT", 4),
                    ("ZS_EP_DONE_AND_TIMELIMIT", 256)):
        assert int(re.search(r"#define %s (\d+)" % name, hdr).group(1)) == v
    assert "hip_runtime" not in hdr  # the header needs no HIP
    b = _abi.single_env_config(3, "extermination", [], "bridge64", 0, episode_stats=True)
    assert b.cfg.flags & 32 and not _abi.single_env_config(3, "extermination", [], "bridge64", 0).cfg.flags & 32


# -- the table, by the oracle alone -----------------------------------------------------------------------------------
def test_rows_cover_the_matrix():
    assert [r.config for r in EC.ROWS[::2]] == list(EC.CONFIGS) and len({r.id for r in EC.ROWS}) == 18
    assert {r.n for r in EC.ROWS} == {13, 37, 67, 300} and EC.STEPS == 24
    for cfg in EC.CONFIGS:
        assert {r.step_kernel for r in EC.ROWS if r.config == cfg} == {"k_step", "k_tick"}
    plans = T.plans([(r.builder(), dict(r.launch, par_exec=1)) for r in EC.ROWS])
    for r, p in zip(EC.ROWS, plans):
        assert "error" not in p and ("k_step" if p["fused"] else "k_tick") == r.step_kernel and p["G"] == r.G, (r.id, p)
    assert {r.R for r in EC.ROWS} >= {1, 2, 4}


CLASS_OF = {1: ("ext_won", "ext_min_won", "safe_won", "evac_won", "single_won"),
            2: ("ext_lost", "safe_lost", "evac_lost", "surv_lost", "single_lost")}


def test_every_outcome_code_occurs_and_agrees_with_classify():
    envs = {1: set(), 2: set(), 3: set(), 4: set(), 256: set()}
    for r in EC.ROWS[::2]:  # the two kernels of a config share seeds and streams: one census per config
        _, ends = EC.trace(r.id)
        for e, t, code, cls in ends:
            envs[code & 255].add((r.config, e))
            if code & 256:
                envs[256].add((r.config, e))
                assert "done_and_timelimit" in cls
            else:
                assert "done_and_timelimit" not in cls
            if (code & 255) in (1, 2):
                assert cls & set(CLASS_OF[code & 255]) and not cls & set(CLASS_OF[3 - (code & 255)]), (r.id, e, t, code, cls)
            assert ("agents_dead_bot_alive" in cls) == ((code & 255) == 3), (r.id, e, t, code, cls)
    for code, where in envs.items():
        assert len(where) >= 3, (code, len(where))


@pytest.mark.parametrize("config", EC.MULTI_STEP)
def test_envs_end_twice_within_sixteen_steps(config):
    """The multi-step launch test means something only if tot[0] grows by 2 or more within one 16-step launch."""
    row = [r for r in EC.ROWS if r.config == config][0]
    snaps, _ = EC.trace(row.id, 48)
    grown = 0
    for lo in (0, 16, 32):
        grown += sum(1 for a, b in zip(snaps[lo]["tot"], snaps[lo + 16]["tot"]) if b[0] - a[0] >= 2)
    assert grown >= 3, grown


def test_no_autoreset_rows_end(host):
    """surv_melee ends for most envs within the 24 steps (the no-autoreset GPU case needs envs that ended)."""
    row = [r for r in EC.ROWS if r.config == "surv_melee"][0]
    snaps, _ = EC.trace(row.id)
    assert sum(1 for t in snaps[-1]["tot"] if t[0] >= 1) >= 3
