"""The oracle under AddressSanitizer + UndefinedBehaviorSanitizer (host code only).

`oracle/Makefile` builds `libzs_oracle_asan.so` from the same source with
-fsanitize=address,undefined.  A child Python (libasan preloaded, since the interpreter is not
instrumented) replays golden fixtures through it and runs the bulk hash runner over the
configurations the GPU parity tests use; any sanitizer report aborts the child.
"""
import os
import subprocess
import sys

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

CHILD = r"""
import sys
sys.path[:0] = [%(root)r, %(tests)r]
from libzombsole_amd import _abi
from oracle.oracle import OracleEnv, load, run_hashes
import oracle.oracle as O
O._lib = load(%(so)r)
import golden_util, test_oracle_golden
for name in ("multi_bridge64_a2_z10", "multi_cityfs_safehouse_a4_z50", "single_easyexit_survival_rngbots_rich",
             "multi_fort_a32_z100"):
    test_oracle_golden.test_oracle_matches_reference(name)
mk = [
    lambda n: _abi.multi_env_config(n, "extermination", [], "bridge64", ["0", "1"], initial_zombies=10,
                                    max_episode_steps=12),
    lambda n: _abi.multi_env_config(n, "safehouse", [], "city128", ["0", "1", "2", "3"], initial_zombies=50,
                                    minimum_zombies=50, obs_dtype=_abi.DTYPE_I16),
    lambda n: _abi.single_env_config(n, "evacuation", ["terminator", "randoman", "hamster", "troll", "sniper"],
                                     "easy_exit", 0, initial_zombies=8, minimum_zombies=6,
                                     observation_scope="world", observation_position_encoding="channels",
                                     agent_weapon="random", max_episode_steps=30),
]
for m in mk:
    run_hashes(m(1), 5, 6, 40, 7 if m(1).cfg.reward_mode == _abi.REWARD_MULTI else 6, threads=1, reset_twice_mod=2)
# the far action stream (geometry_shapes.py): offsets up to the ends of int32 on the 257 x 2 strip and the 1 x 16 000 map
import geometry_shapes
for rid in ("c257x2", "x1x16000"):
    assert len(geometry_shapes.oracle_census(geometry_shapes.BY_ID[rid], 3)) == 3
print("sanitized ok")
"""


def _gcc_lib(name):
    return subprocess.check_output(["gcc", "-print-file-name=" + name]).decode().strip()


def test_oracle_under_asan_ubsan():
    from oracle.oracle import build
    try:
        so = build(asan=True)
    except (subprocess.CalledProcessError, OSError) as e:
        pytest.skip("sanitizer build unavailable: %s" % e)
    asan = _gcc_lib("libasan.so")
    if not os.path.isabs(asan):
        pytest.skip("libasan not found")
    env = dict(os.environ)
    env["LD_PRELOAD"] = asan
    env["ASAN_OPTIONS"] = "detect_leaks=0:abort_on_error=1"
    env["UBSAN_OPTIONS"] = "halt_on_error=1:print_stacktrace=1"
    code = CHILD % dict(root=ROOT, tests=os.path.join(ROOT, "tests"), so=so)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "sanitized ok" in r.stdout, r.stderr[-4000:]
    assert "runtime error" not in r.stderr, r.stderr[-4000:]
