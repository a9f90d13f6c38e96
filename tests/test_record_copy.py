"""The record walker (libzombsole_amd/csrc/zs_record.hpp: the section table and rec_copy_chunk, which the engine's
k_obs_state_pack / k_obs_state_unpack / k_snapshot / k_restore call per 16-B chunk) on the CPU: the header compiled
with the host compiler into tests/record_copy_host.cpp, which packs and unpacks host arrays shaped like the engine's
and compares with records put together element by element.  The same program once more under the address and
undefined-behaviour sanitizers, as a stand-alone executable."""
import json
import os
import subprocess

import pytest

import step_plan_table as T

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

# (E, O, DW, OW, A, N): the smallest shapes that reach every branch of the walker
SHAPES = {
    "odd_everything": (7, 5, 3, 1, 1, 5),        # rows start at odd dword offsets, chunks straddle sections
    "bridge64_E12_A2": (12, 384, 128, 12, 2, 3),  # the aligned fast paths, in both record types
    "no_obstacles": (7, 0, 47, 0, 1, 2),          # empty sections
    "long_byte_rows": (70, 16, 1, 1, 3, 2),       # byte rows longer than a chunk
}
RECORDS = {"snapshot": "S %d %d %d %d %d %d", "obs_state_hp4": "O %d %d %d %d %d %d 4", "obs_state_hp2": "O %d %d %d %d %d %d 2"}


def by_hand(record, E, O, DW, OW, A):
    """rec_bytes from the per-env sizes of the arrays a record copies (zs_snapshot.hpp / zs_obs_state.hpp)."""
    if record == "snapshot":
        nb = 4 * (2 * 624 + DW + O + 2 * OW + 3 * E + 9 + 3 + A) + 3 * E + A
    else:
        nb = 4 * (2 + 2 * E + DW + OW) + (4 if record == "obs_state_hp4" else 2) * O + 2 * E
    return (nb + 15) // 16 * 16


@pytest.mark.parametrize("record", sorted(RECORDS))
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_walker_against_the_naive_record(shape, record):
    s = SHAPES[shape]
    row, = T.dump("record_copy_host", [RECORDS[record] % s])
    assert row["ok"], row.get("error")
    assert row["rec_bytes"] == by_hand(record, *s[:5]) == 16 * row["chunks"]
    E, O, DW, OW, A = s[:5]  # a table leaves empty sections out
    sizes = [1248, DW, O, OW, OW, E, E, E, 9, 1, 1, 1, A, E, E, E, A] if record == "snapshot" else [1, 1, E, E, DW, OW, O, E, E]
    assert row["nsec"] == sum(1 for n in sizes if n)


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("record_copy") / "record_copy_host_san")
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "libzombsole_amd", "csrc"), "-o", exe, os.path.join(HERE, "record_copy_host.cpp")]
    probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", exe + "_probe"],
                           input="int main() { return 0; }\n", capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip("the host g++ lacks the sanitizer runtimes: " + probe.stderr.strip().splitlines()[-1])
    subprocess.check_call(cmd)
    return exe


def test_walker_under_sanitizers(sanitized):
    names = list(SHAPES)
    lines = [RECORDS[r] % SHAPES[n] for n in (names[0], names[-1]) for r in sorted(RECORDS)]
    out = subprocess.run([sanitized], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = [json.loads(l) for l in out.stdout.splitlines()]
    assert len(rows) == len(lines) and all(r["ok"] for r in rows), rows
