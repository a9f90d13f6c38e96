"""C-ABI library: loads without a GPU and exports every entry point include/ declares."""
import ctypes
import os
import re

from libzombsole_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    src = open(os.path.join(ROOT, "include", "zombsole_mi355x.h")).read()
    return sorted(set(re.findall(r"^\s*(?:const\s+)?\w+\*?\s+\*?(zs_\w+)\s*\(", src, re.M)))


def prototypes():
    """{name: parameter list} of every zs_* prototype of the header, comments stripped."""
    src = open(os.path.join(ROOT, "include", "zombsole_mi355x.h")).read()
    src = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", src, flags=re.S))
    protos = re.findall(r"\b(?:const\s+char\s*\*|int)\s+(zs_\w+)\s*\(([^)]*)\)\s*;", src)
    assert len(protos) == len(set(n for n, _ in protos))
    return {n: [] if p.strip() == "void" else [a.strip() for a in p.split(",")] for n, p in protos}


def test_header_declares_the_binding_list():
    assert declared_symbols() == sorted(engine.SYMBOLS)


def test_binding_table_matches_the_header():
    """_abi.ABI has a row for every prototype and no other, each with as many argtypes as the prototype has
    parameters, and load_library binds every one (a function left at ctypes' defaults takes a Python int as a C int:
    a 64-bit pointer would lose its upper half)."""
    from libzombsole_amd import _abi
    protos = prototypes()
    assert set(protos) == set(_abi.ABI) == set(declared_symbols())
    for name, params in protos.items():
        assert len(params) == len(_abi.ABI[name]), name
    L = engine.load_library()
    for name in _abi.ABI:
        f = getattr(L, name)
        assert f.argtypes is not None and list(f.argtypes) == list(_abi.ABI[name]), name
        assert f.restype is (ctypes.c_char_p if name == "zs_last_error" else ctypes.c_int), name


def test_layout_keys_cover_the_declared_words():
    """Every layout call's key tuple (_abi.LAYOUT_KEYS) names as many words as the header declares for its out[]."""
    from libzombsole_amd import _abi
    protos = prototypes()
    sizes = {}
    for name in _abi.LAYOUT_KEYS:
        (n,) = re.findall(r"int32_t out\[(\d+)\]", protos[name][-1])
        sizes[name] = int(n)
        assert len(_abi.LAYOUT_KEYS[name]) == sizes[name], name
        named = [k for k in _abi.LAYOUT_KEYS[name] if k is not None]
        assert len(set(named)) == len(named), name  # the keys become one dict: no name twice
    assert set(_abi.LAYOUT_KEYS) == set(n for n in protos if n.endswith("_layout"))
    assert sizes == {"zs_obs_state_layout": 12, "zs_snapshot_layout": 24, "zs_entity_obs_layout": 8,
                     "zs_episode_stats_layout": 8, "zs_render_layout": 8, "zs_host_layout": 8}


def test_as_index():
    """engine.as_index: sequences and integer tensors of any width come back as the same int32 values; a value int32
    does not hold becomes -1 instead of wrapping (2**32 + 3 used to become 3); bool, float, 2-D and 0-D input raise."""
    import pytest
    import torch
    same = [3, 0, 7, 7, -1]
    for x in (same, torch.tensor(same, dtype=torch.int32), torch.tensor(same, dtype=torch.int64)):
        got = engine.as_index(torch, x, "cpu", "test")
        assert got.dtype == torch.int32 and got.dim() == 1 and got.is_contiguous() and got.tolist() == same
    wide = torch.tensor([2 ** 31, -2 ** 31 - 1, 2 ** 32 + 3, 2 ** 31 - 1, -2 ** 31], dtype=torch.int64)
    assert engine.as_index(torch, wide, "cpu", "test").tolist() == [-1, -1, -1, 2 ** 31 - 1, -2 ** 31]
    assert engine.as_index(torch, wide.tolist(), "cpu", "test").tolist() == [-1, -1, -1, 2 ** 31 - 1, -2 ** 31]
    assert engine.as_index(torch, wide[::2], "cpu", "test").tolist() == [-1, -1, -2 ** 31]  # a strided view
    for bad in (torch.tensor([True, False]), torch.tensor([1.0, 2.0]), torch.zeros((2, 2), dtype=torch.int32),
                torch.tensor(3, dtype=torch.int32)):
        with pytest.raises(ValueError, match="1-D integer"):
            engine.as_index(torch, bad, "cpu", "test")


def test_library_loads_and_exports_all_symbols():
    L = engine.load_library()
    for s in declared_symbols():
        assert hasattr(L, s), s
        assert ctypes.cast(getattr(L, s), ctypes.c_void_p).value


def test_library_is_gfx950_code_object():
    data = open(engine.LIB_PATH, "rb").read()
    assert b"gfx950" in data


def test_struct_layout_matches_header(tmp_path):
    """The ctypes mirrors of zs_map_desc / zs_launch / zs_config (libzombsole_amd/_abi.py) have the
    header's sizes and field offsets (gcc on the header itself)."""
    import subprocess

    from libzombsole_amd import _abi
    structs = {"zs_map_desc": _abi.zs_map_desc, "zs_launch": _abi.zs_launch, "zs_config": _abi.zs_config}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "zombsole_mi355x.h"', 'int main(void) {']
    for name, cls in structs.items():
        lines.append('printf("%s sizeof %%zu\\n", sizeof(%s));' % (name, name))
        for f in cls._fields_:
            lines.append('printf("%s %s %%zu\\n", offsetof(%s, %s));' % (name, f[0], name, f[0]))
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = dict((" ".join(l.split()[:2]), int(l.split()[2])) for l in subprocess.check_output([str(exe)]).decode().splitlines())
    for name, cls in structs.items():
        assert got["%s sizeof" % name] == ctypes.sizeof(cls), name
        for f in cls._fields_:
            assert got["%s %s" % (name, f[0])] == getattr(cls, f[0]).offset, (name, f[0])


def test_checked_launder_build_compiles(tmp_path):
    """The kernels that reload their Dev from kernarg offset 0 (zs_launder_dev: k_reset, k_respawn here) build
    with the contract check on (-DZS_CHECK_LAUNDER: the reloaded fields against the kernel's argument)."""
    import subprocess
    import __graft_entry__ as ge
    subprocess.check_call([ge._hipcc()] + ge.HIPCC_FLAGS + ["-DZS_CHECK_LAUNDER", "-c", "-o", str(tmp_path / "k_reset.o"),
                                                         os.path.join(ge.CSRC, "k_reset.hip")])


def test_lanes_per_env_is_validated():
    """zs_create refuses a lanes_per_env that is neither 0 nor one of the lane counts the step kernels are
    compiled for (1, 2, 4, 8, 16, 32, 64) before it touches a device: ZS_EINVAL (a ValueError through the
    binding) naming the field, and no handle.  Such a value used to size the launch for 64 / G envs per
    workgroup and then run the G = 64 kernel, which ticks one: most envs were never stepped."""
    import pytest

    from libzombsole_amd import _abi
    L = engine.load_library()
    for lanes in (3, 6, 48, 65, 128, -1, -8):
        b = _abi.multi_env_config(8, "extermination", [], "bridge64", ["0", "1"], initial_zombies=10,
                                  lanes_per_env=lanes)
        h = ctypes.c_void_p()
        rc = L.zs_create(ctypes.cast(b.ptr(), ctypes.c_void_p), 0, ctypes.byref(h))
        assert rc == _abi.ZS_EINVAL and not h.value, (lanes, rc)
        assert b"lanes_per_env" in L.zs_last_error()
        with pytest.raises(ValueError, match="lanes_per_env"):
            engine._raise(L, rc, "zs_create")
