"""The entity observation's host side on the CPU: the layout numbers, the bindings, the builders, and the oracle-only
census that says which case classes each GPU row of test_entity_obs.py shows (entity_obs_cases.REQUIRED)."""
import os
import re

import pytest

import entity_obs_cases as EC
from libzombsole_amd import _abi
from libzombsole_amd import engine
from libzombsole_amd import entity_obs as EO

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


@pytest.mark.parametrize("kz,kp", [(1, 0), (4, 1), (16, 16), (16, 0), (1, 16)])
def test_layout_numbers(kz, kp):
    L = _abi.entity_layout(kz, kp)
    assert L["row_words"] == 16 + 4 * (kz + kp) and L["row_bytes"] == 32 + 8 * (kz + kp) and L["row_bytes"] % 8 == 0
    assert (L["self"], L["zombies"], L["players"]) == (0, 8, 8 + 4 * kz)
    assert L["objective"] == L["players"] + 4 * kp and L["rays"] == L["objective"] + 4 and L["row_words"] == L["rays"] + 4
    assert L["ray_cap"] == 16 == EO.RAY_CAP
    assert {k: v for k, v in L.items() if k in EO.layout(kz, kp)} == EO.layout(kz, kp)


@pytest.mark.parametrize("kz,kp", [(0, 0), (17, 0), (1, -1), (1, 17), (-1, 4)])
def test_bad_k_is_refused_on_the_host(kz, kp):
    with pytest.raises(ValueError):
        _abi.entity_layout(kz, kp)
    with pytest.raises(ValueError):
        EO.layout(kz, kp)


def test_the_header_and_the_binding_name_the_calls():
    src = open(os.path.join(ROOT, "include", "zombsole_mi355x.h")).read()
    for s in ("zs_entity_obs_layout", "zs_entity_obs", "zs_entity_obs_bind"):
        assert re.search(r"^int %s\(" % s, src, re.M) and s in engine.SYMBOLS
    L = engine.load_library()
    assert L.zs_entity_obs.argtypes is not None and hasattr(L, "zs_entity_obs_bind")
    # the header's constants are the numpy statement's
    hpp = open(os.path.join(ROOT, "libzombsole_amd", "csrc", "zs_entity_obs.hpp")).read()
    assert "#define ZS_ENT_RAY_CAP %d" % EO.RAY_CAP in hpp and "#define ZS_ENT_HEAL_R2 %d" % EO.HEAL_R2 in hpp
    assert "need not be the one attack_closest hits" in hpp


def test_the_kernel_is_a_unit_of_its_own():
    import __graft_entry__ as ge
    assert ("k_entity_obs.hip", [], "k_entity_obs") in ge.UNITS


@pytest.mark.parametrize("row", EC.ROWS)
def test_census_of_the_gpu_rows(row):
    """Every class a row claims is shown by three or more of its 13 envs, by the oracle alone."""
    got = EC.claimed(row, 13)
    assert EC.REQUIRED[row] <= got, (row, sorted(EC.REQUIRED[row] - got))


def test_the_rows_cover_every_class():
    assert set().union(*EC.REQUIRED.values()) == set(EC.CLASSES)
    assert set(EC.REQUIRED) == set(EC.ROWS)
    b = EC.builder("fort_e132", 1)
    assert b.num_agents + b.num_bots + max(b.cfg.initial_zombies, b.cfg.minimum_zombies) > 64  # a second lane pass
    b = EC.builder("bridge_a4", 1)
    assert b.num_agents == 4 and b.num_bots == 2 and b.cfg.reward_mode == _abi.REWARD_MULTI
