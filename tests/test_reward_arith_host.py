"""The non-terminal rewards as arithmetic (csrc/cat_sim_reward.h), host build, against the tables of as_cops_and_thieves_amd/tables.py.

``reward_arith_max`` is the largest index up to which that function agrees with BOTH tables at every entry (cat_reward_arith_host for any pair of tables,
cat_reward_arith_max for a handle's).  The
kernels load their rewards from the tables (the arithmetic in the write-back measured slower: DESIGN 4.9); the function is kept exact by these tests.  Here: the
host build of the source over all 32768 indices and both roles, the index it reaches, and one run under the address and undefined-behaviour sanitizers in a
stand-alone program (no GPU, nothing preloaded).  The device build is checked by tests/test_gpu_reward_arith.py."""
import ctypes as C
import shutil
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from as_cops_and_thieves_amd import _native as nat
from as_cops_and_thieves_amd import tables
from as_cops_and_thieves_amd.constants import DEFAULT_SENSOR

ROOT = Path(__file__).resolve().parents[1]
EXCEPTION_CAP = 8   # most isolated indices per role an exception list may serve (there is no list: the arithmetic matches without one)


def _f16_bits(x: float) -> int:
    return int(np.array([x], np.float64).astype(np.float16).view(np.uint16)[0])


def _sensor_bounds():
    """f16 bits of ray_length + ray_radius -- no sighting can be further away -- of the default sensor and of the sensors the 64- and 90-ray configurations carry"""
    from as_cops_and_thieves_amd.config import SimConfig
    sensors = [DEFAULT_SENSOR, SimConfig(n_envs=1, n_rays=64).sensor, SimConfig(n_envs=1, n_rays=90).sensor]
    assert {s.num_rays for s in sensors} >= {64, 90}
    return [_f16_bits(s.ray_length + s.ray_radius) for s in sensors]


@pytest.fixture(scope="module")
def host_eval():
    L = nat.lib()
    cop, thief = tables.cop_reward_lut(), tables.thief_reward_lut()
    out = np.zeros((2, 32768), np.float32)
    m = L.cat_reward_arith_host(cop.ctypes.data_as(C.c_void_p), thief.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    return m, out, cop, thief


def test_host_build_equals_both_tables_up_to_reward_arith_max(host_eval):
    m, out, cop, thief = host_eval
    print("reward_arith_max", m, "sensor bounds", _sensor_bounds())
    assert m >= max(_sensor_bounds())
    assert np.array_equal(out[0, :m + 1].view(np.uint32), cop[:m + 1].view(np.uint32))
    assert np.array_equal(out[1, :m + 1].view(np.uint32), thief[:m + 1].view(np.uint32))
    # the scan stops at the FIRST mismatch of either role
    if m < 32767:
        assert out[0, m + 1].view(np.uint32) != cop[m + 1].view(np.uint32) or out[1, m + 1].view(np.uint32) != thief[m + 1].view(np.uint32)


def test_every_finite_distance_and_infinity_match(host_eval):
    """all of 0 .. 0x7C00 (every finite float16 and +inf); what is left above are the NaN patterns, which no distance takes"""
    m, out, cop, thief = host_eval
    assert m >= 0x7C00
    for role, lut in ((0, cop), (1, thief)):
        bad = np.nonzero(out[role, :0x7C01].view(np.uint32) != lut[:0x7C01].view(np.uint32))[0]
        assert len(bad) <= EXCEPTION_CAP and len(bad) == 0, bad[:16]


def test_other_tables_switch_the_arithmetic_off():
    L = nat.lib()
    cop, thief = tables.cop_reward_lut(), tables.thief_reward_lut()
    other = cop.copy()
    other[0] = np.float32(0.25)
    assert L.cat_reward_arith_host(other.ctypes.data_as(C.c_void_p), thief.ctypes.data_as(C.c_void_p), None) == -1
    other = thief.copy()
    other[1000] = np.float32(0.25)
    assert L.cat_reward_arith_host(cop.ctypes.data_as(C.c_void_p), other.ctypes.data_as(C.c_void_p), None) == 999
    assert L.cat_reward_arith_host(None, None, None) == -1


MAIN = r"""
#include <cstdio>
#include <vector>
#include "cat_sim_reward.h"
int main(int argc, char **argv)
{
    std::vector<float> lut(2 * 32768);
    FILE *f = fopen(argv[1], "rb");
    if (!f || fread(lut.data(), 4, lut.size(), f) != lut.size()) return 2;
    fclose(f);
    unsigned long long sum = 0;   // every index, NaN patterns included, through every conversion
    for (unsigned i = 0; i < 32768; i++) sum += reward_arith_f16(true, i) + 3ull * reward_arith_f16(false, i);
    printf("%d %llu\n", reward_arith_scan(lut.data(), lut.data() + 32768), sum);
    return 0;
}
"""


def test_stand_alone_program_under_sanitizers(tmp_path, host_eval):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    (tmp_path / "main.cpp").write_text(MAIN)
    m, _, cop, thief = host_eval
    (tmp_path / "luts.bin").write_bytes(cop.tobytes() + thief.tobytes())
    exe = tmp_path / "reward_main"
    subprocess.run([cxx, "-O1", "-g", "-ffp-contract=off", "-fsanitize=undefined,address", "-fno-sanitize-recover=all",
                    f"-I{ROOT / 'as_cops_and_thieves_amd' / 'csrc'}", "-o", str(exe), str(tmp_path / "main.cpp")], check=True)
    res = subprocess.run([str(exe), str(tmp_path / "luts.bin")], capture_output=True, text=True)
    sys.stdout.write(res.stdout + res.stderr)
    assert res.returncode == 0, res.stderr
    assert int(res.stdout.split()[0]) == m       # a plain C++ build of the header agrees with the library's host build
