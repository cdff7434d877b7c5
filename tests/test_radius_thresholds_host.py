"""The radius tests without the square root (csrc/cat_sim_radius.h), host side: the kernels compare a squared distance against one double per
test instead of taking its root,

    capture   sqrt(x) < termination_radius             ->   x <  X
    near      sqrt(x) - agent_radius <= ray_radius     ->   x <= E

and for every double x within 64 ulps either side of the threshold the old predicate (NumPy's sqrt: IEEE, correctly rounded, like the oracle's)
and the new one must agree -- for the radii of the configuration every preset runs with (constants.py) and for others whose squares are not
representable.  Far from the threshold the two agree by monotonicity, which the sweep also samples.  The header is a plain C++ header: a small
program of its own runs the same sweep under the address and undefined-behaviour sanitizers."""
import ctypes as C
import shutil
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from as_cops_and_thieves_amd import _native
from as_cops_and_thieves_amd.config import SimConfig

ROOT = Path(__file__).resolve().parent.parent
ULPS = 64

DEFAULT = SimConfig()
# (termination radius, agent radius, ray radius): the shipped configuration, the constants the reader test uses, and radii whose squares round
RADII = [(DEFAULT.termination_radius, DEFAULT.agent_radius, DEFAULT.ray_radius), (21.0, 7.5, 1.5), (20.0 / 3.0, 5.0 / 3.0, 0.1), (10.0 * 2.0 ** 0.5, 3.3, 0.7),
         (1e-3, 1e-4, 1e-5), (1e6, 123456.789, 0.001), (1.0, 0.0, 1.0), (400.0, 5.0, 0.0)]


def thresholds(term, rc, r2):
    out = (C.c_double * 2)()
    assert _native.lib().cat_radius_thresholds_host(term, rc, r2, out) == 0
    return float(out[0]), float(out[1])


def around(x, ulps=ULPS):
    """every non-negative double within `ulps` of x (bit patterns of the non-negative doubles are ordered like their values), +inf at most"""
    b = int(np.float64(max(x, 0.0)).view(np.uint64))
    lo, hi = max(b - ulps, 0), min(b + ulps, 0x7FF0000000000000)
    return np.arange(lo, hi + 1, dtype=np.uint64).view(np.float64)


def old_capture(x, term):
    return np.sqrt(x) < term


def old_near(x, rc, r2):
    return np.sqrt(x) - rc <= r2


@pytest.mark.parametrize("term,rc,r2", RADII)
def test_old_and_new_predicate_agree_around_the_threshold(term, rc, r2):
    X, E = thresholds(term, rc, r2)
    with np.errstate(over="ignore", invalid="ignore"):
        far = np.array([0.0, 1e-300, 0.25 * term * term, 4.0 * term * term, 0.25 * (rc + r2) ** 2, 4.0 * (rc + r2) ** 2, 1e300, np.inf, np.nan])
        xs = np.concatenate([around(X), around(term * term), far])
        assert np.array_equal(old_capture(xs, term), xs < X), (term, X)
        xs = np.concatenate([around(E), around((rc + r2) ** 2), far])
        assert np.array_equal(old_near(xs, rc, r2), xs <= E), (rc, r2, E)
    # the thresholds are where they should be: within a few ulps of the squared radius, and the predicates do change there
    assert abs(X - term * term) <= 4 * np.spacing(term * term) and abs(E - (rc + r2) ** 2) <= 8 * np.spacing((rc + r2) ** 2)
    assert old_capture(np.nextafter(X, 0.0), term) and not old_capture(X, term)
    assert old_near(E, rc, r2) and not old_near(np.nextafter(E, np.inf), rc, r2)


def test_degenerate_radii():
    inf, nan = float("inf"), float("nan")
    for term, rc, r2 in [(2.0 ** -600, 2.0 ** -601, 2.0 ** -601), (1e160, 1e159, 1e159), (0.0, 0.0, 0.0), (-1.0, -1.0, -1.0), (nan, 1.0, 1.0), (inf, 1.0, inf),
                         (1.0, nan, 1.0), (1.0, 1.0, nan), (1.0, 5.0, -6.0), (1.0, -inf, 1.0), (5e-324, 0.0, 5e-324), (1.7e308, 1.7e308, 1.7e308)]:
        X, E = thresholds(term, rc, r2)
        xs = np.concatenate([around(0.0), around(1.0), around(X), around(E), [1e300, inf, nan]])
        with np.errstate(over="ignore", invalid="ignore"):
            assert np.array_equal(old_capture(xs, term), xs < X), (term, X)
            assert np.array_equal(old_near(xs, rc, r2), xs <= E), (rc, r2, E)


def test_the_scripted_scenario_sits_on_the_thresholds():
    """tests/radius_cases.py (run on the GPU by tests/test_gpu_radius_thresholds.py): exact squared distances, the oracle's results change there,
    and the library's thresholds are the ones NumPy finds"""
    from tests import radius_cases as rc
    sc = rc.scenario()
    sc.check()
    assert thresholds(sc.cfg.termination_radius, sc.cfg.agent_radius, sc.cfg.ray_radius) == (sc.X, sc.E)


MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include "cat_sim_radius.h"
static uint64_t bits_of(double d) { uint64_t u; memcpy(&u, &d, sizeof u); return u; }
int main(int argc, char **argv)
{
    // argv: triples (termination radius, agent radius, ray radius).  Prints the two thresholds of each and the number of disagreements
    // between the predicates with and without the square root within 64 ulps either side of the thresholds (must be 0).
    long bad = 0;
    for (int a = 1; a + 2 < argc; a += 3) {
        const double term = strtod(argv[a], nullptr), rc = strtod(argv[a + 1], nullptr), r2 = strtod(argv[a + 2], nullptr);
        const double X = radius_lt_threshold(term), E = radius_le_threshold(rc, r2);
        for (int side = 0; side < 2; side++) {
            const double mid = side ? E : X;
            if (!(mid >= 0.0)) continue;
            const uint64_t b = bits_of(mid), lo = b > 64 ? b - 64 : 0, hi = b + 64 < kRadiusInfBits ? b + 64 : kRadiusInfBits;
            for (uint64_t u = lo; u <= hi; u++) {
                const double x = radius_from_bits(u), s = std::sqrt(x);
                if ((s < term) != (x < X)) bad++;
                const double d = s - rc;
                if ((d <= r2) != (x <= E)) bad++;
            }
        }
        printf("%a %a\n", X, E);
    }
    printf("%ld\n", bad);
    return bad ? 1 : 0;
}
"""


def test_stand_alone_program_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    (tmp_path / "main.cpp").write_text(MAIN)
    exe = tmp_path / "radius_main"
    subprocess.run([cxx, "-O1", "-g", "-ffp-contract=off", "-fsanitize=undefined,address", "-fno-sanitize-recover=all",
                    f"-I{ROOT / 'as_cops_and_thieves_amd' / 'csrc'}", "-o", str(exe), str(tmp_path / "main.cpp")], check=True)
    cases = RADII + [(0.0, 0.0, 0.0), (-1.0, 5.0, -6.0), (float("inf"), 1.0, float("inf")), (float("nan"), float("nan"), 1.0)]
    res = subprocess.run([str(exe)] + [repr(float(v)) for tr in cases for v in tr], capture_output=True, text=True)
    sys.stdout.write(res.stdout + res.stderr)
    assert res.returncode == 0, res.stderr
    lines = res.stdout.split("\n")
    assert lines[len(cases)] == "0"
    for tr, ln in zip(cases, lines):                      # a plain C++ build of the header agrees with the library's host build
        X, E = (float.fromhex(v) if "0x" in v else float(v) for v in ln.split())
        got = thresholds(*tr)
        assert (X, E) == got or (X != X and got[0] != got[0]), (tr, ln, got)
