// cat_sim_radius.h -- radius tests without the square root (host only, no device, no other header of the env core: a plain C++ program may include it).
//
// The kernels' two radius tests on a squared distance x = dx * dx + dy * dy (never negative, perhaps NaN or +inf):
//   capture   sqrt(x) < term_radius              BaseEnv._termination_criterion (base_env.py:521-554), termination_captured
//   near      sqrt(x) - rc <= ray_radius         [CP cpCircleShapePointQuery], agent_setup
// A correctly rounded square root is monotone (x <= y gives sqrt(x) <= sqrt(y)), and so is the rounded subtraction of a constant: each predicate is
// true on an initial stretch of the non-negative doubles and false behind it.  The non-negative doubles are ordered like their bit patterns, so the
// end of the stretch is found by bisection on the pattern with the predicate itself (the host's sqrt is IEEE's; the device's is checked against it bit
// for bit by tests/test_gpu_parity.py::test_device_arithmetic_is_ieee_exact), and the kernels compare x against that one double:
//   capture   x <  radius_lt_threshold(term_radius)
//   near      x <= radius_le_threshold(rc, ray_radius)
// Both sides are false for a NaN x.  The oracle keeps the square root.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

inline double radius_from_bits(uint64_t u) { double d; memcpy(&d, &u, sizeof d); return d; }
constexpr uint64_t kRadiusInfBits = 0x7FF0000000000000ull;

// the smallest non-negative double X (+inf included) with !(sqrt(X) < r):  sqrt(x) < r  <=>  x < X  for every x >= 0.  (r <= 0 or NaN: 0 -- never true)
inline double radius_lt_threshold(double r)
{
    uint64_t lo = 0, hi = kRadiusInfBits;   // sqrt(+inf) < r is false for every r: the answer lies in [lo, hi]
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (std::sqrt(radius_from_bits(mid)) < r) lo = mid + 1; else hi = mid;
    }
    return radius_from_bits(lo);
}

// the largest non-negative double E (+inf included) with sqrt(E) - rc <= r2:  sqrt(x) - rc <= r2  <=>  x <= E  for every x >= 0.  (none: -1 -- never true)
inline double radius_le_threshold(double rc, double r2)
{
    auto holds = [&](uint64_t u) { const double s = std::sqrt(radius_from_bits(u)); const double d = s - rc; return d <= r2; };
    if (!holds(0)) return -1.0;
    uint64_t lo = 0, hi = kRadiusInfBits;   // holds(lo) throughout
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo + 1) / 2;
        if (holds(mid)) lo = mid; else hi = mid - 1;
    }
    return radius_from_bits(lo);
}
