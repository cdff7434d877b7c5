// cat_sim_reward.h -- the non-terminal rewards (cop.py:63-72, thief.py:65-66) as arithmetic: what tables.py tabulates, restated so that the
// device computes the value instead of fetching it.  Included by cat_sim.hip after cat_sim_common.h (device build: the hardware conversions) and, on its
// own, by any plain C++ program (host build: integer conversions): the arithmetic between the conversions is the same source for both.
//
// tables.py defines both tables as chains of float16 operations on the float16 distance d; h(x) = the exact value rounded once to float16:
//   cop    h(h(-0.02) + h(1.5 * h(exp(h(h(-d) / 50)))))
//   thief  h(h(tanh(h(h(d - 100) / 50))) / 10)
// Every link but exp / tanh is an exact f64 operation followed by ONE rounding, or can be made one:
//   * d - 100, 1.5 * e and h(-0.02) + m are exact in f64 (and in f32: float16 operands, at most 24 significant bits);
//   * x / 50 and w / 10 are evaluated as x * 0.02 and w * 0.1.  The quotient of a float16 by 50 (by 10) lies no closer than 2^-18 (relative) to a
//     float16 rounding boundary -- a boundary has 12 significant bits, x has 11 and 25 (5) is odd, so x - 50 * boundary is a non-zero multiple of the
//     smaller unit in the last place of the two -- while product and correctly rounded quotient differ by 2^-52: they round to the same float16.
// exp and tanh cannot be exact; they need not be: their float16 roundings are right whenever the f64 approximation is on the same side of every float16
// boundary as the true value.  Nothing here ASSUMES that: reward_arith_scan evaluates this function over all 32768 distances and both roles against a pair of tables and
// returns the largest index below which everything agrees (cat_reward_arith_host, cat_reward_arith_max; with tables.py's tables: 0x7C00, every finite
// distance and infinity -- what is left are the NaN patterns).
// STATUS: the kernels do NOT call it.  Built into rewards_and_positions for distances up to reward_arith_max it was bit-identical and slower (labyrinth 2v1 x4096,
// 30.7 against 30.2 us per launch: ~150 dependent f64 instructions on a slot's last link cost more than the cold table line they replace), so the
// kernels load from the tables as before.  Kept (host side and tests only; nothing of it is in the device structures): this function with its host build, the scan, cat_debug_reward_table (the device build over every index) and their
// tests -- the exact restatement a fused or table-free variant would start from.
//
// One exponential serves both roles (a wave's lanes hold cops and thieves: no divergent transcendental): the cop takes exp(t), t <= 0; the thief takes
// tanh(v) = sign(v) * (1 - 2 / (exp(2|v|) + 1)).  The smallest non-zero |v| is 0.00125, so the cancellation in 1 - 2 / (..) leaves ~43 of 53 bits.
// exp(x), |x| <= 40 after clamping (exp(-40) rounds to float16 zero like every smaller value; tanh is 1.0 in f64 from |v| = 20 on): k = nearest integer to
// x / ln 2, r = x - k * ln 2 with ln 2 in two parts (k * ln2_hi exact: ln2_hi has 32 trailing zero bits), |r| <= 0.3466, Taylor polynomial of degree 11
// (next term 0.3466^12 / 12! = 6e-15), scaled by 2^k through the exponent field (k in [-58, 58], the polynomial in [0.70, 1.42]: no subnormals).
// Only f64 + - * / (IEEE, contraction off as everywhere in this translation unit), comparisons / selects, integer operations and the float16 conversions.
#ifndef CAT_SIM_REWARD_H
#define CAT_SIM_REWARD_H

#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define CAT_RA_FN __host__ __device__ inline
#else
#define CAT_RA_FN inline
#endif

// ---- float16 conversions of the host build (integer arithmetic; the device build uses v_cvt_*)
inline unsigned ra_host_f64_to_f16(double x)   // round to nearest even, subnormals, overflow to infinity
{
    uint64_t b;
    std::memcpy(&b, &x, 8);
    const unsigned sign = (unsigned)(b >> 48) & 0x8000u;
    const int e = (int)((b >> 52) & 0x7FFu), E = e - 1023;
    uint64_t m = b & ((1ull << 52) - 1);
    if (e == 0x7FF) return sign | 0x7C00u | (m ? 0x200u : 0u);
    if (E > 15) return sign | 0x7C00u;
    if (E < -25) return sign;
    m |= 1ull << 52;
    const int shift = E >= -14 ? 42 : 42 + (-14 - E);   // 42 .. 53 bits dropped
    uint64_t q = m >> shift;
    const uint64_t rem = m & ((1ull << shift) - 1), half = 1ull << (shift - 1);
    if (rem > half || (rem == half && (q & 1))) q++;
    if (E >= -14) return sign | (((unsigned)(E + 14) << 10) + (unsigned)q);   // a carry out of the significand moves the exponent (up to infinity) by itself
    return sign | (unsigned)q;
}
inline double ra_host_f16_to_f64(unsigned h)
{
    const unsigned e = (h >> 10) & 31u, m = h & 1023u;
    uint64_t b;
    if (e == 0) {
        const double v = (double)m * (1.0 / 16777216.0);   // m * 2^-24, exact
        return (h & 0x8000u) ? -v : v;
    }
    if (e == 31) b = 0x7FF0000000000000ull | ((uint64_t)m << 42);
    else b = ((uint64_t)(e - 15 + 1023) << 52) | ((uint64_t)m << 42);
    b |= (uint64_t)(h & 0x8000u) << 48;
    double v;
    std::memcpy(&v, &b, 8);
    return v;
}

CAT_RA_FN unsigned ra_to_f16(double x)           // any f64 -> float16 bits, one rounding
{
#if defined(__HIP_DEVICE_COMPILE__)
    return f64_to_f16(x);
#else
    return ra_host_f64_to_f16(x);
#endif
}
CAT_RA_FN unsigned ra_to_f16_via_f32(double x)   // the same for a value that an f32 holds exactly
{
#if defined(__HIP_DEVICE_COMPILE__)
    return f32_to_f16((float)x);
#else
    return ra_host_f64_to_f16(x);
#endif
}
CAT_RA_FN double ra_from_f16(unsigned h)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return (double)f16_to_f32(h);
#else
    return ra_host_f16_to_f64(h);
#endif
}
CAT_RA_FN double ra_scale_pow2(double p, int k)  // p * 2^k for a normal p whose scaled value stays normal
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __hiloint2double(__double2hiint(p) + (k << 20), __double2loint(p));
#else
    int64_t b;
    std::memcpy(&b, &p, 8);
    b += (int64_t)k * ((int64_t)1 << 52);
    std::memcpy(&p, &b, 8);
    return p;
#endif
}

// The reward of a cop (is_cop) / thief whose nearest wanted sighting is at the float16 distance with bits d16 (0 .. 0x7FFF), as float16 bits.
CAT_RA_FN unsigned reward_arith_f16(bool is_cop, unsigned d16)
{
    const double d = ra_from_f16(d16 & 0x7FFFu);
    // cop: t = h(-d / 50);  thief: u = h(d - 100), v = h(u / 50)
    const double u = ra_from_f16(ra_to_f16_via_f32(d - 100.0));
    const double num = is_cop ? -d : u;
    const double tv = ra_from_f16(ra_to_f16(num * 0.02));
    // the shared exponential of x = t (cop, <= 0) or 2|v| (thief, >= 0); the selects also take a NaN to -40
    const double av = tv < 0.0 ? -tv : tv;
    double x = is_cop ? tv : av + av;
    x = x > -40.0 ? x : -40.0;
    x = x < 40.0 ? x : 40.0;
    const double kd = (x * 1.4426950408889634 + 6755399441055744.0) - 6755399441055744.0;   // nearest integer (2^52 + 2^51)
    const int k = (int)kd;
    const double r = (x - kd * 6.93147180369123816490e-01) - kd * 1.90821492927058770002e-10;
    double p = 1.0 / 39916800.0;
    p = p * r + 1.0 / 3628800.0;
    p = p * r + 1.0 / 362880.0;
    p = p * r + 1.0 / 40320.0;
    p = p * r + 1.0 / 5040.0;
    p = p * r + 1.0 / 720.0;
    p = p * r + 1.0 / 120.0;
    p = p * r + 1.0 / 24.0;
    p = p * r + 1.0 / 6.0;
    p = p * r + 0.5;
    p = p * r + 1.0;
    p = p * r + 1.0;
    const double ex = ra_scale_pow2(p, k);
    // cop: e = h(exp t), m = h(1.5 e), reward = h(h(-0.02) + m)
    const double e = ra_from_f16(ra_to_f16(ex));
    const double m = ra_from_f16(ra_to_f16_via_f32(1.5 * e));
    const double cop = -0.0200042724609375 + m;   // float16(-0.02), exactly
    // thief: w = h(tanh v), reward = h(w / 10)
    const double th = 1.0 - 2.0 / (ex + 1.0);
    const double w = ra_from_f16(ra_to_f16(tv < 0.0 ? -th : th));
    const double thief = w * 0.1;
    return is_cop ? ra_to_f16_via_f32(cop) : ra_to_f16(thief);
}

// Host only: the largest index m such that reward_arith_f16 equals both tables (f32 values of float16s, 32768 entries each) at every index <= m; -1 if none.
inline int reward_arith_scan(const float *cop_lut, const float *thief_lut)
{
    for (int i = 0; i < 32768; i++) {
        const float c = (float)ra_host_f16_to_f64(reward_arith_f16(true, (unsigned)i)), t = (float)ra_host_f16_to_f64(reward_arith_f16(false, (unsigned)i));
        if (std::memcmp(&c, &cop_lut[i], 4) != 0 || std::memcmp(&t, &thief_lut[i], 4) != 0) return i - 1;
    }
    return 32767;
}

#endif
