// cat_learn_common.h -- what the translation units of libcat_learn.so (cat_{lstm,trunk,ppo,dense,rollout,render,episodes,act}.hip)
// share: the rules that must agree bit for bit between kernels, and the host boilerplate of every entry.  Internal: not part of
// the C ABI (include/ has that).  Everything is in the anonymous namespace, so each translation unit keeps its own copy -- in
// particular its own thread-local error buffer: cat_x_last_error() of one module never sees another module's failure.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <stdint.h>
#include <stdio.h>

namespace {

using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
using bf16x4 = __attribute__((ext_vector_type(4))) __bf16;
using f32x4 = __attribute__((ext_vector_type(4))) float;
using s16x4 = __attribute__((ext_vector_type(4))) short;

// ---- the LSTM's activations: the act kernel's state follows the window kernel's only while both use these
__device__ __forceinline__ float sigmoidf(float x) { return __builtin_amdgcn_rcpf(1.0f + __expf(-x)); }
__device__ __forceinline__ float tanh_fast(float x) { return 1.0f - 2.0f * __builtin_amdgcn_rcpf(1.0f + __expf(2.0f * x)); }

// ---- the categorical distribution over the 4 actions, from fp32 logits: unnormalised masses e_j = exp(z_j - zmax) and their sum in
// the order e0, e1, e2, e3 (rollout sampling, the fused act tick and the PPO loss all start here)
struct Cat4 {
    float zmax, e0, e1, e2, e3, sum;
};
__device__ __forceinline__ Cat4 cat4_masses(const f32x4 z)
{
    Cat4 m;
    m.zmax = fmaxf(fmaxf(z[0], z[1]), fmaxf(z[2], z[3]));
    m.e0 = __expf(z[0] - m.zmax); m.e1 = __expf(z[1] - m.zmax); m.e2 = __expf(z[2] - m.zmax); m.e3 = __expf(z[3] - m.zmax);
    m.sum = 0.f;
    m.sum += m.e0; m.sum += m.e1; m.sum += m.e2; m.sum += m.e3;
    return m;
}
// the draw: inverse CDF on the unnormalised masses
__device__ __forceinline__ int cat4_draw(const Cat4 &m, float uniform)
{
    const float u = uniform * m.sum;
    return (u >= m.e0) + (u >= m.e0 + m.e1) + (u >= m.e0 + m.e1 + m.e2);
}
// The log-probability exists in TWO forms that round differently, on purpose: what the sampling sites record as old_logp
// (z_act - zmax - log sum) and what the loss subtracts from every logit (lse = zmax + log sum).  Merging them would change the
// bits of old_logp or of the loss, and with them every ratio of the first epoch: keep both.
__device__ __forceinline__ float cat4_sampled_logp(const Cat4 &m, float z_act) { return z_act - m.zmax - __logf(m.sum); }
__device__ __forceinline__ float cat4_loss_lse(const Cat4 &m) { return m.zmax + __logf(m.sum); }

// ---- one element of a policy's observation row: the env core's f16 distance / u8 type times the configured scale, as bf16
__device__ __forceinline__ __bf16 obs_scaled(__half v, float scale) { return (__bf16)(__half2float(v) * scale); }
__device__ __forceinline__ __bf16 obs_scaled(uint8_t v, float scale) { return (__bf16)((float)v * scale); }

// ---- host side.  Every include/cat_*.h of the library uses these three codes (each .hip file asserts it for its own).
constexpr int LEARN_OK = 0, LEARN_ERR_BAD_ARG = -1, LEARN_ERR_HIP = -2;
#define CAT_LEARN_CODES(P) static_assert(P##_OK == LEARN_OK && P##_ERR_BAD_ARG == LEARN_ERR_BAD_ARG && P##_ERR_HIP == LEARN_ERR_HIP, "error codes")

thread_local char g_err[256] = "";
inline int fail(int code, const char *msg)
{
    snprintf(g_err, sizeof g_err, "%s", msg);
    return code;
}
inline int fail(int code, const char *who, const char *msg)
{
    snprintf(g_err, sizeof g_err, "%s: %s", who, msg);
    return code;
}
// after the launches of an entry: 0, or LEARN_ERR_HIP with the runtime's message (behind "who: " where given)
inline int launched(const char *who = nullptr)
{
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return LEARN_OK;
    return who ? fail(LEARN_ERR_HIP, who, hipGetErrorString(e)) : fail(LEARN_ERR_HIP, hipGetErrorString(e));
}
// the agent columns of G stacked policies in an [N][A] buffer
inline bool agents_ok(const int32_t *agent, int G, int A)
{
    for (int g = 0; g < G; ++g)
        if (agent[g] < 0 || agent[g] >= A) return false;
    return true;
}

}   // namespace
