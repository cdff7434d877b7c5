// cat_ppo.hip -- libcat_learn.so, part 3 of 8: PPO loss + gradient, the optimiser step (each also with its hyper-parameters read from
// device memory), the schedule rule on those, the GAE scan (plain and over a normalised critic) and the running f64 moments of the
// returns (include/cat_ppo.h).
//
// The first two are a few flops per element over at most a few million elements: as library elementwise kernels they are
// ~110 launches of ~5 us per minibatch step inside the replayed HIP graph (each a dependent graph node), about a tenth
// of the step.  Here: one launch for the loss, its four per-agent statistics and the gradient w.r.t. logits and
// values (the derivative is written out analytically, no autograd graph for this part), and two launches for the
// gradient-norm clip + masked Adam + bf16 refresh.  Reductions are two-stage (per-block partial sums, added up by the
// consumer), never a semaphore-style single-pass reduction.
#include "cat_learn_common.h"
#include "cat_ppo.h"
#include "cat_rollout.h"
#include <type_traits>

namespace {

CAT_LEARN_CODES(CAT_PPO);
constexpr int BLOCK = 256;

// sum of v over the block; valid in thread 0
template <int N>
__device__ __forceinline__ void block_sum(float (&v)[N], float *lds)
{
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v[i] += __shfl_down(v[i], off, 64);
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    if (l == 0)
#pragma unroll
        for (int i = 0; i < N; ++i) lds[w * N + i] = v[i];
    __syncthreads();
    if (threadIdx.x == 0)
#pragma unroll
        for (int i = 0; i < N; ++i) v[i] = lds[i] + lds[N + i] + lds[2 * N + i] + lds[3 * N + i];
}

// Args = cat_ppo_loss_dev: the ratio clip and the entropy scale are agent g's words of the hyper block in device memory (a replayed
// graph sees what the block holds then); nothing else differs.
template <class Args>
__global__ __launch_bounds__(BLOCK) void ppo_loss_kernel(const Args a)
{
    constexpr bool DEV = std::is_same<Args, cat_ppo_loss_dev>::value;
    __shared__ float lds[4 * 4];
    const int g = blockIdx.y, M = a.M;
    const size_t base = (size_t)g * M;
    float ratio_clip = a.ratio_clip, entropy_scale = a.entropy_scale;
    if constexpr (DEV) {
        const float *h = a.hyper + (size_t)g * CAT_PPO_HYPER_STRIDE;
        ratio_clip = h[CAT_PPO_HYPER_RATIO_CLIP]; entropy_scale = h[CAT_PPO_HYPER_ENTROPY];
    }
    const float inv_m = 1.0f / (float)M, lo = 1.0f - ratio_clip, hi = 1.0f + ratio_clip;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int i = blockIdx.x * BLOCK + threadIdx.x; i < M; i += gridDim.x * BLOCK) {
        const size_t s = base + i;
        const f32x4 z = __builtin_convertvector(*(const bf16x4 *)((const __bf16 *)a.logits + 4 * s), f32x4);
        const Cat4 m = cat4_masses(z);
        const float e[4] = {m.e0, m.e1, m.e2, m.e3}, lse = cat4_loss_lse(m), rs = 1.0f / m.sum;
        float lp[4], p[4];
        float ent = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) { lp[j] = z[j] - lse; p[j] = e[j] * rs; ent -= p[j] * lp[j]; }
        const int act = (int)a.actions[s] & 3;
        const float logp = lp[act], d = logp - a.old_logp[s], ratio = __expf(d), adv = a.adv[s];
        const float s1 = adv * ratio, s2 = adv * fminf(fmaxf(ratio, lo), hi);
        const bool inside = ratio >= lo && ratio <= hi;
        // d min(s1, s2) / d logp: inside the clip range both branches are the same function; outside, the clipped
        // branch is constant, so the gradient flows only when the unclipped branch is the smaller one
        const float dsurr = (inside || s1 < s2) ? s1 : 0.0f;           // adv * ratio * (d ratio / d logp = ratio ... ) = s1
        acc[0] += fminf(s1, s2);
        const float v = (float)((const __bf16 *)a.values)[s], dv = v - a.ret[s];
        acc[1] += dv * dv;
        acc[2] += ent;
        acc[3] += (ratio - 1.0f) - d;
        f32x4 dz;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float onehot = (j == act) ? 1.0f : 0.0f;
            dz[j] = inv_m * (-dsurr * (onehot - p[j]) + entropy_scale * p[j] * (lp[j] + ent));
        }
        *(bf16x4 *)((__bf16 *)a.d_logits + 4 * s) = __builtin_convertvector(dz, bf16x4);
        ((__bf16 *)a.d_values)[s] = (__bf16)(2.0f * a.value_scale * inv_m * dv);
    }
    block_sum(acc, lds);
    if (threadIdx.x == 0) {
        float *out = a.partial + ((size_t)g * gridDim.x + blockIdx.x) * 4;
        out[0] = acc[0]; out[1] = acc[1]; out[2] = acc[2]; out[3] = acc[3];
    }
}

template <class Args>
__global__ __launch_bounds__(BLOCK) void grad_norm_kernel(const Args a)
{
    __shared__ float lds[4];
    const int g = blockIdx.y, P = a.P;
    const float *ar = a.ar + (size_t)g * (P + 1), *col = a.col_train + (size_t)g * P;
    float acc[1] = {0.f};
    for (int i = blockIdx.x * BLOCK + threadIdx.x; i < P; i += gridDim.x * BLOCK) {
        const float x = ar[i] * col[i];
        acc[0] += x * x;
    }
    block_sum(acc, lds);
    if (threadIdx.x == 0) a.norm_partial[(size_t)g * gridDim.x + blockIdx.x] = acc[0];
}

// Args = cat_ppo_adam_dev: the learning rate is agent g's word of the hyper block, and the thread that rewrites epoch_active[g] adds the
// minibatch's KL to the block's sum when the agent entered the step active (include/cat_ppo.h); nothing else differs.
template <class Args>
__global__ __launch_bounds__(BLOCK) void adam_kernel(const Args a)
{
    constexpr bool DEV = std::is_same<Args, cat_ppo_adam_dev>::value;
    __shared__ float lds[4];
    __shared__ float s_scale, s_active;
    const int g = blockIdx.y, P = a.P;
    float acc[1] = {0.f};
    for (int i = threadIdx.x; i < a.chunks; i += BLOCK) acc[0] += a.norm_partial[(size_t)g * a.chunks + i];
    block_sum(acc, lds);
    const float *ar = a.ar + (size_t)g * (P + 1);
    if (threadIdx.x == 0) {
        const float norm = sqrtf(acc[0]), kl = ar[P];
        s_scale = fminf(a.grad_norm_clip / (norm + 1e-6f), 1.0f);
        // the gate is idempotent (a 0/1 factor), so blocks that read epoch_active after block 0 rewrote it agree
        const float was = a.epoch_active[g];
        const float active = was * ((a.kl_threshold > 0.0f && !(kl <= a.kl_threshold)) ? 0.0f : 1.0f);
        s_active = active;
        if (blockIdx.x == 0) {
            if constexpr (DEV) {    // block 0 is the only writer of epoch_active[g], so ``was`` is the value the step was entered with
                if (was != 0.0f) {
                    float *h = a.hyper + (size_t)g * CAT_PPO_HYPER_STRIDE;
                    h[CAT_PPO_HYPER_KL_SUM] += kl; h[CAT_PPO_HYPER_KL_COUNT] += 1.0f;
                }
            }
            a.epoch_active[g] = active; a.kl_out[g] = kl;
        }
    }
    __syncthreads();
    float lr = a.lr;
    if constexpr (DEV) lr = a.hyper[(size_t)g * CAT_PPO_HYPER_STRIDE + CAT_PPO_HYPER_LR];
    const float scale = s_scale, active = s_active, b1 = a.beta1, b2 = a.beta2;
    const size_t row = (size_t)g * P;
    for (int i = blockIdx.x * BLOCK + threadIdx.x; i < P; i += gridDim.x * BLOCK) {
        const float col = a.col_train[row + i], gate = active * col;
        const float gr = ar[i] * col * scale;
        float m = a.m[row + i], v = a.v[row + i], st = a.steps[row + i], w = a.master[row + i];
        st += gate;
        m += gate * (1.0f - b1) * (gr - m);
        v += gate * (1.0f - b2) * (gr * gr - v);
        const float s = fmaxf(st, 1.0f);
        const float bc1 = 1.0f - powf(b1, s), bc2 = 1.0f - powf(b2, s);
        w -= gate * lr * (m / bc1) / (sqrtf(v / bc2) + a.eps);
        a.steps[row + i] = st; a.m[row + i] = m; a.v[row + i] = v; a.master[row + i] = w;
        if (a.lp) ((__bf16 *)a.lp)[row + i] = (__bf16)w;
    }
}

// a normalised critic output back in the returns' units: the product rounded, then the sum rounded (include/cat_ppo.h)
__device__ __forceinline__ float denormalised(float v, float mu, float sigma)
{
#pragma clang fp contract(off)
    const float p = v * sigma;
    return p + mu;
}

// one thread per (agent, env): the reverse scan of the rollout's T ticks; lanes = envs, so every access is coalesced.
// Args = cat_ppo_gae_scaled: every value read goes through denormalised() first, nothing else differs.
template <class Args>
__global__ __launch_bounds__(BLOCK) void gae_kernel(const Args a)
{
    constexpr bool SCALED = std::is_same<Args, cat_ppo_gae_scaled>::value;
    const int n = blockIdx.x * BLOCK + threadIdx.x, g = blockIdx.y;
    if (n >= a.N) return;
    float mu = 0.0f, sigma = 1.0f;
    if constexpr (SCALED) { mu = a.scale[2 * g]; sigma = a.scale[2 * g + 1]; }
    const auto value = [&](float v) { if constexpr (SCALED) return denormalised(v, mu, sigma); else return v; };
    const size_t col = (size_t)g * a.T * a.N + n;
    float last = 0.0f, nxt = value(a.last_values[(size_t)g * a.N + n]);
    const float gl = a.gamma * a.lambda;
    for (int t = a.T - 1; t >= 0; --t) {
        const size_t o = col + (size_t)t * a.N;
        const float nd = a.dones[(size_t)t * a.N + n] ? 0.0f : 1.0f, v = value(a.values[o]);
        const float delta = a.rewards[o] + a.gamma * nxt * nd - v;
        last = delta + gl * nd * last;
        a.adv[o] = last;
        a.ret[o] = last + v;
        nxt = v;
    }
}

// ---- running moments (include/cat_ppo.h has the order; every operation below is one rounded f64 operation)
constexpr int MOMENT_PER_THREAD = CAT_PPO_MOMENT_CHUNK / BLOCK;
static_assert(MOMENT_PER_THREAD * BLOCK == CAT_PPO_MOMENT_CHUNK && BLOCK == 256, "16 elements per thread, a 256-wide tree");

struct Moments {
    double n, mean, m2;
};

__device__ __forceinline__ Moments moments_merge(const Moments a, const Moments b)
{
#pragma clang fp contract(off)
    if (b.n == 0.0) return a;
    if (a.n == 0.0) return b;
    Moments r;
    r.n = a.n + b.n;
    const double delta = b.mean - a.mean, w = b.n / r.n;
    const double shift = delta * w;
    r.mean = a.mean + shift;
    const double sq = delta * delta, cross = a.n * w;
    const double corr = sq * cross;
    r.m2 = (a.m2 + b.m2) + corr;
    return r;
}

// s[0] = the halving-tree sum of the 256 threads' v; every thread returns it
__device__ __forceinline__ double tree_sum(double v, double *s)
{
    s[threadIdx.x] = v;
    __syncthreads();
    for (int stride = BLOCK / 2; stride > 0; stride >>= 1) {
        if ((int)threadIdx.x < stride) s[threadIdx.x] = s[threadIdx.x] + s[threadIdx.x + stride];
        __syncthreads();
    }
    const double total = s[0];
    __syncthreads();
    return total;
}

__global__ __launch_bounds__(BLOCK) void moments_chunk_kernel(const cat_ppo_moments_args a, const int chunks)
{
#pragma clang fp contract(off)
    __shared__ double s[BLOCK];
    const int c = blockIdx.x, g = blockIdx.y;
    const float *x = a.x + (size_t)g * a.M;
    const int first = c * CAT_PPO_MOMENT_CHUNK;                 // c < 65536 (checked by the entry): below 2^28
    const int count = min(CAT_PPO_MOMENT_CHUNK, a.M - first);
    float e[MOMENT_PER_THREAD];
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < MOMENT_PER_THREAD; ++j) {
        const int k = (int)threadIdx.x + BLOCK * j;
        e[j] = k < count ? x[(size_t)first + k] : 0.0f;
        if (k < count) acc = acc + (double)e[j];
    }
    const double n = (double)count, mean = tree_sum(acc, s) / n;
    acc = 0.0;
#pragma unroll
    for (int j = 0; j < MOMENT_PER_THREAD; ++j) {
        const int k = (int)threadIdx.x + BLOCK * j;
        if (k < count) {
            const double d = (double)e[j] - mean;
            const double dd = d * d;
            acc = acc + dd;
        }
    }
    const double m2 = tree_sum(acc, s);
    if (threadIdx.x == 0) {
        double *out = a.partial + ((size_t)g * chunks + c) * 3;
        out[0] = n; out[1] = mean; out[2] = m2;
    }
}

// one workgroup per agent: the halving tree over its chunk triples, in place in partial[g] (a pad triple is (0, 0, 0), which merge()
// passes over: t[i + stride] beyond the chunks leaves t[i] as it is); then the running state and the scale
__global__ __launch_bounds__(BLOCK) void moments_merge_kernel(const cat_ppo_moments_args a, const int chunks, const int P)
{
#pragma clang fp contract(off)
    const int g = blockIdx.x;
    double *t = a.partial + (size_t)g * chunks * 3;
    for (int stride = P / 2; stride > 0; stride >>= 1) {
        for (int i = threadIdx.x; i < stride && i + stride < chunks; i += BLOCK) {
            const double *pa = t + 3 * (size_t)i, *pb = t + 3 * (size_t)(i + stride);
            const Moments r = moments_merge(Moments{pa[0], pa[1], pa[2]}, Moments{pb[0], pb[1], pb[2]});
            t[3 * (size_t)i] = r.n; t[3 * (size_t)i + 1] = r.mean; t[3 * (size_t)i + 2] = r.m2;
        }
        __syncthreads();        // workgroup-scope release / acquire: the next level reads what this one stored
    }
    if (threadIdx.x != 0) return;
    const Moments batch{t[0], t[1], t[2]};
    if (a.batch_out) { double *o = a.batch_out + 3 * (size_t)g; o[0] = batch.n; o[1] = batch.mean; o[2] = batch.m2; }
    if (!a.state) return;
    double *st = a.state + 3 * (size_t)g;
    const Moments now = moments_merge(Moments{st[0], st[1], st[2]}, batch);
    st[0] = now.n; st[1] = now.mean; st[2] = now.m2;
    if (a.scale_out) {
        const bool empty = now.n == 0.0;
        a.scale_out[2 * g] = empty ? 0.0f : (float)now.mean;
        a.scale_out[2 * g + 1] = empty ? 1.0f : (float)sqrt(now.m2 / now.n);
    }
}

// ---- the schedule rule on the hyper block (include/cat_ppo.h has the order; every operation below is one rounded fp32 operation)
__device__ __forceinline__ float annealed(float x0, float x1, float progress)
{
#pragma clang fp contract(off)
    const float d = x1 - x0;
    const float p = d * progress;
    return x0 + p;
}

// one workgroup, thread g = agent g
__global__ __launch_bounds__(64) void schedule_kernel(const cat_ppo_schedule a)
{
#pragma clang fp contract(off)
    const int g = threadIdx.x;
    if (g >= a.G) return;
    float *h = a.hyper + (size_t)g * CAT_PPO_HYPER_STRIDE;
    if (a.mode & CAT_PPO_SCHED_ANNEAL) {
        if (a.anneal_mask & CAT_PPO_ANNEAL_LR) h[CAT_PPO_HYPER_LR] = annealed(a.lr0, a.lr1, a.progress);
        if (a.anneal_mask & CAT_PPO_ANNEAL_ENTROPY) h[CAT_PPO_HYPER_ENTROPY] = annealed(a.ent0, a.ent1, a.progress);
        if (a.anneal_mask & CAT_PPO_ANNEAL_RATIO_CLIP) h[CAT_PPO_HYPER_RATIO_CLIP] = annealed(a.clip0, a.clip1, a.progress);
    }
    if (a.mode & CAT_PPO_SCHED_KL) {
        const float hi = a.kl_target * a.kl_factor, lo = a.kl_target / a.kl_factor;
        const float count = h[CAT_PPO_HYPER_KL_COUNT];
        if (count > 0.0f && a.sched_active[g] != 0.0f) {
            const float kl = h[CAT_PPO_HYPER_KL_SUM] / count;
            float lr = h[CAT_PPO_HYPER_LR];
            if (kl > hi) lr = fmaxf(lr / a.lr_factor, a.lr_min);
            else if (kl < lo) lr = fminf(lr * a.lr_factor, a.lr_max);
            h[CAT_PPO_HYPER_LR] = lr;
        }
        h[CAT_PPO_HYPER_KL_SUM] = 0.0f; h[CAT_PPO_HYPER_KL_COUNT] = 0.0f;
    }
}

// the checks cat_ppo_loss_grad and cat_ppo_loss_grad_dev share
template <class Args>
int loss_checked(const Args *a, const char *who)
{
    if (!a || a->G <= 0 || a->G > 65535 || a->M <= 0 || a->chunks <= 0 || a->chunks > CAT_PPO_MAX_CHUNKS)
        return fail(CAT_PPO_ERR_BAD_ARG, who, "bad dimensions");
    if (!a->logits || !a->values || !a->actions || !a->old_logp || !a->adv || !a->ret || !a->d_logits || !a->d_values || !a->partial)
        return fail(CAT_PPO_ERR_BAD_ARG, who, "a required buffer is NULL");
    if (((uintptr_t)a->logits % 8) || ((uintptr_t)a->d_logits % 8))
        return fail(CAT_PPO_ERR_BAD_ARG, who, "logits must be 8-byte aligned");
    return CAT_PPO_OK;
}

template <class Args>
int adam_checked(const Args *a, const char *who)
{
    if (!a || a->G <= 0 || a->G > 65535 || a->P <= 0 || a->chunks <= 0 || a->chunks > CAT_PPO_MAX_CHUNKS)
        return fail(CAT_PPO_ERR_BAD_ARG, who, "bad dimensions");
    if (!a->ar || !a->col_train || !a->epoch_active || !a->m || !a->v || !a->steps || !a->master || !a->kl_out || !a->norm_partial)
        return fail(CAT_PPO_ERR_BAD_ARG, who, "a required buffer is NULL");
    return CAT_PPO_OK;
}

}   // namespace

extern "C" int cat_ppo_abi_version(void) { return CAT_PPO_ABI_VERSION; }
extern "C" const char *cat_ppo_last_error(void) { return g_err; }

extern "C" int cat_ppo_loss_grad(const cat_ppo_loss *a, void *stream)
{
    if (const int rc = loss_checked(a, "cat_ppo_loss_grad")) return rc;
    hipLaunchKernelGGL(ppo_loss_kernel<cat_ppo_loss>, dim3(a->chunks, a->G), dim3(BLOCK), 0, (hipStream_t)stream, *a);
    return launched();
}

extern "C" int cat_ppo_loss_grad_dev(const cat_ppo_loss_dev *a, void *stream)
{
    if (const int rc = loss_checked(a, "cat_ppo_loss_grad_dev")) return rc;
    if (!a->hyper) return fail(CAT_PPO_ERR_BAD_ARG, "cat_ppo_loss_grad_dev: hyper is NULL");
    hipLaunchKernelGGL(ppo_loss_kernel<cat_ppo_loss_dev>, dim3(a->chunks, a->G), dim3(BLOCK), 0, (hipStream_t)stream, *a);
    return launched();
}

extern "C" int cat_ppo_gae_scan(const cat_ppo_gae *a, void *stream)
{
    if (!a || a->G <= 0 || a->G > 65535 || a->T <= 0 || a->N <= 0) return fail(CAT_PPO_ERR_BAD_ARG, "cat_ppo_gae_scan: bad dimensions");
    if (!a->rewards || !a->values || !a->dones || !a->last_values || !a->adv || !a->ret)
        return fail(CAT_PPO_ERR_BAD_ARG, "cat_ppo_gae_scan: a required buffer is NULL");
    hipLaunchKernelGGL(gae_kernel<cat_ppo_gae>, dim3((a->N + BLOCK - 1) / BLOCK, a->G), dim3(BLOCK), 0, (hipStream_t)stream, *a);
    return launched();
}

extern "C" int cat_ppo_gae_scan_scaled(const cat_ppo_gae_scaled *a, void *stream)
{
    if (!a || a->G <= 0 || a->G > 65535 || a->T <= 0 || a->N <= 0) return fail(CAT_PPO_ERR_BAD_ARG, "cat_ppo_gae_scan_scaled: bad dimensions");
    if (!a->rewards || !a->values || !a->dones || !a->last_values || !a->adv || !a->ret || !a->scale)
        return fail(CAT_PPO_ERR_BAD_ARG, "cat_ppo_gae_scan_scaled: a required buffer is NULL");
    hipLaunchKernelGGL(gae_kernel<cat_ppo_gae_scaled>, dim3((a->N + BLOCK - 1) / BLOCK, a->G), dim3(BLOCK), 0, (hipStream_t)stream, *a);
    return launched();
}

extern "C" int cat_ppo_moment_chunks(int32_t M)
{
    return M <= 0 ? 0 : (int)(((int64_t)M + CAT_PPO_MOMENT_CHUNK - 1) / CAT_PPO_MOMENT_CHUNK);
}

extern "C" int cat_ppo_moments(const cat_ppo_moments_args *a, void *stream)
{
    if (!a || a->G <= 0 || a->G > 65535 || a->M <= 0) return fail(CAT_PPO_ERR_BAD_ARG, "cat_ppo_moments: bad dimensions");
    const int chunks = cat_ppo_moment_chunks(a->M);
    if (chunks > 65536) return fail(CAT_PPO_ERR_BAD_ARG, "cat_ppo_moments: M is above 65536 chunks of 4096 samples");
    if (!a->x || !a->partial) return fail(CAT_PPO_ERR_BAD_ARG, "cat_ppo_moments: a required buffer is NULL");
    if (a->scale_out && !a->state) return fail(CAT_PPO_ERR_BAD_ARG, "cat_ppo_moments: scale_out needs state");
    int P = 1;
    while (P < chunks) P <<= 1;
    hipLaunchKernelGGL(moments_chunk_kernel, dim3(chunks, a->G), dim3(BLOCK), 0, (hipStream_t)stream, *a, chunks);
    hipLaunchKernelGGL(moments_merge_kernel, dim3(a->G), dim3(BLOCK), 0, (hipStream_t)stream, *a, chunks, P);
    return launched();
}

extern "C" int cat_ppo_adam_step(const cat_ppo_adam *a, void *stream)
{
    if (const int rc = adam_checked(a, "cat_ppo_adam_step")) return rc;
    hipLaunchKernelGGL(grad_norm_kernel<cat_ppo_adam>, dim3(a->chunks, a->G), dim3(BLOCK), 0, (hipStream_t)stream, *a);
    hipLaunchKernelGGL(adam_kernel<cat_ppo_adam>, dim3(a->chunks, a->G), dim3(BLOCK), 0, (hipStream_t)stream, *a);
    return launched();
}

extern "C" int cat_ppo_adam_step_dev(const cat_ppo_adam_dev *a, void *stream)
{
    if (const int rc = adam_checked(a, "cat_ppo_adam_step_dev")) return rc;
    if (!a->hyper) return fail(CAT_PPO_ERR_BAD_ARG, "cat_ppo_adam_step_dev: hyper is NULL");
    hipLaunchKernelGGL(grad_norm_kernel<cat_ppo_adam_dev>, dim3(a->chunks, a->G), dim3(BLOCK), 0, (hipStream_t)stream, *a);
    hipLaunchKernelGGL(adam_kernel<cat_ppo_adam_dev>, dim3(a->chunks, a->G), dim3(BLOCK), 0, (hipStream_t)stream, *a);
    return launched();
}

extern "C" int cat_ppo_schedule_step(const cat_ppo_schedule *a, void *stream)
{
    const char *who = "cat_ppo_schedule_step";
    if (!a || a->G <= 0 || a->G > CAT_ROLLOUT_MAX_AGENTS) return fail(CAT_PPO_ERR_BAD_ARG, who, "G must be 1..CAT_ROLLOUT_MAX_AGENTS");
    if (!a->hyper) return fail(CAT_PPO_ERR_BAD_ARG, who, "hyper is NULL");
    if (!a->sched_active) return fail(CAT_PPO_ERR_BAD_ARG, who, "sched_active is NULL");
    if (a->mode < 1 || a->mode > (CAT_PPO_SCHED_KL | CAT_PPO_SCHED_ANNEAL)) return fail(CAT_PPO_ERR_BAD_ARG, who, "mode must be 1..3");
    if (!(a->lr_factor >= 1.0f)) return fail(CAT_PPO_ERR_BAD_ARG, who, "lr_factor must be >= 1");
    if (!(a->kl_factor >= 1.0f)) return fail(CAT_PPO_ERR_BAD_ARG, who, "kl_factor must be >= 1");
    if (!(a->lr_min <= a->lr_max)) return fail(CAT_PPO_ERR_BAD_ARG, who, "lr_min must be <= lr_max");
    if (!(a->progress >= 0.0f && a->progress <= 1.0f)) return fail(CAT_PPO_ERR_BAD_ARG, who, "progress must lie in [0, 1]");
    hipLaunchKernelGGL(schedule_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, *a);
    return launched();
}
