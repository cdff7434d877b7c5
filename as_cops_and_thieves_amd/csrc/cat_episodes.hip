// cat_episodes.hip -- libcat_learn.so, part 7 of 8: episode accounting on the device (include/cat_episodes.h).
// A few bytes per env-tick and a few hundred bytes of state per slot: what matters is that the f64 sums are formed in a fixed
// order (tick order inside a slot, a halving tree across the slots) and that each entry is ONE capturable launch.
#include <limits.h>

#include "cat_learn_common.h"
#include "cat_episodes.h"

// ret_sq += r * r is a multiply and an add, as NumPy does it (no fused multiply-add): this file only, as in cat_render.hip
#pragma clang fp contract(off)

namespace {

CAT_LEARN_CODES(CAT_EPISODES);
constexpr int UBLOCK = 64;      // update: one wave per workgroup, so that a few thousand slots spread over as many CUs as they can
constexpr int UNROLL = 8;       // update: ticks whose loads are issued together before the serial walk over them
constexpr int SBLOCK = 1024;    // summary: ONE workgroup (per segment); the last ten levels of the halving tree run through its LDS
constexpr int SLEVELS = 22;     // summary: levels of the tree a thread folds in registers (2^31 slots / SBLOCK = 2^21 leaves)
constexpr int BINS = CAT_EPISODES_HIST_BINS;

// Lane = slot.  The state of the slot lives in registers for the T ticks; the inputs of UNROLL ticks are loaded ahead of the
// walk (a wave reads 64 * A contiguous floats and 64 contiguous bytes per stream and tick).  kWindows: a row stands for ticks[row]
// env ticks (cat_episode_windows_update); without it ``ticks`` is not read and the code is that of one tick per row.
template <int A, bool kWindows>
__global__ __launch_bounds__(UBLOCK) void episodes_update_kernel(const cat_episodes_update_args a, const int32_t *__restrict__ ticks)
{
    __shared__ unsigned int hist[BINS];
    for (int b = threadIdx.x; b < BINS; b += UBLOCK) hist[b] = 0;
    __syncthreads();
    const long n = (long)blockIdx.x * UBLOCK + threadIdx.x;
    if (n < a.N) {
        const cat_episodes_state &s = a.s;
        double run[A], rsum[A], rsq[A];
#pragma unroll
        for (int i = 0; i < A; ++i) { run[i] = s.ret_run[n * A + i]; rsum[i] = s.ret_sum[n * A + i]; rsq[i] = s.ret_sq[n * A + i]; }
        int len = s.len_run[n], fin = s.finished[n], cop = s.cop_wins[n], thief = s.thief_wins[n], tout = s.timeouts[n];
        int lmin = s.len_min[n], lmax = s.len_max[n];
        long lsum = s.len_sum[n];
        const bool limited = a.quota != nullptr;
        const int quota = limited ? a.quota[n] : 0;
        for (int t0 = 0; t0 < a.T; t0 += UNROLL) {
            float r[UNROLL][A];
            uint8_t term[UNROLL], trunc[UNROLL];
            int8_t win[UNROLL];
            int played[UNROLL];
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                const bool live = t0 + u < a.T;                    // (the same in every lane)
                const size_t row = (size_t)(live ? t0 + u : t0) * (size_t)a.N + (size_t)n;
#pragma unroll
                for (int i = 0; i < A; ++i) r[u][i] = a.reward[row * A + i];
                term[u] = a.terminated[row]; trunc[u] = a.truncated[row]; win[u] = a.winner[row];
                played[u] = kWindows ? ticks[row] : 1;
            }
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                if (t0 + u >= a.T) break;
#pragma unroll
                for (int i = 0; i < A; ++i) run[i] += (double)r[u][i];
                len += played[u];
                if (term[u]) {
                    if (!limited || fin < quota) {
                        fin += 1;
                        cop += win[u] == 0; thief += win[u] == 1; tout += trunc[u] != 0;
                        lsum += len;
                        lmin = len < lmin ? len : lmin;
                        lmax = len > lmax ? len : lmax;
#pragma unroll
                        for (int i = 0; i < A; ++i) { rsum[i] += run[i]; rsq[i] += run[i] * run[i]; }
                        const long bin = ((long)len - 1) * BINS / a.max_step_count;
                        atomicAdd(&hist[bin < BINS - 1 ? (bin < 0 ? 0 : bin) : BINS - 1], 1u);
                    }
#pragma unroll
                    for (int i = 0; i < A; ++i) run[i] = 0.0;
                    len = 0;
                }
            }
        }
#pragma unroll
        for (int i = 0; i < A; ++i) { s.ret_run[n * A + i] = run[i]; s.ret_sum[n * A + i] = rsum[i]; s.ret_sq[n * A + i] = rsq[i]; }
        s.len_run[n] = len; s.finished[n] = fin; s.cop_wins[n] = cop; s.thief_wins[n] = thief; s.timeouts[n] = tout;
        s.len_min[n] = lmin; s.len_max[n] = lmax; s.len_sum[n] = lsum;
    }
    __syncthreads();
    for (int b = threadIdx.x; b < BINS; b += UBLOCK)
        if (hist[b]) atomicAdd((unsigned long long *)&a.s.len_hist[b], (unsigned long long)hist[b]);
}

// The halving tree over x[0 .. P) (x[i] += x[i + h], h = P/2 .. 1), P' = max(P, SBLOCK) (more zero padding adds zeros only).
// After the levels h >= SBLOCK, x[i] (i < SBLOCK) is the same tree over the K = P' / SBLOCK elements i + k * SBLOCK: thread i folds
// them depth first -- leaves in bit-reversed order of k, a stack of one partial sum per level, all statically indexed -- and the
// levels h < SBLOCK run through the LDS.
__device__ double tree_leaf_fold(const double *x, long N, int A, int agent, int i, long K, int logK, double *stack)
{
    double res = 0.0;
    for (long c = 0; c < K; ++c) {
        const long k = logK ? (long)(__brev((unsigned int)c) >> (32 - logK)) : 0;
        const long idx = (long)i + k * SBLOCK;
        double v = idx < N ? x[idx * A + agent] : 0.0;
        bool placed = false;
#pragma unroll
        for (int l = 0; l < SLEVELS; ++l) {
            if (!placed) {
                if ((c >> l) & 1) v = stack[l] + v;        // the left half of this level is waiting: close the pair
                else { stack[l] = v; res = v; placed = true; }
            }
        }
    }
    return res;     // the last leaf (c = K - 1, all ones) closed every level: what it placed is the whole tree
}

// The summary of N consecutive slots -> one block.  ``s`` / ``quota`` point at the first of them (every per-slot pointer already
// advanced), so a segment of a larger batch goes through the very code, and the very order of additions, of the whole batch.
__device__ __forceinline__ void summarise_slots(const cat_episodes_state &s, const int32_t *quota, long N, int A, cat_episodes_summary_block *out)
{
    __shared__ double tree[SBLOCK];
    __shared__ unsigned long long isum[6];
    __shared__ int imin, imax;
    const int i = threadIdx.x;
    if (i < 6) isum[i] = 0;
    if (i == 0) { imin = INT_MAX; imax = 0; }
    __syncthreads();
    unsigned long long part[6] = {0, 0, 0, 0, 0, 0};
    int lmin = INT_MAX, lmax = 0;
    for (long n = i; n < N; n += SBLOCK) {
        const int fin = s.finished[n];
        part[0] += (unsigned long long)fin; part[1] += (unsigned long long)s.cop_wins[n]; part[2] += (unsigned long long)s.thief_wins[n];
        part[3] += (unsigned long long)s.timeouts[n];
        part[4] += (quota && fin < quota[n]) ? 1ull : 0ull;
        part[5] += (unsigned long long)s.len_sum[n];
        const int mn = s.len_min[n], mx = s.len_max[n];
        lmin = mn < lmin ? mn : lmin; lmax = mx > lmax ? mx : lmax;
    }
#pragma unroll
    for (int j = 0; j < 6; ++j) atomicAdd(&isum[j], part[j]);      // integer adds in LDS: order-free
    atomicMin(&imin, lmin); atomicMax(&imax, lmax);
    long P = SBLOCK;
    int logK = 0;
    while (P < N) { P <<= 1; ++logK; }
    const long K = P / SBLOCK;
    double stack[SLEVELS];
#pragma unroll
    for (int l = 0; l < SLEVELS; ++l) stack[l] = 0.0;
    for (int v = 0; v < 2 * A; ++v) {
        const int agent = v < A ? v : v - A;
        tree[i] = tree_leaf_fold(v < A ? s.ret_sum : s.ret_sq, N, A, agent, i, K, logK, stack);
        __syncthreads();
        for (int h = SBLOCK / 2; h >= 1; h >>= 1) {
            if (i < h) tree[i] += tree[i + h];
            __syncthreads();
        }
        if (i == 0) (v < A ? out->ret_sum : out->ret_sq)[agent] = tree[0];
        __syncthreads();
    }
    if (i == 0) {
        cat_episodes_summary_block *o = out;
        o->episodes = (int64_t)isum[0]; o->cop_wins = (int64_t)isum[1]; o->thief_wins = (int64_t)isum[2]; o->timeouts = (int64_t)isum[3];
        o->open_slots = (int64_t)isum[4]; o->len_sum = (int64_t)isum[5];
        o->len_min = imin; o->len_max = imax;
        for (int j = A; j < CAT_EPISODES_MAX_AGENTS; ++j) { o->ret_sum[j] = 0.0; o->ret_sq[j] = 0.0; }
    }
}

__global__ __launch_bounds__(SBLOCK) void episodes_summary_kernel(const cat_episodes_summary_args a)
{
    summarise_slots(a.s, a.quota, a.N, a.A, a.out);
}

// Workgroup = segment: the per-slot pointers advanced to the segment's first row, N = its length, block s of ``out``.  The len_hist
// pointer is not read by a summary.
__global__ __launch_bounds__(SBLOCK) void episodes_segment_summary_kernel(const cat_episodes_segment_summary_args a)
{
    const long lo = a.seg_start[blockIdx.x], n = (long)a.seg_start[blockIdx.x + 1] - lo;
    cat_episodes_state s = a.s;
    s.ret_run += lo * a.A; s.ret_sum += lo * a.A; s.ret_sq += lo * a.A;
    s.len_run += lo; s.finished += lo; s.cop_wins += lo; s.thief_wins += lo; s.timeouts += lo;
    s.len_sum += lo; s.len_min += lo; s.len_max += lo;
    summarise_slots(s, a.quota ? a.quota + lo : nullptr, n, a.A, a.out + blockIdx.x);
}


bool state_complete(const cat_episodes_state &s)
{
    return s.ret_run && s.len_run && s.finished && s.cop_wins && s.thief_wins && s.timeouts && s.len_sum && s.len_min && s.len_max &&
           s.ret_sum && s.ret_sq && s.len_hist;
}

}   // namespace

extern "C" int cat_episodes_abi_version(void) { return CAT_EPISODES_ABI_VERSION; }
extern "C" const char *cat_episodes_last_error(void) { return g_err; }

// The argument checks and the launch of both update entries; ``ticks`` NULL = one tick per row.
static int launch_update(const cat_episodes_update_args *a, const int32_t *ticks, void *stream, const char *dims, const char *null)
{
    if (!a || a->T < 1 || a->T > CAT_EPISODES_MAX_TICKS || a->N <= 0 || a->A <= 0 || a->A > CAT_EPISODES_MAX_AGENTS || a->max_step_count <= 0)
        return fail(CAT_EPISODES_ERR_BAD_ARG, dims);
    if (!a->reward || !a->terminated || !a->truncated || !a->winner || !state_complete(a->s))
        return fail(CAT_EPISODES_ERR_BAD_ARG, null);
    const dim3 grid((unsigned)(((long)a->N + UBLOCK - 1) / UBLOCK)), block(UBLOCK);
    hipStream_t st = (hipStream_t)stream;
#define CAT_EP_LAUNCH(AA)                                                                                          \
    case AA:                                                                                                       \
        if (ticks) hipLaunchKernelGGL((episodes_update_kernel<AA, true>), grid, block, 0, st, *a, ticks);          \
        else hipLaunchKernelGGL((episodes_update_kernel<AA, false>), grid, block, 0, st, *a, ticks);               \
        break;
    switch (a->A) {
    CAT_EP_LAUNCH(1) CAT_EP_LAUNCH(2) CAT_EP_LAUNCH(3) CAT_EP_LAUNCH(4) CAT_EP_LAUNCH(5) CAT_EP_LAUNCH(6) CAT_EP_LAUNCH(7)
    default:
        if (ticks) hipLaunchKernelGGL((episodes_update_kernel<8, true>), grid, block, 0, st, *a, ticks);
        else hipLaunchKernelGGL((episodes_update_kernel<8, false>), grid, block, 0, st, *a, ticks);
        break;
    }
#undef CAT_EP_LAUNCH
    return launched();
}

extern "C" int cat_episodes_update(const cat_episodes_update_args *a, void *stream)
{
    return launch_update(a, nullptr, stream, "cat_episodes_update: bad dimensions", "cat_episodes_update: a required buffer is NULL");
}

extern "C" int cat_episode_windows_update(const cat_episode_windows_args *a, void *stream)
{
    return launch_update(a ? &a->u : nullptr, a ? a->ticks : nullptr, stream, "cat_episode_windows_update: bad dimensions",
                         "cat_episode_windows_update: a required buffer is NULL");
}

extern "C" int cat_episodes_summary(const cat_episodes_summary_args *a, void *stream)
{
    if (!a || a->N <= 0 || a->A <= 0 || a->A > CAT_EPISODES_MAX_AGENTS)
        return fail(CAT_EPISODES_ERR_BAD_ARG, "cat_episodes_summary: bad dimensions");
    if (!a->out || !state_complete(a->s)) return fail(CAT_EPISODES_ERR_BAD_ARG, "cat_episodes_summary: a required buffer is NULL");
    hipLaunchKernelGGL(episodes_summary_kernel, dim3(1), dim3(SBLOCK), 0, (hipStream_t)stream, *a);
    return launched();
}

extern "C" int cat_episodes_segment_summary(const cat_episodes_segment_summary_args *a, void *stream)
{
    if (!a || a->N <= 0 || a->A <= 0 || a->A > CAT_EPISODES_MAX_AGENTS)
        return fail(CAT_EPISODES_ERR_BAD_ARG, "cat_episodes_segment_summary: bad dimensions");
    if (a->S < 1 || a->S > CAT_EPISODES_MAX_SEGMENTS)
        return fail(CAT_EPISODES_ERR_BAD_ARG, "cat_episodes_segment_summary: bad segments: S must lie in 1 .. CAT_EPISODES_MAX_SEGMENTS");
    if (a->seg_start[0] != 0 || a->seg_start[a->S] != a->N)
        return fail(CAT_EPISODES_ERR_BAD_ARG, "cat_episodes_segment_summary: bad segments: seg_start must begin at 0 and end at N");
    for (int s = 0; s < a->S; ++s)
        if (a->seg_start[s + 1] <= a->seg_start[s])
            return fail(CAT_EPISODES_ERR_BAD_ARG, "cat_episodes_segment_summary: bad segments: seg_start must be strictly increasing");
    if (!a->out || !state_complete(a->s)) return fail(CAT_EPISODES_ERR_BAD_ARG, "cat_episodes_segment_summary: a required buffer is NULL");
    hipLaunchKernelGGL(episodes_segment_summary_kernel, dim3((unsigned)a->S), dim3(SBLOCK), 0, (hipStream_t)stream, *a);
    return launched();
}
