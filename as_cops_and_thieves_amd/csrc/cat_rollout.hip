// cat_rollout.hip -- libcat_learn.so, part 5 of 8: observation packing, action sampling, the scripted opponents and the reward / done glue of a rollout tick
// (include/cat_rollout.h).  Byte/half-word shuffling at a few hundred KB per tick: what matters is that each is ONE
// node of the replayed rollout graph.
#include "cat_learn_common.h"
#include "cat_rollout.h"

namespace {

CAT_LEARN_CODES(CAT_ROLLOUT);
constexpr int BLOCK = 256;

__global__ __launch_bounds__(BLOCK) void pack_kernel(const cat_rollout_pack_args a)
{
    const int g = blockIdx.y, R = a.R;
    const int ai = a.agent[g], si = a.first_agent_state ? 0 : ai;          // whose observation / whose shared state
    const int team = si < a.n_cops ? 0 : 1;
    const __half *od = (const __half *)a.obs_distance, *sd = (const __half *)a.shared_distance;
    const uint8_t *ot = (const uint8_t *)a.obs_type, *st = (const uint8_t *)a.shared_type;
    for (long i = (long)blockIdx.x * BLOCK + threadIdx.x; i < (long)a.N * R; i += (long)gridDim.x * BLOCK) {
        const int n = (int)(i / R), r = (int)(i - (long)n * R);
        __bf16 *p = (__bf16 *)a.policy_in + (size_t)g * a.sp_g + (size_t)n * a.sp_n;
        __bf16 *v = (__bf16 *)a.value_in + (size_t)g * a.sv_g + (size_t)n * a.sv_n;
        const size_t own = ((size_t)n * a.A + ai) * R + r, st_own = ((size_t)n * a.A + si) * R + r, sh = ((size_t)n * 2 + team) * R + r;
        p[r] = obs_scaled(od[own], a.distance_scale);
        p[R + r] = obs_scaled(ot[own], a.type_scale);
        v[r] = obs_scaled(sd[sh], a.distance_scale);
        v[R + r] = obs_scaled(st[sh], a.type_scale);
        v[2 * R + r] = obs_scaled(od[st_own], a.distance_scale);
        v[3 * R + r] = obs_scaled(ot[st_own], a.type_scale);
    }
}

__global__ __launch_bounds__(BLOCK) void sample_kernel(const cat_rollout_sample_args a)
{
    const int g = blockIdx.y;
    for (int n = blockIdx.x * BLOCK + threadIdx.x; n < a.N; n += gridDim.x * BLOCK) {
        const size_t s = (size_t)g * a.N + n;
        const f32x4 z = __builtin_convertvector(*(const bf16x4 *)((const __bf16 *)a.logits + 4 * s), f32x4);
        const Cat4 m = cat4_masses(z);
        const int act = cat4_draw(m, a.uniform[s]);
        a.act_out[(size_t)g * a.sa_g + n] = act;
        a.logp_out[(size_t)g * a.sl_g + n] = cat4_sampled_logp(m, z[act]);
        if (a.value_out) a.value_out[(size_t)g * a.sl_g + n] = (float)((const __bf16 *)a.values)[s];
        a.actions[(size_t)n * a.A + a.agent[g]] = act;
    }
}

__global__ __launch_bounds__(BLOCK) void post_kernel(const cat_rollout_post_args a)
{
    for (int n = blockIdx.x * BLOCK + threadIdx.x; n < a.N; n += gridDim.x * BLOCK) {
        for (int g = 0; g < a.G; ++g) a.reward_out[(size_t)g * a.sr_g + n] = a.reward[(size_t)n * a.A + a.agent[g]];
        const uint8_t d = a.terminated[n] ? 1 : 0;
        if (a.done_out) a.done_out[n] = d;
        if (a.start_out) a.start_out[n] = d;
        if (a.keep_out) a.keep_out[n] = d ? 0.0f : 1.0f;
    }
}

// ---- scripted opponents (include/cat_rollout.h; the rule is stated in selfplay/scripted.py).  One wavefront per (policy, env) row, lane =
// ray: the sight key and the four cone minima are unsigned minima (non-negative f16 order as their bit patterns do), reduced across the
// wave; lane 0 decides and stores.
constexpr int WAVE = 64, SCRIPT_ROWS = BLOCK / WAVE;
constexpr uint32_t NO_KEY = 0xffffffffu, F16_INF = 0x7c00u;

__device__ __forceinline__ uint32_t wave_min(uint32_t v)
{
#pragma unroll
    for (int off = WAVE / 2; off; off >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)v, off);
        v = o < v ? o : v;
    }
    return v;
}
__device__ __forceinline__ int quadrant_action(int k) { return k == 3 ? 3 : 2 - k; }       // ACT = (2, 1, 0, 3), its own inverse

__global__ __launch_bounds__(BLOCK) void scripted_kernel(const cat_rollout_scripted_args a)
{
    const int g = blockIdx.y, lane = threadIdx.x & (WAVE - 1);
    const int n = blockIdx.x * SCRIPT_ROWS + __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
    if (n >= a.N) return;
    int s = 0;
    while (n >= a.seg_start[s + 1]) ++s;                    // n < N = seg_start[S]
    const int script = a.seg_script[g][s];
    if (script < 0) return;
    const int R = a.R, target = a.target[g];
    const size_t row = ((size_t)n * a.A + a.agent[g]) * R;
    const uint16_t *dist = (const uint16_t *)a.obs_distance + row;
    const uint8_t *type = (const uint8_t *)a.obs_type + row;
    uint32_t key = NO_KEY, f0 = F16_INF, f1 = F16_INF, f2 = F16_INF, f3 = F16_INF;
    for (int r = lane; r < R; r += WAVE) {
        const uint32_t bits = dist[r];
        if (type[r] == target) {
            const uint32_t k = (bits << 16) | (uint32_t)r;
            key = k < key ? k : key;
        } else {
            const int o = ((16 * r + R) % (16 * R)) / (2 * R);          // the octant; the cone of quadrant k is octant 2k
            f0 = (o == 0 && bits < f0) ? bits : f0;
            f1 = (o == 2 && bits < f1) ? bits : f1;
            f2 = (o == 4 && bits < f2) ? bits : f2;
            f3 = (o == 6 && bits < f3) ? bits : f3;
        }
    }
    key = wave_min(key); f0 = wave_min(f0); f1 = wave_min(f1); f2 = wave_min(f2); f3 = wave_min(f3);
    if (lane != 0) return;

    const size_t sr = (size_t)g * a.N + n;
    int4 st = *(const int4 *)(a.state + 4 * sr);
    if (a.keep && a.keep[n] == 0.0f) st = make_int4(0, 0, 0, 0);
    int mem = st.z, ttl = st.w, b = 0;
    bool bearing = true;
    if (key != NO_KEY) {
        b = mem = (int)(key & 0xffffu);
        ttl = a.memory_ticks;
    } else if (ttl > 0) {
        ttl -= 1;
        b = mem;
    } else {
        bearing = false;
    }
    int o0, o1, o2, o3;
    if (bearing) {
        const int q = ((8 * b + R) % (8 * R)) / (2 * R), lean = ((8 * b + R) % (2 * R)) >= R ? 1 : -1;
        const int k0 = script == CAT_ROLLOUT_EVADE ? q + 2 : q;
        o0 = k0; o1 = k0 + lean; o2 = k0 - lean; o3 = k0 + 2;
    } else {
        const float u = a.uniform[sr];
        const bool first = st.x == 0;
        const int h4 = (int)(4.0f * u), h = first ? (h4 < 3 ? h4 : 3) : (st.y & 3);
        const bool turn = !first && u < a.turn_prob;
        const int side = ((uint32_t)(u * 16777216.0f) & 1u) ? 1 : -1, kh = quadrant_action(h);
        o0 = turn ? kh + side : kh; o1 = turn ? kh - side : kh + side; o2 = turn ? kh : kh - side; o3 = kh + 2;
    }
    const float fr0 = __half2float(__ushort_as_half((unsigned short)f0)), fr1 = __half2float(__ushort_as_half((unsigned short)f1));
    const float fr2 = __half2float(__ushort_as_half((unsigned short)f2)), fr3 = __half2float(__ushort_as_half((unsigned short)f3));
    const int order[4] = {o0 & 3, o1 & 3, o2 & 3, o3 & 3};
    int pick = -1, best_k = 0;
    float best = -1.0f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int k = order[j];
        const float f = k == 0 ? fr0 : k == 1 ? fr1 : k == 2 ? fr2 : fr3;
        if (pick < 0 && f >= a.clear_min) pick = k;
        if (f > best) { best = f; best_k = k; }            // strictly: the earliest in the order keeps a tie
    }
    if (pick < 0) pick = best_k;
    const int act = quadrant_action(pick);
    a.actions[(size_t)n * a.A + a.agent[g]] = act;
    *(int4 *)(a.state + 4 * sr) = make_int4(1, act, mem, ttl);
}

}   // namespace

extern "C" int cat_rollout_abi_version(void) { return CAT_ROLLOUT_ABI_VERSION; }
extern "C" const char *cat_rollout_last_error(void) { return g_err; }

extern "C" int cat_rollout_pack(const cat_rollout_pack_args *a, void *stream)
{
    if (!a || a->N <= 0 || a->R <= 0 || a->A <= 0 || a->A > CAT_ROLLOUT_MAX_AGENTS || a->G <= 0 || a->G > CAT_ROLLOUT_MAX_AGENTS)
        return fail(CAT_ROLLOUT_ERR_BAD_ARG, "cat_rollout_pack: bad dimensions");
    if (!agents_ok(a->agent, a->G, a->A)) return fail(CAT_ROLLOUT_ERR_BAD_ARG, "cat_rollout_pack: agent index out of range");
    if (!a->obs_distance || !a->obs_type || !a->shared_distance || !a->shared_type || !a->policy_in || !a->value_in)
        return fail(CAT_ROLLOUT_ERR_BAD_ARG, "cat_rollout_pack: a required buffer is NULL");
    long work = (long)a->N * a->R;
    int blocks = (int)((work + BLOCK - 1) / BLOCK);
    if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(pack_kernel, dim3(blocks, a->G), dim3(BLOCK), 0, (hipStream_t)stream, *a);
    return launched();
}

extern "C" int cat_rollout_sample(const cat_rollout_sample_args *a, void *stream)
{
    if (!a || a->N <= 0 || a->A <= 0 || a->A > CAT_ROLLOUT_MAX_AGENTS || a->G <= 0 || a->G > CAT_ROLLOUT_MAX_AGENTS)
        return fail(CAT_ROLLOUT_ERR_BAD_ARG, "cat_rollout_sample: bad dimensions");
    if (!agents_ok(a->agent, a->G, a->A)) return fail(CAT_ROLLOUT_ERR_BAD_ARG, "cat_rollout_sample: agent index out of range");
    if (!a->logits || !a->uniform || !a->act_out || !a->logp_out || !a->actions || (a->value_out && !a->values) || ((uintptr_t)a->logits % 8))
        return fail(CAT_ROLLOUT_ERR_BAD_ARG, "cat_rollout_sample: NULL or misaligned buffer");
    int blocks = (a->N + BLOCK - 1) / BLOCK;
    if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(sample_kernel, dim3(blocks, a->G), dim3(BLOCK), 0, (hipStream_t)stream, *a);
    return launched();
}

extern "C" int cat_rollout_post(const cat_rollout_post_args *a, void *stream)
{
    if (!a || a->N <= 0 || a->A <= 0 || a->A > CAT_ROLLOUT_MAX_AGENTS || a->G <= 0 || a->G > CAT_ROLLOUT_MAX_AGENTS)
        return fail(CAT_ROLLOUT_ERR_BAD_ARG, "cat_rollout_post: bad dimensions");
    if (!agents_ok(a->agent, a->G, a->A)) return fail(CAT_ROLLOUT_ERR_BAD_ARG, "cat_rollout_post: agent index out of range");
    if (!a->reward || !a->terminated || !a->reward_out) return fail(CAT_ROLLOUT_ERR_BAD_ARG, "cat_rollout_post: a required buffer is NULL");
    int blocks = (a->N + BLOCK - 1) / BLOCK;
    if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(post_kernel, dim3(blocks), dim3(BLOCK), 0, (hipStream_t)stream, *a);
    return launched();
}

extern "C" int cat_rollout_scripted(const cat_rollout_scripted_args *a, void *stream)
{
    const char *who = "cat_rollout_scripted";
    if (!a) return fail(CAT_ROLLOUT_ERR_BAD_ARG, who, "NULL arguments");
    if (a->N <= 0 || a->A <= 0 || a->A > CAT_ROLLOUT_MAX_AGENTS) return fail(CAT_ROLLOUT_ERR_BAD_ARG, who, "bad dimensions");
    if (a->G <= 0 || a->G > CAT_ROLLOUT_MAX_AGENTS) return fail(CAT_ROLLOUT_ERR_BAD_ARG, who, "G outside 1..8");
    if (a->R < CAT_ROLLOUT_MIN_RAYS || a->R > CAT_ROLLOUT_MAX_RAYS) return fail(CAT_ROLLOUT_ERR_BAD_ARG, who, "R outside 8..1024");
    if (!agents_ok(a->agent, a->G, a->A)) return fail(CAT_ROLLOUT_ERR_BAD_ARG, who, "agent index out of range");
    for (int g = 0; g < a->G; ++g)
        if (a->target[g] != 1 && a->target[g] != 2) return fail(CAT_ROLLOUT_ERR_BAD_ARG, who, "target type outside {1, 2}");
    if (a->memory_ticks < 0) return fail(CAT_ROLLOUT_ERR_BAD_ARG, who, "memory_ticks is negative");
    if (!(a->clear_min >= 0.0f)) return fail(CAT_ROLLOUT_ERR_BAD_ARG, who, "clear_min is not a number >= 0");
    if (!(a->turn_prob >= 0.0f && a->turn_prob <= 1.0f)) return fail(CAT_ROLLOUT_ERR_BAD_ARG, who, "turn_prob outside [0, 1]");
    if (a->S < 1 || a->S > CAT_ROLLOUT_MAX_SEGMENTS) return fail(CAT_ROLLOUT_ERR_BAD_ARG, who, "S outside 1..32");
    if (a->seg_start[0] != 0) return fail(CAT_ROLLOUT_ERR_BAD_ARG, who, "the segments must begin at 0");
    if (a->seg_start[a->S] != a->N) return fail(CAT_ROLLOUT_ERR_BAD_ARG, who, "the segments must end at N");
    for (int s = 0; s < a->S; ++s)
        if (a->seg_start[s + 1] <= a->seg_start[s]) return fail(CAT_ROLLOUT_ERR_BAD_ARG, who, "segment bounds must be strictly increasing");
    for (int g = 0; g < a->G; ++g)
        for (int s = 0; s < a->S; ++s)
            if (a->seg_script[g][s] < -1 || a->seg_script[g][s] > CAT_ROLLOUT_EVADE)
                return fail(CAT_ROLLOUT_ERR_BAD_ARG, who, "script outside {-1, 0, 1}");
    if (!a->obs_distance || !a->obs_type || !a->uniform || !a->state || !a->actions)
        return fail(CAT_ROLLOUT_ERR_BAD_ARG, who, "a required buffer is NULL");
    if ((uintptr_t)a->state % 16) return fail(CAT_ROLLOUT_ERR_BAD_ARG, who, "state is not 16-byte aligned");
    hipLaunchKernelGGL(scripted_kernel, dim3((a->N + SCRIPT_ROWS - 1) / SCRIPT_ROWS, a->G), dim3(BLOCK), 0, (hipStream_t)stream, *a);
    return launched(who);
}
