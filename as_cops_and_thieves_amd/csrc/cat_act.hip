// cat_act.hip -- libcat_learn.so, part 8 of 8: the act tick of the stacked recurrent policies in one launch (include/cat_act.h).
//
// A workgroup of four waves owns TM = 32 or 64 rows (envs) of ONE network and carries them from the env core's observation
// buffers to the action.  Every layer is Y^T = W X^T on mfma_f32_16x16x32_bf16 with the WEIGHTS as the A operand: a lane's
// fragment is 16 contiguous bytes of one weight row, loaded straight from global memory (the parameters of a network, ~0.6 MB,
// are shared by all its workgroups and stay in L2; they never pass through the LDS), the activations are the B operand, read
// from a bf16 LDS image [row][feature], and a lane's four accumulator registers are four consecutive output features of one
// row: one 8-byte LDS store after bias and activation.  The waves split the OUTPUT features of a layer and each keeps all
// TM / 16 row tiles in its accumulators, so a weight fragment is fetched once per workgroup.
//
//  - the two convolutions run by direct taps, one conv2 output position at a time: the five conv1 positions it reads are
//    computed into a [TM][5 * 64] image (wave w owns conv1 channels 16 w .. 16 w + 15, its one weight fragment lives in
//    registers: K = 10 padded to 32), then conv2 is a [TM x 320] x [320 x 32] product whose ten weight fragments per wave
//    also stay in registers for the whole loop.  The 64-channel intermediate of all positions never exists;
//  - conv2 writes its output in (channel, position) order, the column order of the 256-wide layer's weight;
//  - the LSTM: a wave takes 16 hidden units at a time and accumulates their four gates (rows u, 128 + u, 256 + u, 384 + u of
//    W_ih | W_hh over the [f | h] image), so the cell runs on the accumulators and only h', c' leave;
//  - the last layer (4 logits) is one zero-padded 16-row tile; the lanes that hold a row's four logits draw the action.
//
// LDS: two regions that the stages reuse -- A: observation rows + conv1 image, later [f | h], later head layer 1;
// B: conv2 output, later h' and head layer 2.
#include "cat_learn_common.h"
#include "cat_act.h"

namespace {

CAT_LEARN_CODES(CAT_ACT);
static_assert(sizeof(cat_act_args) == 280 && sizeof(cat_act_collect_args) == 400, "the layouts the ctypes mirror pins");
constexpr int BLOCK = 256, HID = CAT_ACT_HIDDEN;

enum { A_NONE = 0, A_RELU = 1, A_TANH = 2 };

template <int R> struct Geo {
    static constexpr int L1 = (R - 5) / 2 + 1, L2 = (L1 - 5) / 3 + 1, KFC = 32 * L2;
    static constexpr int XIN_LD = 2 * R + 8, C1_LD = 5 * 64 + 8, X2_LD = KFC + 8, FH_LD = 256 + HID + 8, HN_LD = HID + 8, H2_LD = 64 + 8;
    static constexpr int A_LD = (XIN_LD + C1_LD > FH_LD ? XIN_LD + C1_LD : FH_LD);          // elements per row of region A
    static constexpr int B_LD = (X2_LD > HN_LD + H2_LD ? X2_LD : HN_LD + H2_LD);            // and of region B
    static constexpr size_t lds_bytes(int tm) { return (size_t)tm * (A_LD + B_LD) * 2; }
};

template <int ACT> __device__ __forceinline__ float act_fwd(float x)
{
    if (ACT == A_RELU) return fmaxf(x, 0.0f);
    if (ACT == A_TANH) return tanh_fast(x);
    return x;
}
__device__ __forceinline__ f32x4 ld4(const __bf16 *p) { return __builtin_convertvector(*(const bf16x4 *)p, f32x4); }

// Y[m][n] = act(sum_k X[m][k] W[n][k] + bias[n]) for the TM rows of the workgroup: X, Y bf16 LDS images, W [nout][K] global.
template <int K, int MT, int ACT>
__device__ __forceinline__ void layer(const __bf16 *W, const __bf16 *bias, int nout, const __bf16 *X, int ldx, __bf16 *Y, int ldy,
                                      int w, int q, int r)
{
    for (int nt = w; nt < nout / 16; nt += 4) {
        f32x4 acc[MT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) acc[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
        const __bf16 *wrow = W + (size_t)(nt * 16 + r) * K + 8 * q;
#pragma unroll
        for (int s = 0; s < K / 32; ++s) {
            const bf16x8 wf = *(const bf16x8 *)(wrow + 32 * s);
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                const bf16x8 xf = *(const bf16x8 *)(X + (mt * 16 + r) * ldx + 32 * s + 8 * q);
                acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, xf, acc[mt], 0, 0, 0);
            }
        }
        const f32x4 b = ld4(bias + nt * 16 + 4 * q);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            f32x4 v;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = act_fwd<ACT>(acc[mt][e] + b[e]);
            *(bf16x4 *)(Y + (mt * 16 + r) * ldy + nt * 16 + 4 * q) = __builtin_convertvector(v, bf16x4);
        }
    }
}

// The chain for the rows row0 .. rend - 1 (at most TM of them) of policy g: the parameters at element offset po of every block, or no
// network at all where ``random``.  Rows at and beyond rend are neither read nor written (their LDS images are zero): in the league
// form they belong to another segment, whose workgroup updates them in place.
// COLLECT (cat_act_collect_step): ``x`` names the rollout's buffers and the same pass also stores the packed input rows, the state as it
// stood before the tick and the action / log-probability where the rollout keeps them; nothing else of the chain changes.
template <int R, int MT, bool COLLECT = false>
__device__ __forceinline__ void act_rows(const cat_act_args &a, const int g, const int row0, const int rend, const size_t po, const bool random,
                                         const cat_act_collect_args *x = nullptr)
{
    using G = Geo<R>;
    constexpr int TM = 16 * MT;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __bf16 *regA = (__bf16 *)smem, *regB = regA + TM * G::A_LD;
    __bf16 *xin = regA, *c1 = regA + TM * G::XIN_LD, *fh = regA, *h1 = regA;       // region A over time
    __bf16 *x2 = regB, *hn = regB, *h2 = regB + TM * G::HN_LD;                      // region B over time

    const int N = a.d.N, A = a.d.A, ai = a.agent[g];
    const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, q = l >> 4, r = l & 15;
    const float *uni = a.uniform + (size_t)g * N;

    if (random) {                                    // a uniformly random agent: no network, no state
        for (int m = tid; m < TM; m += BLOCK) {
            const int n = row0 + m;
            if (n < rend) {
                const int act = (int)(4.0f * uni[n]);
                a.actions[(size_t)n * A + ai] = act < 3 ? act : 3;
            }
        }
        return;
    }

    const __bf16 *w1 = (const __bf16 *)a.p.conv1_w + po, *b1 = (const __bf16 *)a.p.conv1_b + po;
    const __bf16 *w2 = (const __bf16 *)a.p.conv2_w + po, *b2 = (const __bf16 *)a.p.conv2_b + po;
    const __bf16 *wfc = (const __bf16 *)a.p.fc_w + po, *bfc = (const __bf16 *)a.p.fc_b + po;
    const __bf16 *wih = (const __bf16 *)a.p.w_ih + po, *whh = (const __bf16 *)a.p.w_hh + po;
    const __bf16 *bih = (const __bf16 *)a.p.b_ih + po, *bhh = (const __bf16 *)a.p.b_hh + po;
    const __bf16 *hw0 = (const __bf16 *)a.p.head0_w + po, *hb0 = (const __bf16 *)a.p.head0_b + po;
    const __bf16 *hw1 = (const __bf16 *)a.p.head1_w + po, *hb1 = (const __bf16 *)a.p.head1_b + po;
    const __bf16 *hw2 = (const __bf16 *)a.p.head2_w + po, *hb2 = (const __bf16 *)a.p.head2_b + po;

    // ---- the observation rows: [distance (R) | type (R)] of obs_scaled elements, as cat_rollout_pack's policy row; rows >= rend are zero
    {
        const __half *od = (const __half *)a.obs_distance;
        const uint8_t *ot = (const uint8_t *)a.obs_type;
        for (int i = tid; i < TM * R; i += BLOCK) {
            const int m = i / R, rr = i - m * R, n = row0 + m;
            __bf16 dv = (__bf16)0.0f, tv = (__bf16)0.0f;
            if (n < rend) {
                const size_t o = ((size_t)n * A + ai) * R + rr;
                dv = obs_scaled(od[o], a.distance_scale);
                tv = obs_scaled(ot[o], a.type_scale);
            }
            xin[m * G::XIN_LD + rr] = dv;
            xin[m * G::XIN_LD + R + rr] = tv;
        }
        if constexpr (COLLECT) {
            // the critic's rows, cat_rollout_pack's: [shared distance | shared type | distance | type] of agent si and its team, four
            // consecutive elements (8 bytes) per store; with R = 90 the four may come from two quarters of the row
            const int si = x->first_agent_state ? 0 : ai, team = si < x->n_cops ? 0 : 1;
            const __half *sd = (const __half *)x->shared_distance;
            const uint8_t *st = (const uint8_t *)x->shared_type;
            __bf16 *vg = (__bf16 *)x->value_in + (size_t)g * x->sv_g;
            for (int i = tid; i < TM * R; i += BLOCK) {
                const int m = i / R, k = i - m * R, n = row0 + m;
                if (n >= rend) continue;
                bf16x4 v;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int e = 4 * k + j, seg = e / R, rr = e - seg * R;
                    const size_t sh = ((size_t)n * 2 + team) * R + rr, own = ((size_t)n * A + si) * R + rr;
                    v[j] = seg == 0 ? obs_scaled(sd[sh], a.distance_scale) : seg == 1 ? obs_scaled(st[sh], a.type_scale)
                         : seg == 2 ? obs_scaled(od[own], a.distance_scale) : obs_scaled(ot[own], a.type_scale);
                }
                *(bf16x4 *)(vg + (size_t)n * x->sv_n + 4 * k) = v;
            }
        }
    }
    // ---- the convolutions' weights of this wave, in registers for the whole trunk
    const int nt2 = w & 1;                            // conv2: this wave's 16 output channels
    bf16x8 w1f, w2f[10];
    {
        const __bf16 zero = (__bf16)0.0f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {                 // conv1 weight [64][2][5]: row = channel 16 w + r, k = c * 5 + tap < 10
            const int k = 8 * q + j;
            w1f[j] = k < 10 ? w1[(16 * w + r) * 10 + k] : zero;
        }
#pragma unroll
        for (int s = 0; s < 10; ++s)                  // conv2 weight [32][64][5] as k = tap * 64 + c_in: step s = (tap, half of c_in)
#pragma unroll
            for (int j = 0; j < 8; ++j) w2f[s][j] = w2[((16 * nt2 + r) * 64 + (s & 1) * 32 + 8 * q + j) * 5 + (s >> 1)];
    }
    const f32x4 b1v = ld4(b1 + 16 * w + 4 * q), b2v = ld4(b2 + 16 * nt2 + 4 * q);
    __syncthreads();
    if constexpr (COLLECT) {                          // the policy's rows: the xin image as it stands, before region A becomes [f | h]
        __bf16 *pg = (__bf16 *)x->policy_in + (size_t)g * x->sp_g;
        for (int i = tid; i < TM * (R / 2); i += BLOCK) {
            const int m = i / (R / 2), k = i - m * (R / 2), n = row0 + m;
            if (n < rend) *(bf16x4 *)(pg + (size_t)n * x->sp_n + 4 * k) = *(const bf16x4 *)(xin + m * G::XIN_LD + 4 * k);
        }
    }

    for (int p = 0; p < G::L2; ++p) {
        // conv1 at positions 3 p .. 3 p + 4 -> c1[m][tap * 64 + channel]
#pragma unroll
        for (int t = 0; t < 5; ++t) {
            const int c0 = 2 * (3 * p + t);           // first ray of the window
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                const __bf16 *xr = xin + (mt * 16 + r) * G::XIN_LD + c0;
                bf16x8 xf = {};
                if (q == 0) {
#pragma unroll
                    for (int j = 0; j < 5; ++j) xf[j] = xr[j];
#pragma unroll
                    for (int j = 5; j < 8; ++j) xf[j] = xr[R + j - 5];
                } else if (q == 1) {
                    xf[0] = xr[R + 3];
                    xf[1] = xr[R + 4];
                }
                const f32x4 acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w1f, xf, f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
                f32x4 v;
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = fmaxf(acc[e] + b1v[e], 0.0f);
                *(bf16x4 *)(c1 + (mt * 16 + r) * G::C1_LD + t * 64 + 16 * w + 4 * q) = __builtin_convertvector(v, bf16x4);
            }
        }
        __syncthreads();
        // conv2 at position p -> x2[m][channel * L2 + p]
        for (int mt = w >> 1; mt < MT; mt += 2) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < 10; ++s) {
                const bf16x8 xf = *(const bf16x8 *)(c1 + (mt * 16 + r) * G::C1_LD + 32 * s + 8 * q);
                acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w2f[s], xf, acc, 0, 0, 0);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e)
                x2[(mt * 16 + r) * G::X2_LD + (16 * nt2 + 4 * q + e) * G::L2 + p] = (__bf16)fmaxf(acc[e] + b2v[e], 0.0f);
        }
        __syncthreads();                              // c1 is rewritten by the next position
    }

    // ---- h entering the tick (zero where an episode starts) next to f: the LSTM's input image [f (256) | h (128)]
    const __bf16 *hg = (const __bf16 *)a.h + (size_t)g * N * HID, *cg = (const __bf16 *)a.c + (size_t)g * N * HID;
    for (int i = tid; i < TM * (HID / 8); i += BLOCK) {
        const int m = i / (HID / 8), ch = i % (HID / 8), n = row0 + m;
        bf16x8 v = {};
        if constexpr (COLLECT) {                      // h and c as they stand in memory go out first: keep is not applied to them
            if (n < rend) {
                v = *(const bf16x8 *)(hg + (size_t)n * HID + 8 * ch);
                if (x->h0_out) {
                    const size_t o = ((size_t)g * N + n) * HID + 8 * ch;
                    *(bf16x8 *)((__bf16 *)x->h0_out + o) = v;
                    *(bf16x8 *)((__bf16 *)x->c0_out + o) = *(const bf16x8 *)(cg + (size_t)n * HID + 8 * ch);
                }
                if (a.keep && a.keep[n] == 0.0f) v = bf16x8{};
            }
        } else {
            if (n < rend && (!a.keep || a.keep[n] != 0.0f)) v = *(const bf16x8 *)(hg + (size_t)n * HID + 8 * ch);
        }
        *(bf16x8 *)(fh + m * G::FH_LD + 256 + 8 * ch) = v;
    }
    layer<G::KFC, MT, A_TANH>(wfc, bfc, 256, x2, G::X2_LD, fh, G::FH_LD, w, q, r);
    __syncthreads();

    // ---- LSTM cell: 16 hidden units x 4 gates per pass
    for (int j = w; j < HID / 16; j += 4) {
        f32x4 acc[4][MT];
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) acc[k][mt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
        for (int s = 0; s < 8; ++s) {
            bf16x8 wf[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) wf[k] = *(const bf16x8 *)(wih + (size_t)(k * HID + 16 * j + r) * 256 + 32 * s + 8 * q);
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                const bf16x8 xf = *(const bf16x8 *)(fh + (mt * 16 + r) * G::FH_LD + 32 * s + 8 * q);
#pragma unroll
                for (int k = 0; k < 4; ++k) acc[k][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[k], xf, acc[k][mt], 0, 0, 0);
            }
        }
#pragma unroll 2
        for (int s = 0; s < 4; ++s) {
            bf16x8 wf[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) wf[k] = *(const bf16x8 *)(whh + (size_t)(k * HID + 16 * j + r) * HID + 32 * s + 8 * q);
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                const bf16x8 xf = *(const bf16x8 *)(fh + (mt * 16 + r) * G::FH_LD + 256 + 32 * s + 8 * q);
#pragma unroll
                for (int k = 0; k < 4; ++k) acc[k][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[k], xf, acc[k][mt], 0, 0, 0);
            }
        }
        const int u0 = 16 * j + 4 * q;                // this lane's four hidden units
        f32x4 bi[4], bh[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) { bi[k] = ld4(bih + k * HID + u0); bh[k] = ld4(bhh + k * HID + u0); }
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const int m = mt * 16 + r, n = row0 + m;
            f32x4 cp = {0.f, 0.f, 0.f, 0.f};
            if (n < rend && (!a.keep || a.keep[n] != 0.0f)) cp = ld4(cg + (size_t)n * HID + u0);
            f32x4 cn, hv;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float gi = sigmoidf(acc[0][mt][e] + bi[0][e] + bh[0][e]), gf = sigmoidf(acc[1][mt][e] + bi[1][e] + bh[1][e]);
                const float gg = tanh_fast(acc[2][mt][e] + bi[2][e] + bh[2][e]), go = sigmoidf(acc[3][mt][e] + bi[3][e] + bh[3][e]);
                cn[e] = gf * cp[e] + gi * gg;
                hv[e] = go * tanh_fast(cn[e]);
            }
            const bf16x4 hb = __builtin_convertvector(hv, bf16x4);
            *(bf16x4 *)(hn + m * G::HN_LD + u0) = hb;
            if (n < rend) {
                *(bf16x4 *)((__bf16 *)a.h + ((size_t)g * N + n) * HID + u0) = hb;
                *(bf16x4 *)((__bf16 *)a.c + ((size_t)g * N + n) * HID + u0) = __builtin_convertvector(cn, bf16x4);
            }
        }
    }
    __syncthreads();

    // ---- the head
    layer<HID, MT, A_RELU>(hw0, hb0, 128, hn, G::HN_LD, h1, G::HN_LD, w, q, r);
    __syncthreads();
    layer<HID, MT, A_RELU>(hw1, hb1, 64, h1, G::HN_LD, h2, G::H2_LD, w, q, r);
    __syncthreads();
    for (int mt = w; mt < MT; mt += 4) {              // 4 logits: one 16-row tile whose rows 4 .. 15 are zero
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            bf16x8 wf = {};
            if (r < 4) wf = *(const bf16x8 *)(hw2 + r * 64 + 32 * s + 8 * q);
            const bf16x8 xf = *(const bf16x8 *)(h2 + (mt * 16 + r) * G::H2_LD + 32 * s + 8 * q);
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, xf, acc, 0, 0, 0);
        }
        const int n = row0 + mt * 16 + r;
        if (q != 0 || n >= rend) continue;               // lanes 0 .. 15 hold the four logits of row r
        const f32x4 bz = ld4(hb2);
        f32x4 zf;
#pragma unroll
        for (int e = 0; e < 4; ++e) zf[e] = acc[e] + bz[e];
        const bf16x4 zb = __builtin_convertvector(zf, bf16x4);
        const f32x4 z = __builtin_convertvector(zb, f32x4);
        const size_t sidx = (size_t)g * N + n;
        const Cat4 cm = cat4_masses(z);                 // on the bf16 logits, as cat_rollout_sample
        int act;
        if (a.mode == CAT_ACT_GREEDY) {
            act = 0;
            float best = z[0];
            if (z[1] > best) { best = z[1]; act = 1; }
            if (z[2] > best) { best = z[2]; act = 2; }
            if (z[3] > best) { best = z[3]; act = 3; }
        } else {
            act = cat4_draw(cm, uni[n]);
        }
        const float zact = act == 0 ? z[0] : act == 1 ? z[1] : act == 2 ? z[2] : z[3];
        a.actions[(size_t)n * A + ai] = act;
        if (a.logits_out) *(bf16x4 *)((__bf16 *)a.logits_out + 4 * sidx) = zb;
        if constexpr (COLLECT) {
            const float lp = cat4_sampled_logp(cm, zact);
            if (a.logp_out) a.logp_out[sidx] = lp;
            x->act_out[(size_t)g * x->sa_g + n] = act;
            x->logp_out[(size_t)g * x->sl_g + n] = lp;
        } else {
            if (a.logp_out) a.logp_out[sidx] = cat4_sampled_logp(cm, zact);
        }
    }
}

template <int R, int MT>
__global__ __launch_bounds__(BLOCK) void act_kernel(const cat_act_args a)
{
    const int g = blockIdx.y;
    act_rows<R, MT>(a, g, blockIdx.x * (16 * MT), a.d.N, (size_t)g * a.p.stride, (a.random_mask >> g) & 1u);
}

template <int R, int MT>
__global__ __launch_bounds__(BLOCK) void act_collect_kernel(const cat_act_collect_args a)
{
    const int g = blockIdx.y;
    act_rows<R, MT, true>(a.base, g, blockIdx.x * (16 * MT), a.base.d.N, (size_t)g * a.base.p.stride, false, &a);
}

// The league form: workgroup blockIdx.x is tile t of segment s, found by a uniform scan of the (at most 32) segment lengths -- the
// host's grid.x is the sum of ceil(len_s / TM) -- and plays parameter set seg_set[g][s] of the bank on the rows of that segment only.
template <int R, int MT>
__global__ __launch_bounds__(BLOCK) void act_league_kernel(const cat_act_league_args a)
{
    constexpr int TM = 16 * MT;
    const int g = blockIdx.y;
    int t = blockIdx.x, s = 0;
    for (; s < a.S - 1; ++s) {
        const int tiles = (a.seg_start[s + 1] - a.seg_start[s] + TM - 1) / TM;
        if (t < tiles) break;
        t -= tiles;
    }
    const int row0 = a.seg_start[s] + t * TM, send = a.seg_start[s + 1], set = a.seg_set[g][s];
    if (row0 >= send) return;                        // a grid larger than the table's tiles: nothing to do
    act_rows<R, MT>(a.base, g, row0, row0 + TM < send ? row0 + TM : send, (size_t)(set < 0 ? 0 : set) * a.base.p.stride, set < 0);
}

bool dims_ok(const cat_act_dims &d)
{
    return d.G >= 1 && d.G <= CAT_ACT_MAX_AGENTS && d.N >= 1 && d.A >= 1 && d.A <= CAT_ACT_MAX_AGENTS && (d.R == 64 || d.R == 90);
}

// The checks both entries share, before any device call.  ``need_params``: some policy evaluates a network.
int check_args(const cat_act_args *a, const char *who, bool need_params)
{
    if (!a || !dims_ok(a->d)) return fail(CAT_ACT_ERR_BAD_ARG, who, "bad dimensions (G 1..8, A 1..8, N >= 1, R 64 or 90)");
    if (!agents_ok(a->agent, a->d.G, a->d.A)) return fail(CAT_ACT_ERR_BAD_ARG, who, "agent index out of range");
    if ((a->mode != CAT_ACT_SAMPLE && a->mode != CAT_ACT_GREEDY) || (a->random_mask >> a->d.G) != 0 ||
        (a->row_tile != 0 && a->row_tile != 32 && a->row_tile != 64))
        return fail(CAT_ACT_ERR_BAD_ARG, who, "bad mode, random_mask or row_tile");
    if (!a->obs_distance || !a->obs_type || !a->uniform || !a->actions) return fail(CAT_ACT_ERR_BAD_ARG, who, "a required buffer is NULL");
    if (need_params) {
        const void *ps[] = {a->p.conv1_w, a->p.conv1_b, a->p.conv2_w, a->p.conv2_b, a->p.fc_w, a->p.fc_b, a->p.w_ih, a->p.w_hh, a->p.b_ih, a->p.b_hh,
                            a->p.head0_w, a->p.head0_b, a->p.head1_w, a->p.head1_b, a->p.head2_w, a->p.head2_b, a->h, a->c};
        for (const void *p : ps)
            if (!p || ((uintptr_t)p % 16)) return fail(CAT_ACT_ERR_BAD_ARG, who, "a parameter or state pointer is NULL or not 16-byte aligned");
        if (a->p.stride % 8) return fail(CAT_ACT_ERR_BAD_ARG, who, "the parameter stride must be a multiple of 8 elements");
        if (a->logits_out && ((uintptr_t)a->logits_out % 8)) return fail(CAT_ACT_ERR_BAD_ARG, who, "logits_out must be 8-byte aligned");
    }
    return CAT_ACT_OK;
}

// ``tiles``: grid.x -- the row tiles of the N rows, or of all segments of the league form
template <int R, int MT, typename Args> int launch(void (*kernel)(const Args), const Args &a, int tiles, int G, const char *who, hipStream_t stream)
{
    const size_t lds = Geo<R>::lds_bytes(16 * MT);
    // the 64-row tiles take more than the default 64 KB of dynamic LDS: raised on every launch (per device, not a stream operation)
    if (hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        return fail(CAT_ACT_ERR_HIP, who, "hipFuncSetAttribute failed");
    hipLaunchKernelGGL(kernel, dim3(tiles, G), dim3(BLOCK), lds, stream, a);
    return launched(who);
}

}   // namespace

extern "C" int cat_act_abi_version(void) { return CAT_ACT_ABI_VERSION; }
extern "C" const char *cat_act_last_error(void) { return g_err; }
extern "C" int cat_act_supported(const cat_act_dims *d) { return d && dims_ok(*d) ? 1 : 0; }

extern "C" int cat_act_step(const cat_act_args *a, void *stream)
{
    const char *who = "cat_act_step";
    const bool all_random = a && dims_ok(a->d) && a->random_mask == (1u << a->d.G) - 1u;
    if (const int rc = check_args(a, who, !all_random)) return rc;
    const int TM = a->row_tile ? a->row_tile : 32, tiles = (a->d.N + TM - 1) / TM, G = a->d.G;
    hipStream_t s = (hipStream_t)stream;
    if (a->d.R == 64) return TM == 32 ? launch<64, 2>(act_kernel<64, 2>, *a, tiles, G, who, s) : launch<64, 4>(act_kernel<64, 4>, *a, tiles, G, who, s);
    return TM == 32 ? launch<90, 2>(act_kernel<90, 2>, *a, tiles, G, who, s) : launch<90, 4>(act_kernel<90, 4>, *a, tiles, G, who, s);
}

extern "C" int cat_act_collect_step(const cat_act_collect_args *a, void *stream)
{
    const char *who = "cat_act_collect_step";
    if (!a || !dims_ok(a->base.d)) return fail(CAT_ACT_ERR_BAD_ARG, who, "bad dimensions (G 1..8, A 1..8, N >= 1, R 64 or 90)");
    if (a->base.random_mask != 0) return fail(CAT_ACT_ERR_BAD_ARG, who, "random_mask must be 0 (a learner's rollout rows come from its network)");
    if (const int rc = check_args(&a->base, who, true)) return rc;
    const int R = a->base.d.R;
    if (!a->shared_distance || !a->shared_type || !a->policy_in || !a->value_in || !a->act_out || !a->logp_out)
        return fail(CAT_ACT_ERR_BAD_ARG, who, "a required collect buffer is NULL");
    if (!a->h0_out != !a->c0_out) return fail(CAT_ACT_ERR_BAD_ARG, who, "h0_out and c0_out must be given together (or both NULL)");
    if (a->n_cops < 0 || a->n_cops > a->base.d.A) return fail(CAT_ACT_ERR_BAD_ARG, who, "n_cops outside 0..A");
    if (((uintptr_t)a->policy_in % 8) || ((uintptr_t)a->value_in % 8) || ((uintptr_t)a->act_out % 8) || ((uintptr_t)a->logp_out % 4) ||
        ((uintptr_t)a->h0_out % 16) || ((uintptr_t)a->c0_out % 16))
        return fail(CAT_ACT_ERR_BAD_ARG, who, "a collect pointer is misaligned (policy_in, value_in, act_out 8 bytes; h0_out, c0_out 16; logp_out 4)");
    if ((a->sp_g % 4) || (a->sp_n % 4) || (a->sv_g % 4) || (a->sv_n % 4) || a->sp_n < 2 * R || a->sv_n < 4 * R)
        return fail(CAT_ACT_ERR_BAD_ARG, who, "a row stride is misaligned or short (sp_g, sp_n, sv_g, sv_n multiples of 4 elements; sp_n >= 2R, sv_n >= 4R)");
    const int TM = a->base.row_tile ? a->base.row_tile : 32, tiles = (a->base.d.N + TM - 1) / TM, G = a->base.d.G;
    hipStream_t s = (hipStream_t)stream;
    if (R == 64)
        return TM == 32 ? launch<64, 2>(act_collect_kernel<64, 2>, *a, tiles, G, who, s) : launch<64, 4>(act_collect_kernel<64, 4>, *a, tiles, G, who, s);
    return TM == 32 ? launch<90, 2>(act_collect_kernel<90, 2>, *a, tiles, G, who, s) : launch<90, 4>(act_collect_kernel<90, 4>, *a, tiles, G, who, s);
}

extern "C" int cat_act_league_step(const cat_act_league_args *a, void *stream)
{
    const char *who = "cat_act_league_step";
    if (!a || !dims_ok(a->base.d)) return fail(CAT_ACT_ERR_BAD_ARG, who, "bad dimensions (G 1..8, A 1..8, N >= 1, R 64 or 90)");
    if (a->S < 1 || a->S > CAT_ACT_MAX_SEGMENTS) return fail(CAT_ACT_ERR_BAD_ARG, who, "S outside 1..32 segments");
    if (a->sets < 1) return fail(CAT_ACT_ERR_BAD_ARG, who, "the bank needs at least one parameter set");
    if (a->base.random_mask != 0) return fail(CAT_ACT_ERR_BAD_ARG, who, "random_mask must be 0 (a random policy is set index -1 of its segment)");
    if (a->seg_start[0] != 0 || a->seg_start[a->S] != a->base.d.N) return fail(CAT_ACT_ERR_BAD_ARG, who, "seg_start must begin at 0 and end at N");
    const int TM = a->base.row_tile == 64 ? 64 : 32, G = a->base.d.G;
    int tiles = 0;
    bool any_net = false;
    for (int s = 0; s < a->S; ++s) {
        if (a->seg_start[s + 1] <= a->seg_start[s]) return fail(CAT_ACT_ERR_BAD_ARG, who, "seg_start must be strictly increasing");
        tiles += (a->seg_start[s + 1] - a->seg_start[s] + TM - 1) / TM;
        for (int g = 0; g < G; ++g) {
            if (a->seg_set[g][s] < -1 || a->seg_set[g][s] >= a->sets) return fail(CAT_ACT_ERR_BAD_ARG, who, "a set index outside [-1, sets)");
            any_net |= a->seg_set[g][s] >= 0;
        }
    }
    if (const int rc = check_args(&a->base, who, any_net)) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (a->base.d.R == 64)
        return TM == 32 ? launch<64, 2>(act_league_kernel<64, 2>, *a, tiles, G, who, st) : launch<64, 4>(act_league_kernel<64, 4>, *a, tiles, G, who, st);
    return TM == 32 ? launch<90, 2>(act_league_kernel<90, 2>, *a, tiles, G, who, st) : launch<90, 4>(act_league_kernel<90, 4>, *a, tiles, G, who, st);
}
