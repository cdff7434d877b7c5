// cat_render_nav.h -- the navigation kernels of cat_render.hip (included there and nowhere else): the all-pairs hop table of a batch of
// map grids (cat_render_nav_build), one tick of the privileged "pursue" / "flee" opponents (cat_render_nav_step) and one tick of geodesic reward
// shaping (cat_render_nav_shape) and the start states of the geodesic curriculum (cat_render_nav_spawn).  include/cat_render.h states the
// rules; as_cops_and_thieves_amd/navigation.py (hops_reference, navigate_step, shaping_step, spawn_step) is their NumPy / torch statement, which the kernels equal exactly: every value is an integer, or an fp32
// result of the same rounded operations.
#pragma once

#include "cat_learn_common.h"
#include "cat_render.h"

namespace {

constexpr int NAV_BLOCK = 256;
constexpr uint32_t NAV_NONE = CAT_NAV_NONE;

// ---- the table.  One workgroup per (map, goal): blockIdx.x is the goal's index in the concatenated cell arrays.  The goal's row and the
// map's free mask (with each cell's on-grid neighbours) live in LDS; a level never reads a value it writes (a cell taken in level L
// holds L + 1, the level looks for L), so the sweep runs in place with one barrier per level.  `changed` rotates over three words: word (L + 1) % 3 is cleared during level L, and its
// last readers (level L - 2) have all passed the barrier of level L - 1.
__global__ __launch_bounds__(NAV_BLOCK) void nav_build_kernel(const cat_render_nav_build_args a)
{
    __shared__ uint16_t dist[CAT_NAV_MAX_CELLS];
    __shared__ uint8_t open[CAT_NAV_MAX_CELLS];
    __shared__ int changed[3];
    const int kg = blockIdx.x, tid = threadIdx.x;
    int Wc = 0, Hc = 0, cell_off = 0, hops_off = 0;
    bool found = false;
    for (int m = 0; m < a.n_maps; ++m) {                    // (uniform: the table is at most 16 rows)
        const int w = a.grid[4 * m], h = a.grid[4 * m + 1], off = a.grid[4 * m + 2];
        if (!found && w >= 1 && h >= 1 && (long)w * h <= CAT_NAV_MAX_CELLS && kg >= off && kg < off + w * h) {
            Wc = w; Hc = h; cell_off = off; hops_off = a.grid[4 * m + 3];
            found = true;
        }
    }
    if (!found) return;                                     // checked on the host; a bad device copy writes nothing
    const int C = Wc * Hc, goal = kg - cell_off;
    for (int k = tid; k < C; k += NAV_BLOCK) {
        const bool f = a.free[cell_off + k] != 0;
        const int ix = k / Hc, iy = k - ix * Hc;
        // 0 = blocked; else bit 0 and, in bits 1 .. 4, which of the neighbours k - Hc, k + Hc, k - 1, k + 1 are on the grid
        open[k] = f ? (uint8_t)(1 | (ix > 0) << 1 | (ix + 1 < Wc) << 2 | (iy > 0) << 3 | (iy + 1 < Hc) << 4) : 0;
        dist[k] = (k == goal && f) ? 0 : NAV_NONE;
    }
    if (tid < 3) changed[tid] = 0;
    __syncthreads();
    for (int L = 0; L < C; ++L) {
        bool any = false;
        for (int k = tid; k < C; k += NAV_BLOCK) {
            const int o = open[k];
            if (!o || dist[k] != NAV_NONE) continue;
            const bool hit = ((o & 2) && dist[k - Hc] == L) || ((o & 4) && dist[k + Hc] == L) || ((o & 8) && dist[k - 1] == L) ||
                             ((o & 16) && dist[k + 1] == L);
            if (hit) { dist[k] = (uint16_t)(L + 1); any = true; }
        }
        if (any) changed[L % 3] = 1;
        if (tid == 0) changed[(L + 1) % 3] = 0;
        __syncthreads();
        if (!changed[L % 3]) break;                         // (uniform over the workgroup)
    }
    uint16_t *row = a.hops + (size_t)hops_off + (size_t)goal * C;
    for (int k = tid; k < C; k += NAV_BLOCK) row[k] = dist[k];
}

// ---- the tick.  blockIdx.y is the navigator, so its column, mask and scripts are scalar loads; a thread owns one slot.
struct NavGrid { int Wc, Hc, C; const uint16_t *snap, *hops; const uint8_t *free; };

// the (snapped) cell of an agent's f16 position pair, -1 = none; x, y receive the position
__device__ __forceinline__ int nav_cell(uint32_t xy, int cell, const NavGrid &g, float &x, float &y)
{
    const uint32_t xb = xy & 0xFFFFu, yb = xy >> 16;
    x = (float)__builtin_bit_cast(_Float16, (uint16_t)xb);
    y = (float)__builtin_bit_cast(_Float16, (uint16_t)yb);
    if ((xb & 0x7C00u) == 0x7C00u || (yb & 0x7C00u) == 0x7C00u || !(x >= 0.0f) || !(y >= 0.0f)) return -1;
    const int ix = (int)floorf(x) / cell, iy = (int)floorf(y) / cell;      // a finite f16 is below 65536: the int is exact
    if (ix >= g.Wc || iy >= g.Hc) return -1;
    const int s = g.snap[ix * g.Hc + iy];
    return s < g.C ? s : -1;                                // CAT_NAV_NONE, or anything else that is no cell of this grid
}

__global__ __launch_bounds__(NAV_BLOCK) void nav_step_kernel(const cat_render_nav_step_args a)
{
    const int g = blockIdx.y, n = blockIdx.x * NAV_BLOCK + threadIdx.x;
    if (n >= a.N) return;
    int script = -1;
    for (int s = 0; s < a.S; ++s)                           // (scalar: no per-lane index into the argument block)
        if (n >= a.seg_start[s] && n < a.seg_start[s + 1]) script = a.seg_script[g][s];
    if (script < 0) return;
    const int A = a.A, me = a.agent[g];
    const uint32_t mask = a.opp_mask[g];
    const float u = a.uniform[(size_t)g * a.N + n];
    int action = min(3, (int)(4.0f * u)), d_out = -1;

    const int m = a.slot_map ? a.slot_map[n] : 0;
    NavGrid gr{0, 0, 0, nullptr, nullptr, nullptr};
    if (m >= 0 && m < a.n_maps) {
        const int32_t *row = a.grid + 4 * m;
        const int w = row[0], h = row[1];
        if (w >= 1 && h >= 1 && (long)w * h <= CAT_NAV_MAX_CELLS) {
            gr.Wc = w; gr.Hc = h; gr.C = w * h;
            gr.snap = a.snap + row[2]; gr.free = a.free + row[2]; gr.hops = a.hops + row[3];
        }
    }
    const uint32_t *pos = (const uint32_t *)a.team_positions + (size_t)n * A;
    float px, py;
    const int ca = gr.C ? nav_cell(pos[me], a.cell, gr, px, py) : -1;
    if (ca >= 0) {
        const int C = gr.C, ix = ca / gr.Hc, iy = ca - ix * gr.Hc;
        // the four neighbours by action: 0 = -x, 1 = +y, 2 = +x, 3 = -y
        const int nb[4] = {ca - gr.Hc, ca + 1, ca + gr.Hc, ca - 1};
        const bool on[4] = {ix > 0, iy + 1 < gr.Hc, ix + 1 < gr.Wc, iy > 0};
        bool use[4];
        uint32_t lo[4], sum[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            use[i] = on[i] && gr.free[on[i] ? nb[i] : ca] != 0;
            lo[i] = 0xFFFFu; sum[i] = 0u;
        }
        const bool any_use = use[0] || use[1] || use[2] || use[3];
        const bool flee = script == CAT_NAV_FLEE;
        uint32_t best = 0xFFFFFFFFu;
        int bt = -1;
        float tx = 0.0f, ty = 0.0f;
        for (int j = 0; j < A; ++j) {
            if (!((mask >> j) & 1u)) continue;
            float ox, oy;
            const int b = nav_cell(pos[j], a.cell, gr, ox, oy);
            if (b < 0) continue;
            const uint16_t *row = gr.hops + (size_t)b * C;
            const uint32_t ha = row[ca];
            if (ha != NAV_NONE) {
                const uint32_t key = (ha << 8) | (uint32_t)j;
                if (key < best) { best = key; bt = b; tx = ox; ty = oy; }
            }
            if (flee) {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (use[i]) {
                        const uint32_t h = row[nb[i]];
                        lo[i] = min(lo[i], h); sum[i] += h;
                    }
            }
        }
        if (bt >= 0 && any_use) {
            const int d = (int)(best >> 8);
            const float dx = tx - px, dy = ty - py;
            const int pref = fabsf(dx) >= fabsf(dy) ? (dx >= 0.0f ? 2 : 0) : (dy >= 0.0f ? 1 : 3);
            d_out = d;
            if (flee) {
                int pick = -1;
                uint32_t bm = 0, bs = 0;
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (use[i] && (pick < 0 || lo[i] > bm || (lo[i] == bm && sum[i] > bs))) { pick = i; bm = lo[i]; bs = sum[i]; }
                action = pick;
            } else if (d == 0) {
                action = pref;
            } else {
                const uint16_t *row = gr.hops + (size_t)bt * C;
                uint32_t v[4], vmin = 0xFFFFFFFFu;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    v[i] = use[i] ? (uint32_t)row[nb[i]] : 0xFFFFFFFFu;
                    vmin = min(vmin, v[i]);
                }
                int pick = -1;
#pragma unroll
                for (int i = 3; i >= 0; --i)
                    if (v[i] == vmin) pick = i;
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (i == pref && v[i] == vmin) pick = i;
                action = pick;
            }
        }
    }
    a.actions[(size_t)n * A + me] = action;
    if (a.nav_hops) a.nav_hops[(size_t)g * a.N + n] = d_out;
}

// ---- reward shaping.  A thread owns one slot: it finds the cells of the slot's A agents once (they are the same for every shaped agent g),
// then walks the G rows; g is uniform, so agent / opp_mask / coef are scalar loads.  The cell arrays are indexed by unrolled constants only
// (agent[g] is picked by comparison), so they stay in registers.  The enclosing file is compiled with contraction off: gamma * phi1 - phi0 is a
// rounded multiply and a rounded subtraction, as navigation.shaping_step has them.
__device__ __forceinline__ void nav_cells(const uint32_t *pos, int A, int cell, const NavGrid &gr, int (&c)[CAT_RENDER_MAX_AGENTS])
{
#pragma unroll
    for (int j = 0; j < CAT_RENDER_MAX_AGENTS; ++j) {
        float x, y;
        c[j] = (j < A && gr.C) ? nav_cell(pos[j], cell, gr, x, y) : -1;
    }
}

// separation(P, g) of include/cat_render.h over the cells c of P's row
__device__ __forceinline__ int nav_separation(const int (&c)[CAT_RENDER_MAX_AGENTS], int me, uint32_t mask, const NavGrid &gr)
{
    int ca = -1;
#pragma unroll
    for (int j = 0; j < CAT_RENDER_MAX_AGENTS; ++j)
        if (j == me) ca = c[j];
    if (ca < 0) return -1;
    uint32_t best = NAV_NONE;
#pragma unroll
    for (int j = 0; j < CAT_RENDER_MAX_AGENTS; ++j)
        if (((mask >> j) & 1u) && c[j] >= 0) best = min(best, (uint32_t)gr.hops[(size_t)c[j] * gr.C + ca]);
    return best == NAV_NONE ? -1 : (int)best;
}

__global__ __launch_bounds__(NAV_BLOCK) void nav_shape_kernel(const cat_render_nav_shape_args a)
{
    const int n = blockIdx.x * NAV_BLOCK + threadIdx.x;
    if (n >= a.N) return;
    const int A = a.A;
    const int m = a.slot_map ? a.slot_map[n] : 0;
    NavGrid gr{0, 0, 0, nullptr, nullptr, nullptr};
    if (m >= 0 && m < a.n_maps) {
        const int32_t *row = a.grid + 4 * m;
        const int w = row[0], h = row[1];
        if (w >= 1 && h >= 1 && (long)w * h <= CAT_NAV_MAX_CELLS) {
            gr.Wc = w; gr.Hc = h; gr.C = w * h;
            gr.snap = a.snap + row[2]; gr.hops = a.hops + row[3];
        }
    }
    int now[CAT_RENDER_MAX_AGENTS], fin[CAT_RENDER_MAX_AGENTS];
    nav_cells((const uint32_t *)a.team_positions + (size_t)n * A, A, a.cell, gr, now);
    const bool prime = a.prime != 0;
    const bool term = !prime && a.terminated[n] != 0;
    const bool timeout = term && a.truncated[n] != 0;
    if (timeout) {                                          // the only rows of final_positions that are ever read
        nav_cells((const uint32_t *)a.final_positions + (size_t)n * A, A, a.cell, gr, fin);
    } else {
#pragma unroll
        for (int j = 0; j < CAT_RENDER_MAX_AGENTS; ++j) fin[j] = -1;
    }
    for (int g = 0; g < a.G; ++g) {
        const int me = a.agent[g];
        const uint32_t mask = a.opp_mask[g];
        const int d_now = nav_separation(now, me, mask, gr);
        int32_t *state = a.hops_prev + (size_t)g * a.N + n;
        if (!prime) {
            const float coef = a.coef[g];
            const int d0 = *state;
            bool defined = d0 >= 0;
            float phi1 = 0.0f;                              // a capture: the potential of a terminal state
            if (!term || timeout) {
                const int d1 = timeout ? nav_separation(fin, me, mask, gr) : d_now;
                defined = defined && d1 >= 0;
                phi1 = coef * (float)min(max(d1, 0), a.cap);
            }
            float F = 0.0f;
            if (defined) {
                const float phi0 = coef * (float)min(d0, a.cap);
                F = a.gamma * phi1 - phi0;
            }
            float *r = a.reward_out + (size_t)g * a.sr_g + n;
            *r = *r + F;
            if (a.shaping_out) a.shaping_out[(size_t)g * a.ss_g + n] = F;
        }
        *state = d_now;
    }
}

// ---- the start-state curriculum.  A wavefront owns one slot (four slots to a workgroup); n is made provably wave-uniform, so the slot's mask,
// band, map row and draws are scalar loads.  `mine` holds the cells chosen so far, one per lane: lane i the cell of the i-th placed agent
// (thieves first); a uniform lane read brings one back, so no array is indexed by a variable and nothing spills.  Every load of the sweeps is
// unconditional and clamped to the grid (k < C is part of the predicate), so the ballots run with all 64 lanes.
constexpr int SPAWN_WAVE = 64;

// is cell k a candidate of the i-th placed agent?  (i, nt, lo, hi and the lane reads of `mine` are wave-uniform)
__device__ __forceinline__ bool spawn_candidate(int k, int i, int nt, int lo, int hi, const NavGrid &g, int mine)
{
    const int kk = min(k, g.C - 1);
    bool c = k < g.C && g.free[kk] != 0;
    for (int p = 0; p < i; ++p) c = c && kk != __builtin_amdgcn_readlane(mine, p);
    if (i > 0 && i < nt) {
        c = c && g.hops[(size_t)__builtin_amdgcn_readlane(mine, 0) * g.C + kk] != NAV_NONE;
    } else if (i >= nt) {
        uint32_t d = NAV_NONE;
        for (int t = 0; t < nt; ++t) d = min(d, (uint32_t)g.hops[(size_t)__builtin_amdgcn_readlane(mine, t) * g.C + kk]);
        c = c && d != NAV_NONE && d >= (uint32_t)lo && d <= (uint32_t)hi;
    }
    return c;
}

__global__ __launch_bounds__(NAV_BLOCK) void nav_spawn_kernel(const cat_render_nav_spawn_args a)
{
    const int lane = threadIdx.x & (SPAWN_WAVE - 1);
    const int n = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (NAV_BLOCK / SPAWN_WAVE) + threadIdx.x / SPAWN_WAVE));
    if (n >= a.N) return;
    const int lo = a.band[2 * n], hi = a.band[2 * n + 1];
    bool ok = a.mask[n] != 0 && lo >= 1 && lo <= hi && hi <= 65534;
    NavGrid gr{0, 0, 0, nullptr, nullptr, nullptr};
    if (ok) {
        const int m = a.slot_map ? a.slot_map[n] : 0;
        ok = m >= 0 && m < a.n_maps;
        if (ok) {
            const int32_t *row = a.grid + 4 * m;
            const int w = row[0], h = row[1];
            ok = w >= 1 && h >= 1 && (long)w * h <= CAT_NAV_MAX_CELLS;
            if (ok) { gr.Wc = w; gr.Hc = h; gr.C = w * h; gr.free = a.free + row[2]; gr.hops = a.hops + row[3]; }
        }
    }
    if (!ok) {                                              // off, unmasked, or a bad device copy of the tables: the env's own spawn
        if (lane == 0) a.placed[n] = 0;
        return;
    }
    const int A = a.A, nt = A - a.n_cops;
    int mine = 0;
    for (int i = 0; i < A; ++i) {
        int cnt = 0;
        for (int base = 0; base < gr.C; base += SPAWN_WAVE)
            cnt += __popcll(__ballot(spawn_candidate(base + lane, i, nt, lo, hi, gr, mine)));
        if (cnt == 0) {                                     // (uniform) nothing of this slot has been written
            if (lane == 0) a.placed[n] = 0;
            return;
        }
        const float u = a.uniform[(size_t)i * a.N + n];
        const int j = min(cnt - 1, max(0, (int)(u * (float)cnt)));
        int before = 0, pick = 0;
        for (int base = 0; base < gr.C; base += SPAWN_WAVE) {
            const bool c = spawn_candidate(base + lane, i, nt, lo, hi, gr, mine);
            const unsigned long long bits = __ballot(c);
            const int here = __popcll(bits);
            if (before + here > j) {                        // the (j - before)-th set bit: the lane with that many candidates below it
                const int rank = __popcll(bits & ((1ull << lane) - 1ull));
                pick = base + __ffsll((long long)__ballot(c && rank == j - before)) - 1;
                break;
            }
            before += here;
        }
        if (lane == i) mine = pick;
    }
    if (lane < A) {
        const int agent = lane < nt ? a.n_cops + lane : lane - nt;
        const int ix = mine / gr.Hc, iy = mine - ix * gr.Hc;
        double *p = a.positions + ((size_t)n * A + agent) * 2;
        p[0] = ((double)ix + 0.5) * (double)a.cell;
        p[1] = ((double)iy + 0.5) * (double)a.cell;
    }
    if (lane == 0) a.placed[n] = 1;
}

int nbfail(const char *msg) { return fail(CAT_RENDER_ERR_BAD_ARG, "cat_render_nav_build", msg); }
int nsfail(const char *msg) { return fail(CAT_RENDER_ERR_BAD_ARG, "cat_render_nav_step", msg); }
int nhfail(const char *msg) { return fail(CAT_RENDER_ERR_BAD_ARG, "cat_render_nav_shape", msg); }
int npfail(const char *msg) { return fail(CAT_RENDER_ERR_BAD_ARG, "cat_render_nav_spawn", msg); }

}   // namespace
