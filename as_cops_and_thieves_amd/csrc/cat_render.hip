// cat_render.hip -- libcat_learn.so, part 6 of 8: batched rgb_array frames on MI355X (gfx950).  include/cat_render.h has the interface and
// the pixel contract; as_cops_and_thieves_amd/render.py (render_frame_reference) is its NumPy statement, byte for byte.
//
// One workgroup draws one TX x TY tile of one frame.  The frame is x-major, [width][height][3], so a column x is a contiguous run of
// height pixels: a lane owns 4 consecutive pixels along y (12 bytes, three dword stores) in each of ROWS columns, and the 16 lanes of
// a column group write 192 contiguous bytes.  Before drawing, the workgroup culls into LDS, in their original order, the walls and ray
// segments whose pixel windows meet the tile; then every pixel takes the first hit of a backward walk over the discs, the rays and the
// walls (a later item overwrites an earlier one in the reference, so the last hit is the one that stays).  Lists longer than a chunk
// are culled and walked chunk by chunk, last chunk first.
//
// Byte equality with NumPy needs binary64 arithmetic in the reference's operation order and no a*b+c contraction into an FMA, which
// hip-clang does by default: the pragma below turns it off for this file (and only here: the library's other kernels keep their flags).
#pragma clang fp contract(off)

#include <math.h>

#include "cat_learn_common.h"
#include "cat_render.h"
#include "cat_render_nav.h"

namespace {

CAT_LEARN_CODES(CAT_RENDER);
constexpr int BLOCK = 256, WAVES = BLOCK / 64;
constexpr int LANES_Y = 16, PIX = 4, ROWS = 2;            // 16 lanes x 4 pixels along y; each thread draws 2 columns
constexpr int TY = LANES_Y * PIX;                         // 64 pixels along y per tile
constexpr int COLS = BLOCK / LANES_Y;                     // 16 columns per pass
constexpr int TX = COLS * ROWS;                           // 32 columns per tile
constexpr int CHUNK = BLOCK;                              // culled items per pass: one candidate per thread
constexpr uint32_t WHITE = 0xFFFFFFu, GREY = 0x3C3C3Cu, BLUE = 0xFF0000u, RED = 0x0000FFu;   // 0xBBGGRR

__device__ __forceinline__ uint32_t rgb(int r, int g, int b) { return (uint32_t)r | ((uint32_t)g << 8) | ((uint32_t)b << 16); }

__device__ __forceinline__ uint32_t ray_colour(int type)
{
    constexpr uint8_t pal[5][3] = CAT_RENDER_RAY_COLOURS;
    const int t = type > 4 ? 4 : type;
    return rgb(pal[t][0], pal[t][1], pal[t][2]);
}

// [trunc(v) + off] clamped to [0, limit]: one bound of a reference window max(int(v) + off, 0) / min(int(v) + off, limit), formed
// in binary64 so that no coordinate can overflow an int (a NaN bound opens the whole window; the pixel tests reject it anyway)
__device__ __forceinline__ int bound(double v, double off, int limit)
{
    return (int)fmin(fmax(trunc(v) + off, 0.0), (double)limit);
}

struct Window { int x0, x1, y0, y1; };

__device__ __forceinline__ bool meets(const Window &w, int dx0, int dx1, int dy0, int dy1)
{
    return w.x0 < w.x1 && w.y0 < w.y1 && w.x0 < dx1 && w.x1 > dx0 && w.y0 < dy1 && w.y1 > dy0;
}

struct Shared {
    int wave_count[WAVES];
    int n;                                                // length of the current list
    // discs
    double dpx[CAT_RENDER_MAX_AGENTS], dpy[CAT_RENDER_MAX_AGENTS];
    Window dwin[CAT_RENDER_MAX_AGENTS];
    // the current chunk's ray segments, in order
    double px[CHUNK], py[CHUNK], ex[CHUNK], ey[CHUNK], vx[CHUNK], vy[CHUNK], c2[CHUNK];
    Window rwin[CHUNK];
    uint32_t rcol[CHUNK];
    // the current chunk's walls
    int wall[CHUNK];
    Window wwin[CHUNK];
};

// Ordered compaction of one candidate per thread: the slot of this thread's item among the kept ones (by thread index), and the
// number kept in s.n.  Ends with a barrier, after which s.n is valid; the caller writes the record, then synchronises again.
__device__ __forceinline__ int compact(bool keep, Shared &s)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long mask = __ballot(keep);
    const int before = __popcll(mask & ((1ull << lane) - 1ull));
    if (lane == 0) s.wave_count[wave] = __popcll(mask);
    __syncthreads();
    int off = 0, total = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
        off += w < wave ? s.wave_count[w] : 0;
        total += s.wave_count[w];
    }
    if (threadIdx.x == 0) s.n = total;
    return off + before;
}

__global__ __launch_bounds__(BLOCK) void render_tiles_kernel(const cat_render_scene sc, const cat_render_args a, int tiles_x, int tiles_y)
{
    __shared__ Shared s;
    const int tiles = tiles_x * tiles_y;
    const int f = blockIdx.x / tiles, tile = blockIdx.x - f * tiles;
    const int x0t = (tile / tiles_y) * TX, y0t = (tile % tiles_y) * TY;
    const int m = a.map_ids_dev[f];
    const bool map_ok = m >= 0 && m < sc.n_maps;          // checked on the host; a bad device copy draws a blank frame, not a fault
    const int Wm = map_ok ? sc.window[2 * m] : 0, Hm = map_ok ? sc.window[2 * m + 1] : 0;
    // the part of the tile inside the map's window: every item is clipped to it, and the frame beyond it stays white
    const int dx0 = x0t, dx1 = min(x0t + TX, Wm), dy0 = y0t, dy1 = min(y0t + TY, Hm);
    const bool live = dx0 < dx1 && dy0 < dy1;             // uniform over the workgroup

    const int ly = (threadIdx.x % LANES_Y) * PIX, lx = threadIdx.x / LANES_Y;
    uint32_t col[ROWS][PIX];
    bool done[ROWS][PIX];
#pragma unroll
    for (int j = 0; j < ROWS; ++j)
#pragma unroll
        for (int i = 0; i < PIX; ++i) { col[j][i] = WHITE; done[j][i] = false; }

    if (live) {
        const int A = a.A;
        const double r = a.agent_radius, r2 = r * r;
        const double *pos = a.positions + (size_t)f * A * 2;
        if ((int)threadIdx.x < A) {
            const int i = threadIdx.x;
            const double px = pos[2 * i], py = pos[2 * i + 1];
            s.dpx[i] = px;
            s.dpy[i] = py;
            s.dwin[i] = Window{bound(px - r, -1.0, Wm), bound(px + r, 2.0, Wm), bound(py - r, -1.0, Hm), bound(py + r, 2.0, Hm)};
        }
        __syncthreads();
        // 3. discs: the last agent that covers a pixel wins
        for (int i = A - 1; i >= 0; --i) {
            const Window w = s.dwin[i];
            const double px = s.dpx[i], py = s.dpy[i];
            const uint32_t c = i < a.n_cops ? BLUE : RED;
#pragma unroll
            for (int j = 0; j < ROWS; ++j) {
                const int x = x0t + lx + COLS * j;
                if (x < w.x0 || x >= w.x1) continue;
                const double X = x + 0.5, dx = X - px;
#pragma unroll
                for (int k = 0; k < PIX; ++k) {
                    const int y = y0t + ly + k;
                    if (done[j][k] || y < w.y0 || y >= w.y1) continue;
                    const double dy = (y + 0.5) - py;
                    if (dx * dx + dy * dy <= r2) { col[j][k] = c; done[j][k] = true; }
                }
            }
        }
        // 2. ray segments, last chunk first, each list backwards
        if (a.flags & CAT_RENDER_RAYS) {
            const int R = a.R, n_items = A * R;
            const uint16_t *dist = a.obs_distance + (size_t)f * A * R;
            const uint8_t *type = a.obs_type + (size_t)f * A * R;
            for (int c0 = ((n_items - 1) / CHUNK) * CHUNK; c0 >= 0; c0 -= CHUNK) {
                const int item = c0 + threadIdx.x;
                double px = 0, py = 0, ex = 0, ey = 0;
                Window w{0, 0, 0, 0};
                bool keep = false;
                if (item < n_items) {
                    const int ag = item / R, k = item - ag * R;
                    px = pos[2 * ag];
                    py = pos[2 * ag + 1];
                    const double d = (double)__builtin_bit_cast(_Float16, dist[item]);
                    const double t = d / a.ray_length;
                    ex = px + t * sc.ray_dx[k];
                    ey = py + t * sc.ray_dy[k];
                    const double lo_x = px < ex ? px : ex, hi_x = px < ex ? ex : px;   // Python's min / max of two floats
                    const double lo_y = py < ey ? py : ey, hi_y = py < ey ? ey : py;
                    w = Window{bound(lo_x, -1.0, Wm), bound(hi_x, 2.0, Wm), bound(lo_y, -1.0, Hm), bound(hi_y, 2.0, Hm)};
                    keep = meets(w, dx0, dx1, dy0, dy1);
                }
                const int slot = compact(keep, s);
                if (keep) {
                    const double vx = ex - px, vy = ey - py;
                    s.px[slot] = px; s.py[slot] = py; s.ex[slot] = ex; s.ey[slot] = ey;
                    s.vx[slot] = vx; s.vy[slot] = vy; s.c2[slot] = vx * vx + vy * vy;
                    s.rwin[slot] = w;
                    s.rcol[slot] = ray_colour(type[item]);
                }
                __syncthreads();
                for (int q = s.n - 1; q >= 0; --q) {
                    const Window rw = s.rwin[q];
                    const double spx = s.px[q], spy = s.py[q], sex = s.ex[q], sey = s.ey[q], svx = s.vx[q], svy = s.vy[q], sc2 = s.c2[q];
                    const uint32_t c = s.rcol[q];
#pragma unroll
                    for (int j = 0; j < ROWS; ++j) {
                        const int x = x0t + lx + COLS * j;
                        if (x < rw.x0 || x >= rw.x1) continue;
                        const double X = x + 0.5, wx = X - spx;
#pragma unroll
                        for (int k = 0; k < PIX; ++k) {
                            const int y = y0t + ly + k;
                            if (done[j][k] || y < rw.y0 || y >= rw.y1) continue;
                            const double Y = y + 0.5, wy = Y - spy;
                            const double c1 = wx * svx + wy * svy;
                            double d2;
                            if (c1 <= 0.0) {
                                d2 = wx * wx + wy * wy;
                            } else if (c1 >= sc2) {
                                const double ax = X - sex, ay = Y - sey;
                                d2 = ax * ax + ay * ay;
                            } else {
                                const double u = c1 / sc2, qx = wx - u * svx, qy = wy - u * svy;
                                d2 = qx * qx + qy * qy;
                            }
                            if (d2 <= 0.25) { col[j][k] = c; done[j][k] = true; }
                        }
                    }
                }
                __syncthreads();
            }
        }
        // 1. walls: any hit is grey
        const int s_begin = sc.shape_off[m], s_end = sc.shape_off[m + 1];
        for (int c0 = s_begin; c0 < s_end; c0 += CHUNK) {
            const int sh = c0 + threadIdx.x;
            Window w{0, 0, 0, 0};
            bool keep = false;
            if (sh < s_end) {
                const double *bb = sc.shape_bb + 4 * (size_t)sh;
                w = Window{bound(bb[0], 0.0, Wm), bound(bb[2], 1.0, Wm), bound(bb[1], 0.0, Hm), bound(bb[3], 1.0, Hm)};
                keep = meets(w, dx0, dx1, dy0, dy1);
            }
            const int slot = compact(keep, s);
            if (keep) { s.wall[slot] = sh; s.wwin[slot] = w; }
            __syncthreads();
            for (int q = 0; q < s.n; ++q) {
                const Window ww = s.wwin[q];
                const int first = sc.shape_first[s.wall[q]], count = sc.shape_count[s.wall[q]];
#pragma unroll
                for (int j = 0; j < ROWS; ++j) {
                    const int x = x0t + lx + COLS * j;
                    if (x < ww.x0 || x >= ww.x1) continue;
                    const double X = x + 0.5;
#pragma unroll
                    for (int k = 0; k < PIX; ++k) {
                        const int y = y0t + ly + k;
                        if (done[j][k] || y < ww.y0 || y >= ww.y1) continue;
                        const double Y = y + 0.5;
                        bool inside = true;
                        for (int p = 0; p < count && inside; ++p) {
                            const double *pl = sc.planes + 5 * (size_t)(first + p);
                            inside = pl[0] * X + pl[1] * Y - pl[4] <= 1.0;
                        }
                        if (inside) { col[j][k] = GREY; done[j][k] = true; }
                    }
                }
            }
            __syncthreads();
        }
    }

    // store: 4 pixels = 12 bytes per column, as three dwords where the address allows it
#pragma unroll
    for (int j = 0; j < ROWS; ++j) {
        const int x = x0t + lx + COLS * j, y = y0t + ly;
        if (x >= a.width || y >= a.height) continue;
        uint8_t *p = a.frames + (((size_t)f * a.width + x) * a.height + y) * 3;
        if (y + PIX <= a.height && ((uintptr_t)p & 3) == 0) {
            uint32_t *q = (uint32_t *)p;
            q[0] = col[j][0] | (col[j][1] << 24);
            q[1] = (col[j][1] >> 8) | (col[j][2] << 16);
            q[2] = (col[j][2] >> 16) | (col[j][3] << 8);
        } else {
            for (int k = 0; k < PIX && y + k < a.height; ++k) {
                p[3 * k] = (uint8_t)col[j][k];
                p[3 * k + 1] = (uint8_t)(col[j][k] >> 8);
                p[3 * k + 2] = (uint8_t)(col[j][k] >> 16);
            }
        }
    }
}

int fail(const char *msg) { return fail(CAT_RENDER_ERR_BAD_ARG, "cat_render_frames", msg); }

// ---- position statistics (cat_render_positions_update; include/cat_render.h has the counting rule) ------------------------------
// One wave per workgroup.  A lane owns one (slot, agent) and walks its T rows serially; a wave holds floor(64 / A) whole slots, so the
// lanes of a slot never straddle a wave and the slot's "who sees whom" is two ballots.  An agent moves a few pixels per tick, so it
// stays in a cell for several rows: the lane keeps (cell, run length) of the plane it is adding to in registers and issues one 64-bit
// integer atomic when the cell or the plane changes, and one at the end.  For SEEN every lane scans its OWN R type bytes once (each
// byte of obs_type is read once) into two bits, "I see a cop" and "I see a thief".
constexpr int PBLOCK = 64;
constexpr uint32_t COP4 = 0x01010101u, THIEF4 = 0x02020202u;      // CAT_COP / CAT_THIEF (cat_sim.h) in every byte of a dword

// non-zero iff some byte of v equals the byte repeated in code4 (exact: the classic zero-byte test on v ^ code4)
__device__ __forceinline__ uint32_t has_byte(uint32_t v, uint32_t code4)
{
    const uint32_t x = v ^ code4;
    return (x - 0x01010101u) & ~x & 0x80808080u;
}

// bit 0: some of the R bytes at p is CAT_COP; bit 1: some is CAT_THIEF.  p has any alignment (rows of R = 90 start on 2-byte
// boundaries, an odd R on any byte): bytes and halfwords up to a 4-byte boundary, dwords up to a 16-byte one, 16-byte loads over
// the body, then the same in reverse.  Every load lies inside [p, p + R).
__device__ __forceinline__ uint32_t scan_types(const uint8_t *p, int R)
{
    const uint8_t *const end = p + R;
    uint32_t cop = 0, thief = 0;
    if (((uintptr_t)p & 1) && p < end) {
        const uint32_t b = *p;
        cop |= b == 1u; thief |= b == 2u;
        p += 1;
    }
    if (((uintptr_t)p & 2) && p + 2 <= end) {
        const uint32_t h = *(const uint16_t *)p | 0xFFFF0000u;     // (0xFF is no type code)
        cop |= has_byte(h, COP4); thief |= has_byte(h, THIEF4);
        p += 2;
    }
    while (((uintptr_t)p & 15) && p + 4 <= end) {
        const uint32_t v = *(const uint32_t *)p;
        cop |= has_byte(v, COP4); thief |= has_byte(v, THIEF4);
        p += 4;
    }
    while (p + 16 <= end) {
        const uint4 v = *(const uint4 *)p;
        cop |= has_byte(v.x, COP4) | has_byte(v.y, COP4) | has_byte(v.z, COP4) | has_byte(v.w, COP4);
        thief |= has_byte(v.x, THIEF4) | has_byte(v.y, THIEF4) | has_byte(v.z, THIEF4) | has_byte(v.w, THIEF4);
        p += 16;
    }
    while (p + 4 <= end) {
        const uint32_t v = *(const uint32_t *)p;
        cop |= has_byte(v, COP4); thief |= has_byte(v, THIEF4);
        p += 4;
    }
    if (p + 2 <= end) {
        const uint32_t h = *(const uint16_t *)p | 0xFFFF0000u;
        cop |= has_byte(h, COP4); thief |= has_byte(h, THIEF4);
        p += 2;
    }
    if (p < end) {
        const uint32_t b = *p;
        cop |= b == 1u; thief |= b == 2u;
    }
    return (cop ? 1u : 0u) | (thief ? 2u : 0u);
}

__device__ __forceinline__ void add64(int64_t *p, unsigned int v) { atomicAdd((unsigned long long *)p, (unsigned long long)v); }

__global__ __launch_bounds__(PBLOCK) void positions_update_kernel(const cat_render_positions_args a, int slots_per_wave)
{
    const int lane = threadIdx.x, A = a.A;
    const int sw = lane / A, ag = lane - sw * A;            // slot of the wave, agent
    const long n = (long)blockIdx.x * slots_per_wave + sw;
    const bool active = sw < slots_per_wave && n < a.N;
    int g = -1, quota = 0, done = 0;
    if (active) {
        g = a.group ? a.group[n] : 0;
        if (g >= a.G) g = -1;                               // no group of the buffers: not counted (and never an index)
        if (a.quota) quota = a.quota[n];
        done = a.done[n];
    }
    const bool limited = a.quota != nullptr, scan = a.obs_type != nullptr;
    const bool cop = ag < a.n_cops;
    // the lanes of the other role in my slot
    unsigned long long opp = 0;
    if (active) {
        const int first = sw * A + (cop ? a.n_cops : 0), count = cop ? A - a.n_cops : a.n_cops;
        if (count > 0) opp = ((1ull << count) - 1ull) << first;         // first + count <= 64 and count <= 16
    }
    const size_t cells = (size_t)a.Wc * (size_t)a.Hc, plane = (size_t)A * cells;
    int64_t *const mine = g >= 0 ? a.counts + ((size_t)g * 3 * A + ag) * cells : nullptr;    // my cells of plane OCC; plane p is p * plane further
    const uint32_t *const pos = (const uint32_t *)a.team_positions;
    long run_off = -1, seen_off = -1;                       // the cell (with its plane) of the run under way
    unsigned int run_n = 0, seen_n = 0, out_n = 0, rows_n = 0;
    for (int t = 0; t < a.T; ++t) {
        const size_t row = (size_t)t * (size_t)a.N + (size_t)n;
        const bool counted = g >= 0 && (!limited || done < quota);      // the same in every lane of a slot
        bool term = false;
        uint32_t xy = 0;
        if (counted) {
            term = a.terminated[row] != 0;
            xy = pos[row * A + ag];
        }
        uint32_t bits = 0;
        if (scan && counted && !term) bits = scan_types(a.obs_type + (row * A + ag) * (size_t)a.R, a.R);
        const unsigned long long sees_cop = __ballot(bits & 1u), sees_thief = __ballot(bits & 2u);
        if (counted) {
            rows_n += 1;
            done += term;
            const uint32_t xb = xy & 0xFFFFu, yb = xy >> 16;
            const float x = (float)__builtin_bit_cast(_Float16, (uint16_t)xb), y = (float)__builtin_bit_cast(_Float16, (uint16_t)yb);
            bool valid = (xb & 0x7C00u) != 0x7C00u && (yb & 0x7C00u) != 0x7C00u && x >= 0.0f && y >= 0.0f;
            int cx = 0, cy = 0;
            if (valid) {                                    // a finite f16 is below 65536: the int is exact
                cx = (int)floorf(x) / a.cell;
                cy = (int)floorf(y) / a.cell;
                valid = cx < a.Wc && cy < a.Hc;
            }
            if (!valid) out_n += 1;
            else {
                const long c = (long)cx * a.Hc + cy;
                const long off = term ? (long)(CAT_POSITIONS_SPAWN * plane) + c : c;
                if (off == run_off) run_n += 1;
                else {
                    if (run_n) add64(mine + run_off, run_n);
                    run_off = off; run_n = 1;
                }
                if (!term && ((cop ? sees_cop : sees_thief) & opp)) {
                    const long soff = (long)(CAT_POSITIONS_SEEN * plane) + c;
                    if (soff == seen_off) seen_n += 1;
                    else {
                        if (seen_n) add64(mine + seen_off, seen_n);
                        seen_off = soff; seen_n = 1;
                    }
                }
            }
        }
    }
    if (run_n) add64(mine + run_off, run_n);
    if (seen_n) add64(mine + seen_off, seen_n);
    if (out_n) add64(a.outside + (size_t)g * A + ag, out_n);
    if (active && ag == 0) a.done[n] = done;
    // rows[g]: the slots of a wave mostly share one group -- one atomic per group and wave
    const bool has_rows = ag == 0 && rows_n != 0;
    unsigned long long pending = __ballot(has_rows);
    while (pending) {                                       // (uniform over the wave)
        const int leader = __ffsll((long long)pending) - 1;
        const int gl = __shfl(g, leader);
        const bool same = has_rows && g == gl;
        unsigned int sum = same ? rows_n : 0u;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d);
        if (lane == leader) add64(a.rows + gl, sum);
        pending &= ~__ballot(same);
    }
}

// Capture / timeout maps: lane = (slot of the wave, agent) as above; a slot's rows in order (the quota rule counts its terminal rows), and only a
// terminal row -- one in an episode's length -- reads a position and adds: one atomic each, no runs to merge.
__global__ __launch_bounds__(PBLOCK) void positions_ends_kernel(const cat_render_positions_ends_args a, int slots_per_wave)
{
    const int lane = threadIdx.x, A = a.A;
    const int sw = lane / A, ag = lane - sw * A;
    const long n = (long)blockIdx.x * slots_per_wave + sw;
    if (sw >= slots_per_wave || n >= a.N) return;
    int g = a.group ? a.group[n] : 0;
    if (g < 0 || g >= a.G) return;                          // no group of the buffers: not counted (and never an index)
    const bool limited = a.quota != nullptr;
    const int quota = limited ? a.quota[n] : 0;
    int done = a.done_before ? a.done_before[n] : 0;
    const size_t cells = (size_t)a.Wc * (size_t)a.Hc;
    const uint32_t *const pos = (const uint32_t *)a.final_positions;
    for (int t = 0; t < a.T; ++t) {
        if (limited && done >= quota) break;                // done only grows: every later row is skipped too
        const size_t row = (size_t)t * (size_t)a.N + (size_t)n;
        if (a.terminated[row] == 0) continue;
        done += 1;
        const int plane = a.truncated[row] != 0 ? CAT_POSITIONS_TIMEOUT : CAT_POSITIONS_CAPTURE;
        const uint32_t xy = pos[row * A + ag];
        const uint32_t xb = xy & 0xFFFFu, yb = xy >> 16;
        const float x = (float)__builtin_bit_cast(_Float16, (uint16_t)xb), y = (float)__builtin_bit_cast(_Float16, (uint16_t)yb);
        bool valid = (xb & 0x7C00u) != 0x7C00u && (yb & 0x7C00u) != 0x7C00u && x >= 0.0f && y >= 0.0f;
        int cx = 0, cy = 0;
        if (valid) {                                        // a finite f16 is below 65536: the int is exact
            cx = (int)floorf(x) / a.cell;
            cy = (int)floorf(y) / a.cell;
            valid = cx < a.Wc && cy < a.Hc;
        }
        const size_t pa = ((size_t)g * 2 + plane) * A + ag;
        if (!valid) add64(a.ends_outside + pa, 1u);
        else add64(a.ends + pa * cells + (size_t)cx * a.Hc + cy, 1u);
    }
}

int pfail(const char *msg) { return fail(CAT_RENDER_ERR_BAD_ARG, "cat_render_positions_update", msg); }
int efail(const char *msg) { return fail(CAT_RENDER_ERR_BAD_ARG, "cat_render_positions_ends_update", msg); }

}   // namespace

extern "C" int cat_render_positions_update(const cat_render_positions_args *a, void *stream)
{
    if (!a) return pfail("NULL arguments");
    if (a->T < 1 || a->T > CAT_POSITIONS_MAX_TICKS || a->N <= 0 || a->A <= 0 || a->A > CAT_RENDER_MAX_AGENTS || a->n_cops < 0 || a->n_cops > a->A)
        return pfail("bad dimensions");
    if (a->cell < 1) return pfail("cell must be >= 1");
    if (a->Wc < 1 || a->Hc < 1) return pfail("the grid needs Wc >= 1 and Hc >= 1");
    if (a->G < 1) return pfail("G must be >= 1");
    if (!a->team_positions || !a->terminated || !a->counts || !a->outside || !a->rows || !a->done) return pfail("a required buffer is NULL");
    if ((uintptr_t)a->team_positions & 3) return pfail("team_positions must be 4-byte aligned");
    if (a->obs_type && a->R < 1) return pfail("obs_type needs R >= 1");
    const int spw = PBLOCK / a->A;
    const long blocks = ((long)a->N + spw - 1) / spw;
    hipLaunchKernelGGL(positions_update_kernel, dim3((unsigned)blocks), dim3(PBLOCK), 0, (hipStream_t)stream, *a, spw);
    return launched("cat_render_positions_update");
}

extern "C" int cat_render_positions_ends_update(const cat_render_positions_ends_args *a, void *stream)
{
    if (!a) return efail("NULL arguments");
    if (a->T < 1 || a->T > CAT_POSITIONS_MAX_TICKS || a->N <= 0 || a->A <= 0 || a->A > CAT_RENDER_MAX_AGENTS) return efail("bad dimensions");
    if (a->cell < 1) return efail("cell must be >= 1");
    if (a->Wc < 1 || a->Hc < 1) return efail("the grid needs Wc >= 1 and Hc >= 1");
    if (a->G < 1) return efail("G must be >= 1");
    if (!a->final_positions || !a->terminated || !a->truncated || !a->ends || !a->ends_outside) return efail("a required buffer is NULL");
    if ((uintptr_t)a->final_positions & 3) return efail("final_positions must be 4-byte aligned");
    const int spw = PBLOCK / a->A;
    const long blocks = ((long)a->N + spw - 1) / spw;
    hipLaunchKernelGGL(positions_ends_kernel, dim3((unsigned)blocks), dim3(PBLOCK), 0, (hipStream_t)stream, *a, spw);
    return launched("cat_render_positions_ends_update");
}

// ---- navigation (include/cat_render.h; the kernels are in cat_render_nav.h)
extern "C" int cat_render_nav_build(const cat_render_nav_build_args *a, void *stream)
{
    if (!a) return nbfail("NULL arguments");
    if (a->n_maps < 1 || a->n_maps > CAT_NAV_MAX_MAPS) return nbfail("n_maps must lie in 1 .. 16");
    if (!a->grid_host || !a->grid) return nbfail("the grid table is NULL (host or device)");
    if (!a->free || !a->hops) return nbfail("a required buffer is NULL");
    if ((uintptr_t)a->hops & 1) return nbfail("hops must be 2-byte aligned");
    long cells = 0, entries = 0;
    for (int m = 0; m < a->n_maps; ++m) {
        const int32_t *g = a->grid_host + 4 * m;
        if (g[0] < 1 || g[1] < 1) return nbfail("a grid needs Wc >= 1 and Hc >= 1");
        const long C = (long)g[0] * g[1];
        if (C > CAT_NAV_MAX_CELLS) return nbfail("a grid has more than 4096 cells");
        if (g[2] != cells || g[3] != entries) return nbfail("the offsets must be those of the maps concatenated in order");
        cells += C;
        entries += C * C;
    }
    hipLaunchKernelGGL(nav_build_kernel, dim3((unsigned)cells), dim3(NAV_BLOCK), 0, (hipStream_t)stream, *a);
    return launched("cat_render_nav_build");
}

extern "C" int cat_render_nav_step(const cat_render_nav_step_args *a, void *stream)
{
    if (!a) return nsfail("NULL arguments");
    if (a->N <= 0 || a->A <= 0 || a->A > CAT_RENDER_MAX_AGENTS) return nsfail("bad dimensions");
    if (a->G < 1 || a->G > CAT_NAV_MAX_NAVIGATORS) return nsfail("G must lie in 1 .. 8");
    if (a->S < 1 || a->S > CAT_NAV_MAX_SEGMENTS) return nsfail("S must lie in 1 .. 32");
    if (a->n_maps < 1 || a->n_maps > CAT_NAV_MAX_MAPS) return nsfail("n_maps must lie in 1 .. 16");
    if (a->cell < 1) return nsfail("cell must be >= 1");
    if (!agents_ok(a->agent, a->G, a->A)) return nsfail("an agent index outside [0, A)");
    for (int g = 0; g < a->G; ++g)
        if ((a->A < 32 && (a->opp_mask[g] >> a->A)) || ((a->opp_mask[g] >> a->agent[g]) & 1u))
            return nsfail("opp_mask names an agent outside [0, A) or the navigator itself");
    if (a->seg_start[0] != 0) return nsfail("the segments must begin at 0");
    if (a->seg_start[a->S] != a->N) return nsfail("the segments must end at N");
    for (int s = 0; s < a->S; ++s)
        if (a->seg_start[s + 1] <= a->seg_start[s]) return nsfail("segment bounds must be strictly increasing");
    for (int g = 0; g < a->G; ++g)
        for (int s = 0; s < a->S; ++s)
            if (a->seg_script[g][s] < -1 || a->seg_script[g][s] > CAT_NAV_FLEE) return nsfail("a script outside {-1, 0, 1}");
    if (!a->grid || !a->free || !a->snap || !a->hops) return nsfail("a table of the field is NULL");
    if (!a->team_positions || !a->uniform || !a->actions) return nsfail("a required buffer is NULL");
    if ((uintptr_t)a->team_positions & 3) return nsfail("team_positions must be 4-byte aligned");
    hipLaunchKernelGGL(nav_step_kernel, dim3((unsigned)((a->N + NAV_BLOCK - 1) / NAV_BLOCK), (unsigned)a->G), dim3(NAV_BLOCK), 0, (hipStream_t)stream, *a);
    return launched("cat_render_nav_step");
}

extern "C" int cat_render_nav_shape(const cat_render_nav_shape_args *a, void *stream)
{
    if (!a) return nhfail("NULL arguments");
    if (a->N <= 0 || a->A <= 0 || a->A > CAT_RENDER_MAX_AGENTS) return nhfail("bad dimensions");
    if (a->G < 1 || a->G > CAT_NAV_MAX_NAVIGATORS) return nhfail("G must lie in 1 .. 8");
    if (a->n_maps < 1 || a->n_maps > CAT_NAV_MAX_MAPS) return nhfail("n_maps must lie in 1 .. 16");
    if (a->cell < 1) return nhfail("cell must be >= 1");
    if (a->cap < 1 || a->cap > 65534) return nhfail("cap must lie in 1 .. 65534");
    if (a->prime != 0 && a->prime != 1) return nhfail("prime must be 0 or 1");
    if (!agents_ok(a->agent, a->G, a->A)) return nhfail("an agent index outside [0, A)");
    for (int g = 0; g < a->G; ++g) {
        if ((a->A < 32 && (a->opp_mask[g] >> a->A)) || ((a->opp_mask[g] >> a->agent[g]) & 1u))
            return nhfail("opp_mask names an agent outside [0, A) or the shaped agent itself");
        if (!isfinite(a->coef[g])) return nhfail("a coefficient is not finite");
    }
    if (!isfinite(a->gamma) || a->gamma < 0.0f) return nhfail("gamma must be finite and >= 0");
    if (!a->grid || !a->snap || !a->hops) return nhfail("a table of the field is NULL");
    if (!a->team_positions || !a->hops_prev) return nhfail("a required buffer is NULL");
    if ((uintptr_t)a->team_positions & 3) return nhfail("team_positions must be 4-byte aligned");
    if (!a->prime) {
        if (!a->final_positions || !a->terminated || !a->truncated || !a->reward_out) return nhfail("a required buffer is NULL (only prime mode does without)");
        if ((uintptr_t)a->final_positions & 3) return nhfail("final_positions must be 4-byte aligned");
        if (a->G > 1 && (a->sr_g < a->N || (a->shaping_out && a->ss_g < a->N))) return nhfail("a row stride below N: the rows would overlap");
    }
    hipLaunchKernelGGL(nav_shape_kernel, dim3((unsigned)((a->N + NAV_BLOCK - 1) / NAV_BLOCK)), dim3(NAV_BLOCK), 0, (hipStream_t)stream, *a);
    return launched("cat_render_nav_shape");
}

extern "C" int cat_render_nav_spawn(const cat_render_nav_spawn_args *a, void *stream)
{
    if (!a) return npfail("NULL arguments");
    if (a->N <= 0 || a->A <= 0) return npfail("bad dimensions");
    if (a->A > CAT_RENDER_MAX_AGENTS) return npfail("more agents than CAT_RENDER_MAX_AGENTS");
    if (a->n_cops < 1 || a->n_cops > a->A - 1) return npfail("n_cops must lie in 1 .. A - 1");
    if (a->n_maps < 1 || a->n_maps > CAT_NAV_MAX_MAPS) return npfail("n_maps must lie in 1 .. 16");
    if (a->cell < 1) return npfail("cell must be >= 1");
    if (!a->grid || !a->free || !a->hops) return npfail("a table of the field is NULL");
    if (!a->mask || !a->band || !a->uniform || !a->positions || !a->placed) return npfail("a required buffer is NULL");
    if ((uintptr_t)a->positions & 7) return npfail("positions must be 8-byte aligned");
    const unsigned per = NAV_BLOCK / SPAWN_WAVE;
    hipLaunchKernelGGL(nav_spawn_kernel, dim3(((unsigned)a->N + per - 1) / per), dim3(NAV_BLOCK), 0, (hipStream_t)stream, *a);
    return launched("cat_render_nav_spawn");
}

extern "C" int cat_render_abi_version(void) { return CAT_RENDER_ABI_VERSION; }
extern "C" const char *cat_render_last_error(void) { return g_err; }

extern "C" int cat_render_frames(const cat_render_scene *sc, const cat_render_args *a, void *stream)
{
    if (!sc || !a) return fail("NULL scene or arguments");
    if (sc->n_maps <= 0 || !sc->window || !sc->window_host || !sc->shape_off || !sc->shape_off_host || !sc->shape_bb ||
        !sc->shape_first || !sc->shape_count || !sc->planes)
        return fail("incomplete scene");
    if (a->F <= 0 || a->width <= 0 || a->height <= 0 || a->A <= 0 || a->A > CAT_RENDER_MAX_AGENTS || a->n_cops < 0 || a->n_cops > a->A)
        return fail("bad dimensions");
    if (!(a->agent_radius >= 0.0) || !isfinite(a->agent_radius)) return fail("agent_radius must be finite and >= 0");
    if (a->flags & ~CAT_RENDER_RAYS) return fail("unknown flags");
    const bool rays = a->flags & CAT_RENDER_RAYS;
    if (rays) {
        if (a->R <= 0 || a->R != sc->n_rays || !sc->ray_dx || !sc->ray_dy) return fail("rays: R must equal the scene's ray table");
        if (!(a->ray_length > 0.0) || !isfinite(a->ray_length)) return fail("rays: ray_length must be finite and > 0");
        if (!a->obs_distance || !a->obs_type) return fail("rays: obs_distance / obs_type is NULL");
    }
    if (!a->map_ids || !a->map_ids_dev || !a->positions || !a->frames) return fail("a required buffer is NULL");
    for (int f = 0; f < a->F; ++f) {
        const int m = a->map_ids[f];
        if (m < 0 || m >= sc->n_maps) {
            snprintf(g_err, sizeof g_err, "cat_render_frames: map_ids[%d] = %d outside [0, %d)", f, m, sc->n_maps);
            return CAT_RENDER_ERR_BAD_ARG;
        }
        if (sc->window_host[2 * m] > a->width || sc->window_host[2 * m + 1] > a->height) {
            snprintf(g_err, sizeof g_err, "cat_render_frames: frame %d: map %d's window %dx%d exceeds the frame size %dx%d", f, m,
                     sc->window_host[2 * m], sc->window_host[2 * m + 1], a->width, a->height);
            return CAT_RENDER_ERR_BAD_ARG;
        }
    }
    const long long tiles_x = (a->width + TX - 1) / TX, tiles_y = (a->height + TY - 1) / TY;
    const long long blocks = tiles_x * tiles_y * a->F;
    if (blocks > INT32_MAX) return fail("too many frames for one launch");
    hipLaunchKernelGGL(render_tiles_kernel, dim3((unsigned)blocks), dim3(BLOCK), 0, (hipStream_t)stream, *sc, *a, (int)tiles_x, (int)tiles_y);
    return launched("cat_render_frames");
}
