/*
 * cat_render.h -- C ABI of libcat_learn.so, part 6: batched rgb_array frames of the env core's state, drawn on the GPU
 * straight from device buffers (many frames per launch, no host copy of the state).
 *
 * Pixel contract: render.render_frame_reference (NumPy) defines every byte; render.render_rgb_array when no rays are drawn.
 *   frame [width][height][3] uint8, x-major (the layout of pygame's surfarray); pixel (x, y) has its centre at (x + .5, y + .5).
 *   Later layers overwrite earlier ones:
 *   1. white background, then walls grey (60,60,60): the pixels of a wall's clipped bounding-box window
 *      [max(int(l),0), min(int(r)+1,W)) x [max(int(b),0), min(int(t)+1,H)) with pl[0]*X + pl[1]*Y - pl[4] <= 1.0 on every plane;
 *   2. with CAT_RENDER_RAYS: every agent's ray fan, agent by agent, ray by ray -- the segment from the agent's position to
 *      position + (distance / ray_length) * (ray_dx[k], ray_dy[k]) in float64, lit where the pixel centre's squared distance to the
 *      segment is <= 0.25, inside the window [int(min)-1, int(max)+2) of the segment's bounding box, coloured by obs_type;
 *   3. the agents' discs: (X-px)^2 + (Y-py)^2 <= r^2 inside [int(px-r)-1, int(px+r)+2), blue (0,0,255) for agents < n_cops,
 *      red (255,0,0) after; a later agent overwrites an earlier one.
 *   W, H are the frame's own map window (int(window)); everything is clipped to it, and pixels of the frame beyond it are 255.
 *   All arithmetic is binary64 without contraction, in the order the reference writes it.
 *
 * Conventions as in cat_rollout.h (status codes, stream as void*, no CPU fallback).  Bad arguments return
 * CAT_RENDER_ERR_BAD_ARG with a message in cat_render_last_error() before any device call.
 */
#ifndef CAT_RENDER_H
#define CAT_RENDER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CAT_RENDER_ABI_VERSION 1
#define CAT_RENDER_MAX_AGENTS 16
#define CAT_RENDER_RAYS 1            /* flags: draw the agents' ray fans */

enum { CAT_RENDER_OK = 0, CAT_RENDER_ERR_BAD_ARG = -1, CAT_RENDER_ERR_HIP = -2 };

/* ray colours by object type (WALL, COP, THIEF, MOVABLE, EMPTY); a type above 4 is drawn as EMPTY */
#define CAT_RENDER_RAY_COLOURS { {255, 140, 0}, {0, 170, 255}, {255, 60, 160}, {0, 160, 0}, {190, 190, 190} }

/* The maps of a batch, concatenated, uploaded once.  DEVICE pointers unless marked HOST. */
typedef struct cat_render_scene {
    int32_t n_maps;               /* M */
    int32_t n_rays;               /* R of the ray table */
    const int32_t *window;        /* [M][2] int(window): frame pixels of map m are [0, W) x [0, H) */
    const int32_t *window_host;   /* HOST [M][2], the same values (argument checks) */
    const int32_t *shape_off;     /* [M + 1] first wall of map m in the lists below; shape_off[M] = S */
    const int32_t *shape_off_host;/* HOST [M + 1], the same values */
    const double *shape_bb;       /* [S][4] l, b, r, t (CompiledMap.shape_bb) */
    const int32_t *shape_first;   /* [S] first plane of the wall in `planes` (already offset to the concatenated list) */
    const int32_t *shape_count;   /* [S] */
    const double *planes;         /* [P][5] the first five doubles of CompiledMap.planes */
    const double *ray_dx;         /* [R] ray_length * cos(angle) (tables.ray_table) */
    const double *ray_dy;         /* [R] */
} cat_render_scene;

typedef struct cat_render_args {
    int32_t F;                    /* frames */
    int32_t width, height;        /* frame size; at least the window of every map drawn */
    int32_t flags;                /* CAT_RENDER_RAYS */
    int32_t n_cops, A, R, pad;    /* agents [0, n_cops) are cops; R = scene n_rays when rays are drawn */
    double agent_radius, ray_length;
    const int32_t *map_ids;       /* HOST [F] map of frame f (checked against n_maps and the frame size) */
    const int32_t *map_ids_dev;   /* [F] the same values on the device */
    const double *positions;      /* [F][A][2] */
    const uint16_t *obs_distance; /* [F][A][R] float16 bits (cat_outputs.obs_distance); CAT_RENDER_RAYS only */
    const uint8_t *obs_type;      /* [F][A][R] ObjectType; CAT_RENDER_RAYS only */
    uint8_t *frames;              /* [F][width][height][3], any byte alignment */
} cat_render_args;

int cat_render_abi_version(void);
const char *cat_render_last_error(void);
int cat_render_frames(const cat_render_scene *scene, const cat_render_args *a, void *stream);

/*
 * Position statistics: where the agents spend their time.  cat_render_positions_update adds T >= 1 consecutive rows of N slots (the
 * env core's team_positions / obs_type / terminated buffers, with a leading T from cat_rollout_fused) into per-group count maps on a
 * grid of cell x cell pixels, in ONE launch without allocation or synchronisation (capturable with the env tick it follows).
 * positions.PositionTracker (NumPy) defines every number.
 *
 *   Grid: Wc = ceil(W / cell), Hc = ceil(H / cell) cells, W x H the largest map window of the batch; all groups share it.
 *   group[n] in 0 .. G-1 is the group of slot n, anything else (-1) means "not counted"; NULL = every slot in group 0.
 *   counts [G][3][A][Wc][Hc] int64, x-major like the frames, planes CAT_POSITIONS_OCC / _SEEN / _SPAWN; outside [G][A] int64;
 *   rows [G] int64 slot-rows counted; done [N] int32 terminal rows the slot has had.
 *
 *   Row t of slot n, g = group[n]: skipped if g is no group, or if quota is non-NULL and done[n] >= quota[n].  Otherwise rows[g] += 1;
 *   term = terminated[t][n] != 0; for every agent a, (x, y) are the two f16 values of team_positions[t][n][a].  The position is valid
 *   iff both are finite, x >= 0, y >= 0, cx = (int)floor(x) / cell < Wc and cy = (int)floor(y) / cell < Hc (integer division).
 *   Invalid: outside[g][a] += 1.  Valid and term: counts[g][SPAWN][a][cx][cy] += 1 (the env resets a slot inside its terminal tick, so
 *   a terminal row holds the first position of the NEW episode; where the old one ended: cat_render_positions_ends_update below).  Valid and
 *   not term: counts[g][OCC][a][cx][cy] += 1 and, if obs_type is given and seen(a) holds, counts[g][SEEN][a][cx][cy] += 1.  Finally
 *   done[n] += term.
 *   seen(a): some agent b of the OTHER role has a ray k with obs_type[t][n][b][k] == a's role code (CAT_COP = 1 for a < n_cops,
 *   CAT_THIEF = 2 after).  This is role-level: with two agents of one role it says "an agent of my role is in an opponent's sight";
 *   obs_type cannot tell which one.
 *
 * All sums are integers (64-bit global atomics): the result does not depend on the order or on how rows are chunked into launches.
 */
#define CAT_POSITIONS_OCC 0
#define CAT_POSITIONS_SEEN 1
#define CAT_POSITIONS_SPAWN 2
#define CAT_POSITIONS_MAX_TICKS 65536    /* = CAT_MAX_ROLLOUT_TICKS */

typedef struct cat_render_positions_args {
    int32_t T, N, A, n_cops;      /* rows, slots, agents (<= CAT_RENDER_MAX_AGENTS), agents [0, n_cops) are cops */
    int32_t R, cell, Wc, Hc;      /* rays per agent (obs_type only), cell size in pixels (>= 1), grid cells */
    int32_t G, pad;               /* groups (>= 1) */
    const uint16_t *team_positions; /* [T][N][A][2] float16 bits (cat_outputs.team_positions), 4-byte aligned */
    const uint8_t *terminated;    /* [T][N] */
    const uint8_t *obs_type;      /* [T][N][A][R] ObjectType, any byte alignment, or NULL = no SEEN plane */
    const int32_t *group;         /* [N] or NULL = all slots in group 0 */
    const int32_t *quota;         /* [N] or NULL = unlimited */
    int64_t *counts;              /* [G][3][A][Wc][Hc] */
    int64_t *outside;             /* [G][A] */
    int64_t *rows;                /* [G] */
    int32_t *done;                /* [N] */
} cat_render_positions_args;

/* An entry added after ABI version 1 was fixed (cat_render_frames and its two structs are unchanged). */
int cat_render_positions_update(const cat_render_positions_args *a, void *stream);

/*
 * Where episodes END: capture and timeout maps.  cat_render_positions_ends_update adds T >= 1 consecutive rows of the env core's end-of-episode
 * positions (cat_bind_final_positions, include/cat_sim.h: on a terminal row the tick-start positions of the episode that ended, any other row is
 * never read) into ends [G][2][A][Wc][Hc] int64, planes CAT_POSITIONS_CAPTURE / _TIMEOUT, and ends_outside [G][2][A] int64, on the grid and with
 * the groups of cat_render_positions_update.  One launch, no allocation, no synchronisation (capturable).
 *
 *   Row t of slot n, g = group[n]: skipped if g is no group, or if quota is non-NULL and d[n] >= quota[n], where d[n] starts at done_before[n]
 *   (0 where done_before is NULL) and grows by one with every terminal row of the slot in this call -- the quota rule of
 *   cat_render_positions_update.  done_before is only read: give this entry the positions update's `done` BEFORE that update has advanced it over
 *   the same rows (run this entry first, or pass a copy).  Only rows with terminated[t][n] != 0 count: plane = truncated[t][n] != 0 ? TIMEOUT :
 *   CAPTURE; for every agent a, (x, y) are the two f16 values of final_positions[t][n][a], valid iff both are finite, x >= 0, y >= 0,
 *   cx = (int)floor(x) / cell < Wc and cy = (int)floor(y) / cell < Hc (integer division).  Invalid: ends_outside[g][plane][a] += 1.
 *   Valid: ends[g][plane][a][cx][cy] += 1.
 *
 * All sums are integers (64-bit global atomics): the result does not depend on the order or on how rows are chunked into launches (with
 * done_before carried along).  positions.PositionTracker (NumPy) defines every number.
 */
#define CAT_POSITIONS_CAPTURE 0
#define CAT_POSITIONS_TIMEOUT 1

typedef struct cat_render_positions_ends_args {
    int32_t T, N, A, cell;          /* rows, slots, agents (<= CAT_RENDER_MAX_AGENTS), cell size in pixels (>= 1) */
    int32_t Wc, Hc, G, pad;         /* grid cells, groups (>= 1) */
    const uint16_t *final_positions;/* [T][N][A][2] float16 bits, 4-byte aligned; read on terminal rows only */
    const uint8_t *terminated;      /* [T][N] */
    const uint8_t *truncated;       /* [T][N] */
    const int32_t *group;           /* [N] or NULL = all slots in group 0 */
    const int32_t *quota;           /* [N] or NULL = unlimited */
    const int32_t *done_before;     /* [N] terminal rows each slot had before row 0, or NULL = none; read only */
    int64_t *ends;                  /* [G][2][A][Wc][Hc] */
    int64_t *ends_outside;          /* [G][2][A] */
} cat_render_positions_ends_args;

/* An entry added after ABI version 1 was fixed (the entries and structs above are unchanged). */
int cat_render_positions_ends_update(const cat_render_positions_ends_args *a, void *stream);

/*
 * Navigation: shortest paths around the walls, for the PRIVILEGED yardstick opponents "pursue" and "flee" (selfplay/navigators.py), which
 * read team_positions and the map -- information no policy sees -- and for geodesic separation as a metric.  navigation.py (NumPy / torch)
 * defines every number: hops_reference the table, navigate_step the tick.
 *
 * The field of a batch of M <= CAT_NAV_MAX_MAPS maps.  Map m has a grid of Wc x Hc cells of cell x cell pixels, C = Wc * Hc <=
 * CAT_NAV_MAX_CELLS, cell (ix, iy) at index k = ix * Hc + iy (x-major, like the position statistics).
 *   grid [M][4] int32: Wc, Hc, cell_off, hops_off -- map m's first element in the per-cell arrays (free, snap) and in hops.  hops_off is
 *     the plain ELEMENT offset: M * C^2 <= 16 * 4096^2 = 2^28 fits an int32, so no scaled offset and no 64-bit table beside it is needed.
 *   free [sum C] uint8: 1 = an agent's centre may stand on the cell's centre.
 *   snap [sum C] uint16: a free cell is its own; a blocked one names the nearest free cell within two rings, or CAT_NAV_NONE.
 *   hops [sum C^2] uint16: hops[hops_off + goal * C + k] = 4-connected steps over free cells from k to goal; CAT_NAV_NONE where goal or k
 *     is blocked or no path exists.  Symmetric.
 *
 * cat_render_nav_build fills hops from free: one workgroup of 256 threads per (map, goal), the goal's row in LDS (C uint16 <= 8 KiB),
 * level-synchronous sweeps (in level L every unvisited free cell with a 4-neighbour at distance L takes L + 1) until a level changes
 * nothing, then the row goes out in coalesced 16-bit stores.  No global atomics, no waiting between workgroups, no allocation: capturable.
 */
#define CAT_NAV_MAX_CELLS 4096
#define CAT_NAV_MAX_MAPS 16
#define CAT_NAV_NONE 0xFFFF
#define CAT_NAV_MAX_NAVIGATORS 8
#define CAT_NAV_MAX_SEGMENTS 32      /* = CAT_ROLLOUT_MAX_SEGMENTS */
#define CAT_NAV_PURSUE 0
#define CAT_NAV_FLEE 1

typedef struct cat_render_nav_build_args {
    int32_t n_maps, pad;            /* 1 .. CAT_NAV_MAX_MAPS */
    const int32_t *grid_host;       /* HOST [n_maps][4] (argument checks and the launch size) */
    const int32_t *grid;            /* [n_maps][4] the same values on the device */
    const uint8_t *free;            /* [sum C] */
    uint16_t *hops;                 /* [sum C^2], 2-byte aligned */
} cat_render_nav_build_args;

/* An entry added after ABI version 1 was fixed (the entries and structs above are unchanged). */
int cat_render_nav_build(const cat_render_nav_build_args *a, void *stream);

/*
 * One tick of G <= CAT_NAV_MAX_NAVIGATORS navigators over N slots in ONE launch: a thread per row (navigator g, slot n), workgroups of 256,
 * no LDS, no atomics, no allocation (capturable).  Actions as in cat_rollout_scripted: 0 = -x, 1 = +y, 2 = +x, 3 = -y.
 *
 *   script = seg_script[g][s] for the segment s with seg_start[s] <= n < seg_start[s + 1]; -1: the row touches nothing.
 *   Map m = slot_map[n] (0 where slot_map is NULL).  The cell of a position (x, y), the two f16 values of team_positions[n][j]: both
 *   finite, x >= 0, y >= 0, ix = (int)floor(x) / cell < Wc, iy = (int)floor(y) / cell < Hc, then snap[ix * Hc + iy]; CAT_NAV_NONE is no cell.
 *   a = the cell of agent[g]; the opponents j are the bits of opp_mask[g], b_j their cells; H(b, k) = hops[b][k].
 *   Target: among the opponents with a cell and H(b_j, a) != CAT_NAV_NONE the smallest key (H(b_j, a) << 8) | j; d = its H, b = its cell.
 *   Fallback: no a, no target, or none of a's four neighbours usable (on the grid and free): action = min(3, (int)(4 u)), nav_hops = -1.
 *   pref: with D = target position - own position in fp32, the x axis if |D.x| >= |D.y| else y; on x: 2 if D.x >= 0 else 0, on y: 1 if
 *   D.y >= 0 else 3.
 *   Pursue: d == 0 (one cell): pref.  Otherwise, over the usable neighbours nb_i (i = the action that leads there) the minimum of
 *   H(b, nb_i); among those that reach it pref if it is one of them, else the lowest i.
 *   Flee: m_i = min and t_i = sum (int32) over ALL opponents with a cell of H(b_j, nb_i), CAT_NAV_NONE counting as 65535; the largest m_i,
 *   then the largest t_i, then the lowest i.
 *   actions[n][agent[g]] = the action; nav_hops[g][n] (where given) = d, or -1 after the fallback.
 */
typedef struct cat_render_nav_step_args {
    int32_t N, A, G, S;             /* slots, agents (<= CAT_RENDER_MAX_AGENTS), navigators, segments (1 .. CAT_NAV_MAX_SEGMENTS) */
    int32_t n_maps, cell;           /* maps of the field (1 .. CAT_NAV_MAX_MAPS), cell size in pixels (>= 1) */
    int32_t agent[CAT_NAV_MAX_NAVIGATORS];       /* navigator g's column of team_positions / actions */
    uint32_t opp_mask[CAT_NAV_MAX_NAVIGATORS];   /* bit j: agent j is an opponent of navigator g (not agent[g] itself, j < A) */
    int32_t seg_start[CAT_NAV_MAX_SEGMENTS + 1]; /* seg_start[0] = 0 < ... < seg_start[S] = N */
    int32_t pad;
    int32_t seg_script[CAT_NAV_MAX_NAVIGATORS][CAT_NAV_MAX_SEGMENTS];   /* CAT_NAV_PURSUE, CAT_NAV_FLEE or -1 */
    const int32_t *grid;            /* [n_maps][4] */
    const uint8_t *free;            /* [sum C] */
    const uint16_t *snap;           /* [sum C] */
    const uint16_t *hops;           /* [sum C^2] */
    const int32_t *slot_map;        /* [N] map of slot n, or NULL = map 0 */
    const uint16_t *team_positions; /* [N][A][2] float16 bits (cat_outputs.team_positions), 4-byte aligned */
    const float *uniform;           /* [G][N] in [0, 1) */
    int32_t *actions;               /* [N][A]; only column agent[g] of rows with a script is written */
    int32_t *nav_hops;              /* [G][N] or NULL; rows of -1 segments are not written */
} cat_render_nav_step_args;

/* An entry added after ABI version 1 was fixed (the entries and structs above are unchanged). */
int cat_render_nav_step(const cat_render_nav_step_args *a, void *stream);

/*
 * Geodesic potential-based reward shaping (Ng, Harada and Russell 1999): one tick of G <= CAT_NAV_MAX_NAVIGATORS shaped agents over N slots in
 * ONE launch -- a thread per slot, which finds the cells of the slot's A agents once and then walks the G rows; workgroups of 256, no LDS, no
 * atomics, no allocation, no synchronisation (capturable).  A row's state and outputs are touched by the thread of its slot alone.
 * navigation.py (separation, shaping_step) defines every number; the fp32 results are bit-equal to it (this file is compiled without a*b+c
 * contraction).
 *
 *   Map m = slot_map[n] (0 where slot_map is NULL); the cell of a position as in cat_render_nav_step.
 *   separation(P, g), P an [N][A][2] f16 position array: a = the cell of P[n][agent[g]]; the smallest hops[b_j][a] over the opponents j (the
 *   bits of opp_mask[g]) that have a cell and whose entry is not CAT_NAV_NONE; -1 if there is no a or no such opponent.
 *   phi(g, d) = coef[g] * (float)min(d, cap) for d >= 0: one rounded multiply, the conversion is exact.
 *   Row (g, n), d0 = hops_prev[g][n] (the separation at the start of the tick):
 *     terminated[n] and not truncated[n] (a capture, a true terminal state): phi1 = +0.0f, defined;
 *     terminated[n] and truncated[n] (the time limit, no property of the state): d1 = separation(final_positions, g);
 *     otherwise d1 = separation(team_positions, g);  phi1 = phi(g, d1) where d1 >= 0.
 *     F = +0.0f if d0 < 0 or a needed d1 < 0, else (gamma * phi1) - phi(g, d0): two rounded operations in that order.
 *     reward_out[g * sr_g + n] += F (the add is always performed: -0.0f + +0.0f = +0.0f); shaping_out[g * ss_g + n] = F where given;
 *     hops_prev[g][n] = separation(team_positions, g), always -- on a terminal row the NEW episode's first state (the env resets in the tick).
 *   prime != 0: only the last assignment; final_positions, terminated, truncated, reward_out and shaping_out are not touched and may be NULL.
 *   final_positions is read on rows with terminated and truncated both set and on no other row (those hold stale positions or NaN).
 */
typedef struct cat_render_nav_shape_args {
    int32_t N, A, G, n_maps;        /* slots, agents (<= CAT_RENDER_MAX_AGENTS), shaped agents, maps of the field (1 .. CAT_NAV_MAX_MAPS) */
    int32_t cell, cap, prime, pad;  /* cell size in pixels (>= 1), hop cap (1 .. 65534), prime mode (0 / 1) */
    int32_t agent[CAT_NAV_MAX_NAVIGATORS];       /* shaped agent g's column of the position arrays */
    uint32_t opp_mask[CAT_NAV_MAX_NAVIGATORS];   /* bit j: agent j is an opponent of g (not agent[g] itself, j < A) */
    float coef[CAT_NAV_MAX_NAVIGATORS];          /* finite; negative for a cop, positive for a thief */
    float gamma;                    /* the learner's discount factor: finite, >= 0 */
    int32_t pad2;
    const int32_t *grid;            /* [n_maps][4] */
    const uint16_t *snap;           /* [sum C] */
    const uint16_t *hops;           /* [sum C^2] */
    const int32_t *slot_map;        /* [N] map of slot n, or NULL = map 0 */
    const uint16_t *team_positions; /* [N][A][2] float16 bits (cat_outputs.team_positions), 4-byte aligned */
    const uint16_t *final_positions;/* [N][A][2] float16 bits (cat_bind_final_positions), 4-byte aligned; may be NULL only if prime */
    const uint8_t *terminated;      /* [N] */
    const uint8_t *truncated;       /* [N] */
    float *reward_out;              /* row g begins at element g * sr_g, N elements */
    int64_t sr_g;                   /* >= N where G > 1 */
    float *shaping_out;             /* row g begins at element g * ss_g, or NULL */
    int64_t ss_g;                   /* >= N where G > 1 and shaping_out is given */
    int32_t *hops_prev;             /* [G][N] */
} cat_render_nav_shape_args;

/* An entry added after ABI version 1 was fixed (the entries and structs above are unchanged). */
int cat_render_nav_shape(const cat_render_nav_shape_args *a, void *stream);

/*
 * A geodesic start-state curriculum: start positions for the masked slots such that every cop stands a chosen number of shortest-path hops
 * from a thief, in ONE launch -- a wavefront (64 lanes) per slot, workgroups of 256 = four slots; no LDS, no atomics, no scratch, no
 * allocation, no synchronisation (capturable).  navigation.spawn_step defines every number: cells are integers, positions exact f64.
 *
 *   Slot n takes part iff mask[n] != 0 and (lo, hi) = band[n] satisfies 1 <= lo <= hi <= 65534; any other band keeps the map's own spawn.  A
 *   slot that does not take part leaves after its mask byte and band (the common case: a few slots end per tick) with placed[n] = 0.
 *   Map m = slot_map[n] (0 where slot_map is NULL).  Agents 0 .. n_cops - 1 are the cops, the rest the thieves (the env's order).
 *   Placement order: the thieves in env order, then the cops in env order; the i-th placed agent draws with u = uniform[i][n] in [0, 1):
 *     among cnt candidates in cell-index order the one at rank j = min(cnt - 1, (int)(u * (float)cnt)) -- one rounded fp32 multiply.
 *     Thief 0 (the anchor): every free cell.  A further thief: the free cells k with hops[anchor][k] != CAT_NAV_NONE not taken by an earlier
 *     agent.  A cop: the free cells k not taken with lo <= d(k) <= hi, d(k) the smallest hops[b_j][k] over the placed thieves' cells b_j,
 *     CAT_NAV_NONE entries ignored (all CAT_NAV_NONE: no candidate).
 *   Per agent the wave sweeps the map's cells 64 at a time, a lane a cell (free and the thieves' hop rows are read coalesced); the predicate
 *   goes through a ballot, a chunk's count is its popcount; a second sweep stops in the chunk where the running count passes j and takes its
 *   (j - before)-th set bit.  The cells chosen so far live one per lane and are read back with a lane read.
 *   cnt == 0 for any agent: placed[n] = 0 and positions[n] is NOT written.  Otherwise placed[n] = 1 and positions[n][agent] = the cell's
 *   centre ((ix + .5) cell, (iy + .5) cell).  Nothing is checked about captures (lo = 1 puts a cop inside the termination radius).
 */
typedef struct cat_render_nav_spawn_args {
    int32_t N, A, n_cops, n_maps;   /* slots, agents (<= CAT_RENDER_MAX_AGENTS), cops (1 .. A - 1), maps of the field (1 .. CAT_NAV_MAX_MAPS) */
    int32_t cell, pad;              /* cell size in pixels (>= 1) */
    const int32_t *grid;            /* [n_maps][4] */
    const uint8_t *free;            /* [sum C] */
    const uint16_t *hops;           /* [sum C^2] */
    const int32_t *slot_map;        /* [N] map of slot n, or NULL = map 0 */
    const uint8_t *mask;            /* [N] */
    const int32_t *band;            /* [N][2] lo, hi */
    const float *uniform;           /* [A][N] in [0, 1) */
    double *positions;              /* [N][A][2], 8-byte aligned (cat_reset's positions); rows with placed[n] == 0 are not written */
    uint8_t *placed;                /* [N], every row written */
} cat_render_nav_spawn_args;

/* An entry added after ABI version 1 was fixed (the entries and structs above are unchanged). */
int cat_render_nav_spawn(const cat_render_nav_spawn_args *a, void *stream);

#ifdef __cplusplus
}
#endif
#endif
