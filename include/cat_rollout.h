/*
 * cat_rollout.h -- C ABI of libcat_learn.so, part 5: the glue of a rollout tick between the env core and the networks
 * (observation -> model-input packing; rank 2: action sampling), one launch each instead
 * of ~30 / ~20 small tensor kernels per tick.
 *
 *  - cat_rollout_pack: libcat_sim.so's observation buffers -> the networks' input rows, in the layouts skrl's flattening
 *    of the reference's Dict spaces produces (src/models/lstm_policy_net.py:101-103: policy row = [distance(R) |
 *    object_type(R)]; src/models/lstm_value_net.py:122-137: critic row = the first 4R entries of an agent's shared state
 *    in sorted-key order = [distance_shared | object_type_shared | own_distances | own_obj_types]; SURVEY quirk Q11: the
 *    reference feeds every critic the FIRST agent's state), scaled and stored as bf16.
 *  - cat_rollout_sample: one categorical draw per (agent, env) from the policy logits by inverse CDF on a supplied
 *    uniform number, with the log-probability of the drawn action, written where the rollout keeps them, and the action
 *    into the env's [N][A] action matrix.
 *  - cat_rollout_scripted: the same place for agents that follow a fixed rule instead of a network: the env core's observation
 *    buffers -> the action matrix, for the scripted chase / evade opponents.
 *
 * Conventions as in cat_sim.h.
 */
#ifndef CAT_ROLLOUT_H
#define CAT_ROLLOUT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CAT_ROLLOUT_ABI_VERSION 1
#define CAT_ROLLOUT_MAX_AGENTS 8

enum { CAT_ROLLOUT_OK = 0, CAT_ROLLOUT_ERR_BAD_ARG = -1, CAT_ROLLOUT_ERR_HIP = -2 };

typedef struct cat_rollout_pack_args {
    int32_t N, A, R, G;                         /* envs, agents in the env, rays, agents packed by this call */
    int32_t agent[CAT_ROLLOUT_MAX_AGENTS];      /* env agent index of packed agent g */
    int32_t n_cops;                             /* agents [0, n_cops) are team 0 */
    int32_t first_agent_state;                  /* 1: every critic row is built from env agent 0 (reference quirk Q11) */
    float distance_scale, type_scale;
    const void *obs_distance;                   /* f16 [N][A][R]   (cat_outputs.obs_distance) */
    const void *obs_type;                       /* u8  [N][A][R] */
    const void *shared_distance;                /* f16 [N][2][R] */
    const void *shared_type;                    /* u8  [N][2][R] */
    void *policy_in;                            /* bf16 [G][N][2R], strides below (elements) */
    int64_t sp_g, sp_n;
    void *value_in;                             /* bf16 [G][N][4R] */
    int64_t sv_g, sv_n;
} cat_rollout_pack_args;

typedef struct cat_rollout_sample_args {
    int32_t N, A, G, pad;
    int32_t agent[CAT_ROLLOUT_MAX_AGENTS];      /* column of packed agent g in the action matrix */
    const void *logits;                         /* bf16 [G][N][4] contiguous */
    const float *uniform;                       /* [G][N] in [0, 1) */
    const void *values;                         /* bf16 [G][N] contiguous or NULL */
    int64_t *act_out;                           /* [G][N], row stride sa_g */
    float *logp_out;                            /* [G][N], row stride sl_g */
    float *value_out;                           /* [G][N], row stride sl_g; or NULL */
    int64_t sa_g, sl_g;
    int32_t *actions;                           /* [N][A] */
} cat_rollout_sample_args;

/* After the env tick: the agents' rewards into the rollout's [G][N] rows, and the episode-end flags (cat_outputs.terminated,
   u8 [N]) as the rollout keeps them: done_out / start_out (bool = 1 byte) and keep_out = 1 - terminated as fp32 (the recurrent
   networks' "carry the state" mask of the NEXT tick).  Any of the three flag outputs may be NULL. */
typedef struct cat_rollout_post_args {
    int32_t N, A, G, pad;
    int32_t agent[CAT_ROLLOUT_MAX_AGENTS];
    const float *reward;                        /* [N][A] (cat_outputs.reward) */
    const uint8_t *terminated;                  /* [N] */
    float *reward_out;                          /* [G][N], row stride sr_g */
    int64_t sr_g;
    uint8_t *done_out, *start_out;              /* [N] */
    float *keep_out;                            /* [N] */
} cat_rollout_post_args;
int cat_rollout_post(const cat_rollout_post_args *a, void *stream);

/* Scripted opponents: a deterministic, parameter-free rule from an agent's own ray fan to its action, one launch for all (policy g,
   env n) rows, where cat_rollout_sample / cat_act_step sit.  Script CAT_ROLLOUT_CHASE heads for the nearest ray of type target[g] (a
   cop's: THIEF = 2) and for where it last saw one for memory_ticks more ticks; CAT_ROLLOUT_EVADE runs from it (a thief's target:
   COP = 1).  Both keep clear of what their ray fan shows closer than clear_min in the cone of the direction they take, and wander
   (hold the heading, turn with probability turn_prob) when they have no bearing.  All integer arithmetic but the two fp32
   comparisons free >= clear_min and uniform < turn_prob; as_cops_and_thieves_amd/selfplay/scripted.py states the rule in full and
   the kernel equals it bit for bit.
   Rows seg_start[s] .. seg_start[s + 1] - 1 of policy g follow seg_script[g][s]; -1: neither the action column nor the state row of
   those rows is touched.  S = 1 is the plain form.  state rows are (valid, heading, mem_ray, ttl); keep as in cat_act_step: 0 takes
   the row's state as all zero before the tick, NULL carries every state.  No atomics, no allocation, no synchronisation. */
#define CAT_ROLLOUT_MAX_SEGMENTS 32
#define CAT_ROLLOUT_MIN_RAYS 8
#define CAT_ROLLOUT_MAX_RAYS 1024
enum { CAT_ROLLOUT_CHASE = 0, CAT_ROLLOUT_EVADE = 1 };

typedef struct cat_rollout_scripted_args {
    int32_t N, A, R, G;                         /* envs, agents in the env, rays (8 .. 1024), scripted policies (<= 8) */
    int32_t agent[CAT_ROLLOUT_MAX_AGENTS];      /* env agent index of policy g: its observation row and its action column */
    int32_t target[CAT_ROLLOUT_MAX_AGENTS];     /* the type code policy g looks for: 1 (cop) or 2 (thief) */
    int32_t memory_ticks;                       /* >= 0: ticks a lost bearing is still followed */
    float clear_min;                            /* >= 0: a cone is free when nothing but the target is closer than this */
    float turn_prob;                            /* in [0, 1]: chance per tick of a turn while wandering */
    int32_t S;                                  /* segments, 1 .. CAT_ROLLOUT_MAX_SEGMENTS */
    int32_t seg_start[CAT_ROLLOUT_MAX_SEGMENTS + 1];                        /* 0 first, N last, strictly increasing */
    int32_t seg_script[CAT_ROLLOUT_MAX_AGENTS][CAT_ROLLOUT_MAX_SEGMENTS];   /* [g][s]: CAT_ROLLOUT_CHASE / _EVADE / -1 */
    const void *obs_distance;                   /* f16 [N][A][R], non-negative and finite */
    const void *obs_type;                       /* u8  [N][A][R] */
    const float *uniform;                       /* [G][N] in [0, 1) */
    const float *keep;                          /* [N] or NULL */
    int32_t *state;                             /* [G][N][4], 16-byte aligned, updated in place */
    int32_t *actions;                           /* [N][A] */
} cat_rollout_scripted_args;
int cat_rollout_scripted(const cat_rollout_scripted_args *a, void *stream);

int cat_rollout_abi_version(void);
const char *cat_rollout_last_error(void);
int cat_rollout_pack(const cat_rollout_pack_args *a, void *stream);
int cat_rollout_sample(const cat_rollout_sample_args *a, void *stream);

#ifdef __cplusplus
}
#endif
#endif
