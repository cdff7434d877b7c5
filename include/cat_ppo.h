/*
 * cat_ppo.h -- C ABI of libcat_learn.so, part 3: the PPO loss (with its gradient) and the optimiser step of the
 * self-play learner, each as one or two launches instead of dozens of elementwise
 * kernels.  What is restated: skrl's MAPPO update as configured by the reference (src/configs/mappo_config.py:5-50 --
 * clipped surrogate, entropy bonus, scaled MSE value loss, KL early stop, gradient-norm clip, Adam); [SKRL-RECALL], as
 * the torch formulation in as_cops_and_thieves_amd/selfplay/mappo.py which these kernels are tested against.
 *
 * Conventions as in cat_sim.h (status codes, device buffers, stream as void*, no CPU fallback).
 */
#ifndef CAT_PPO_H
#define CAT_PPO_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CAT_PPO_ABI_VERSION 2
#define CAT_PPO_ACTIONS 4            /* the four impulse actions of every agent (cat_sim.h, cat_step) */
#define CAT_PPO_MAX_CHUNKS 256

enum { CAT_PPO_OK = 0, CAT_PPO_ERR_BAD_ARG = -1, CAT_PPO_ERR_HIP = -2 };

/* For each of the G agents, over its M samples:
 *   surrogate = sum min(adv ratio, adv clamp(ratio, 1 - clip, 1 + clip)),  ratio = exp(logp(action) - old_logp)
 *   sq_error  = sum (value - ret)^2
 *   entropy   = sum -sum_j p_j log p_j
 *   kl        = sum (ratio - 1) - (logp - old_logp)
 * partial[g][chunk] = {surrogate, sq_error, entropy, kl} of one chunk of the samples (the caller adds the chunks up), and
 * the gradient of   L = sum_g ( -surrogate_g - entropy_scale entropy_g + value_scale sq_error_g ) / M
 * w.r.t. the logits and the values. */
typedef struct cat_ppo_loss {
    int32_t G, M, chunks, pad;
    const void *logits;         /* bf16 [G][M][4] */
    const void *values;         /* bf16 [G][M] */
    const int64_t *actions;     /* [G][M], 0..3 */
    const float *old_logp, *adv, *ret;   /* [G][M] */
    float ratio_clip, value_scale, entropy_scale, pad2;
    void *d_logits;             /* bf16 [G][M][4] */
    void *d_values;             /* bf16 [G][M] */
    float *partial;             /* [G][chunks][4] */
} cat_ppo_loss;

/* One optimiser step on the flat [G][P] parameter buffers of a role:
 *   active_g  = epoch_active_g * (kl_g <= kl_threshold)           (kl_threshold <= 0: no gate); written back
 *   grad      = ar[g][0..P) * col_train;  clipped per agent to grad_norm_clip (torch.nn.utils.clip_grad_norm_)
 *   Adam (bias-corrected, per-entry step counts) on the entries with gate = active_g * col_train = 1
 *   lp        = bf16(master)                                       (when lp != NULL)
 * ar is [G][P + 1]: column P carries the agent's KL statistic (copied to kl_out). */
typedef struct cat_ppo_adam {
    int32_t G, P, chunks, pad;
    const float *ar;            /* [G][P + 1] */
    const float *col_train;     /* [G][P] */
    float *epoch_active;        /* [G] */
    float *m, *v, *steps;       /* [G][P] */
    float *master;              /* [G][P] */
    void *lp;                   /* bf16 [G][P] or NULL */
    float *kl_out;              /* [G] */
    float *norm_partial;        /* [G][chunks] scratch */
    float lr, beta1, beta2, eps, grad_norm_clip, kl_threshold;
} cat_ppo_adam;

/* Generalised advantage estimation over a stored rollout (skrl's compute_gae, reverse scan over the T ticks; one thread per
 * (agent, env) column):  delta_t = r_t + gamma * V_{t+1} * (1 - done_t) - V_t,  A_t = delta_t + gamma * lambda * (1 - done_t) * A_{t+1},
 * V_T = last_values, A_T = 0;  adv = A, ret = A + V.  The advantage normalisation stays with the caller. */
typedef struct cat_ppo_gae {
    int32_t G, T, N, pad;
    const float *rewards, *values;      /* [G][T][N] */
    const uint8_t *dones;               /* [T][N]: 1 = the episode ended with tick t (no bootstrap across it) */
    const float *last_values;           /* [G][N] */
    float gamma, lambda;
    float *adv, *ret;                   /* [G][T][N] */
} cat_ppo_gae;
int cat_ppo_gae_scan(const cat_ppo_gae *a, void *stream);

/* The same scan over a critic that is trained on NORMALISED returns (running value normalisation, below): every value the scan
 * reads -- values[g][t][n] and last_values[g][n] -- is denormalised first, V = v * sigma_g + mu_g with scale[g] = (mu_g, sigma_g):
 * one fp32 multiply, then one fp32 add, each rounded (never a fused multiply-add).  adv is the advantage, ret = adv + V the RAW
 * return.  Everything else is cat_ppo_gae_scan's arithmetic, instruction for instruction (one kernel template): the result is
 * bit-equal to cat_ppo_gae_scan run on values and last_values denormalised by those two operations beforehand, and with
 * scale = (0, 1) to cat_ppo_gae_scan itself.  Same grid, no atomics, capturable. */
typedef struct cat_ppo_gae_scaled {
    int32_t G, T, N, pad;
    const float *rewards, *values;      /* [G][T][N] */
    const uint8_t *dones;               /* [T][N] */
    const float *last_values;           /* [G][N] */
    float gamma, lambda;
    float *adv, *ret;                   /* [G][T][N] */
    const float *scale;                 /* [G][2] = (mu_g, sigma_g); device memory, not NULL */
} cat_ppo_gae_scaled;
int cat_ppo_gae_scan_scaled(const cat_ppo_gae_scaled *a, void *stream);

/* Running moments (n, mean, M2 = sum of squared deviations from the mean) of each agent's M samples, in f64 and in ONE fixed
 * order, so that the result is bit-reproducible and a host restatement of the order below reproduces it bit for bit.  Two
 * launches, no atomics, capturable.  All arithmetic is f64 with every operation rounded on its own (no contraction of a product
 * into a sum); divide and square root are the correctly rounded ones.
 *
 * Chunk launch: one workgroup of 256 threads per (g, chunk c); chunk c covers x[g][c * 4096 .. c * 4096 + 4095].
 *   1. thread i: s_i = 0; for j = 0 .. 15 in this order: e = c * 4096 + i + 256 j; if e < M: s_i = s_i + (double)x[g][e]
 *   2. halving tree in LDS: for stride = 128, 64, .., 1: s_i = s_i + s_{i + stride} for every i < stride; sum = s_0
 *   3. n_c = the number of e < M in the chunk (as a double); mean_c = sum / n_c
 *   4. steps 1 and 2 again over d * d, d = (double)x[g][e] - mean_c (the product rounded, then added); M2_c = that sum
 *   5. partial[g][c] = (n_c, mean_c, M2_c)
 * Merge launch: one workgroup per g.
 *   1. t[0 .. P) = partial[g][0 .. chunks) followed by (0, 0, 0) up to P, the next power of two >= chunks;
 *      for stride = P / 2, .., 1: t[i] = merge(t[i], t[i + stride]) for every i < stride; batch = t[0].
 *      (This tree runs in place in partial[g]: after the call partial holds intermediate values.)
 *   2. merge(a, b) = a if b.n == 0; b if a.n == 0; otherwise (Chan et al.), in this order of operations:
 *        n     = a.n + b.n
 *        delta = b.mean - a.mean
 *        mean  = a.mean + delta * (b.n / n)
 *        M2    = (a.M2 + b.M2) + (delta * delta) * (a.n * (b.n / n))
 *   3. batch_out[g] = batch                                 (when batch_out != NULL)
 *   4. state[g] = merge(state[g], batch)                    (when state != NULL)
 *   5. scale_out[g] = (mu, sigma) = ((float)state.mean, (float)sqrt(state.M2 / state.n)), or (0, 1) while state.n == 0
 *                                                           (when scale_out != NULL; needs state)
 * 1 <= M and cat_ppo_moment_chunks(M) <= 65536; a larger M is CAT_PPO_ERR_BAD_ARG. */
#define CAT_PPO_MOMENT_CHUNK 4096
typedef struct cat_ppo_moments_args {
    int32_t G, M;
    const float *x;                     /* [G][M], contiguous */
    double *partial;                    /* [G][chunks][3] scratch, chunks = cat_ppo_moment_chunks(M); caller-owned */
    double *batch_out;                  /* [G][3] = (n, mean, M2) of this call's samples, or NULL */
    double *state;                      /* [G][3], merged in place, or NULL */
    float *scale_out;                   /* [G][2] = (mu, sigma) of the merged state, or NULL; needs state */
} cat_ppo_moments_args;
int cat_ppo_moment_chunks(int32_t M);   /* ceil(M / CAT_PPO_MOMENT_CHUNK); 0 for M <= 0 */
int cat_ppo_moments(const cat_ppo_moments_args *a, void *stream);

int cat_ppo_abi_version(void);
const char *cat_ppo_last_error(void);
int cat_ppo_loss_grad(const cat_ppo_loss *a, void *stream);
int cat_ppo_adam_step(const cat_ppo_adam *a, void *stream);

/* ---- Hyper-parameters in device memory (entries added to version 2; nothing above changes).
 * The two entries above take the learning rate, the entropy scale and the ratio clip BY VALUE: a captured graph bakes them in.  The
 * _dev entries below read them from a per-agent block in device memory instead, so a replay sees what the block holds at that time:
 *   float hyper[G][CAT_PPO_HYPER_STRIDE]
 * Columns 5..7 are reserved: the caller writes 0, no kernel touches them. */
#define CAT_PPO_HYPER_STRIDE 8
enum {
    CAT_PPO_HYPER_LR = 0,               /* learning rate */
    CAT_PPO_HYPER_ENTROPY = 1,          /* entropy scale */
    CAT_PPO_HYPER_RATIO_CLIP = 2,       /* ratio clip */
    CAT_PPO_HYPER_KL_SUM = 3,           /* sum of the minibatch KLs of the current epoch */
    CAT_PPO_HYPER_KL_COUNT = 4          /* number of minibatches in that sum */
};

/* cat_ppo_loss with ``hyper``: agent g takes ratio_clip = hyper[g][RATIO_CLIP] and entropy_scale = hyper[g][ENTROPY]; the two by-value
 * fields are ignored, value_scale stays by value.  One kernel template with cat_ppo_loss_grad: with the block holding the by-value
 * numbers the result is bit-equal to it. */
typedef struct cat_ppo_loss_dev {
    int32_t G, M, chunks, pad;
    const void *logits;
    const void *values;
    const int64_t *actions;
    const float *old_logp, *adv, *ret;
    float ratio_clip, value_scale, entropy_scale, pad2;
    void *d_logits;
    void *d_values;
    float *partial;
    const float *hyper;         /* [G][CAT_PPO_HYPER_STRIDE]; device memory, not NULL */
} cat_ppo_loss_dev;
int cat_ppo_loss_grad_dev(const cat_ppo_loss_dev *a, void *stream);

/* cat_ppo_adam with ``hyper``: agent g's learning rate is hyper[g][LR]; the ``lr`` field is ignored.  The same two kernel templates as
 * cat_ppo_adam_step, bit-equal to it when hyper[g][LR] = lr.  In addition the one thread that rewrites epoch_active[g] reads
 * was = epoch_active[g] before that store and, when was != 0, does (plain fp32 adds)
 *   hyper[g][KL_SUM] += kl_g;   hyper[g][KL_COUNT] += 1
 * so the minibatch that trips the KL early stop still counts and the gated ones after it do not (skrl appends the KL, then breaks). */
typedef struct cat_ppo_adam_dev {
    int32_t G, P, chunks, pad;
    const float *ar;
    const float *col_train;
    float *epoch_active;
    float *m, *v, *steps;
    float *master;
    void *lp;
    float *kl_out;
    float *norm_partial;
    float lr, beta1, beta2, eps, grad_norm_clip, kl_threshold;
    float *hyper;               /* [G][CAT_PPO_HYPER_STRIDE]; device memory, not NULL */
} cat_ppo_adam_dev;
int cat_ppo_adam_step_dev(const cat_ppo_adam_dev *a, void *stream);

/* The schedule rule on the block: one workgroup, thread g = agent g (G <= CAT_ROLLOUT_MAX_AGENTS = 8), no atomics, capturable.  Every
 * operation below is ONE rounded fp32 operation (no contraction of a product into a sum; the divides are the correctly rounded ones).
 * ``mode`` is a set of the two bits; with both the anneal runs first.
 *
 * CAT_PPO_SCHED_ANNEAL (start of an update), for every agent and each field chosen by ``anneal_mask``
 * (CAT_PPO_ANNEAL_LR: lr0, lr1 -> LR; CAT_PPO_ANNEAL_ENTROPY: ent0, ent1 -> ENTROPY; CAT_PPO_ANNEAL_RATIO_CLIP: clip0, clip1 -> RATIO_CLIP):
 *   d = x1 - x0;  p = d * progress;  x = x0 + p                    (0 <= progress <= 1)
 *
 * CAT_PPO_SCHED_KL (end of an epoch; skrl's KLAdaptiveLR [SKRL-RECALL], per agent):
 *   hi = kl_target * kl_factor;  lo = kl_target / kl_factor
 *   if (hyper[g][KL_COUNT] > 0 && sched_active[g] != 0) {
 *       kl = hyper[g][KL_SUM] / hyper[g][KL_COUNT];  lr = hyper[g][LR]
 *       if      (kl > hi) lr = fmaxf(lr / lr_factor, lr_min)
 *       else if (kl < lo) lr = fminf(lr * lr_factor, lr_max)
 *       hyper[g][LR] = lr
 *   }
 *   hyper[g][KL_SUM] = hyper[g][KL_COUNT] = 0                      (always)
 * sched_active[g] = 1 iff agent g's policy is being trained: a frozen policy has KL exactly 0, and without the gate its learning rate
 * would climb to lr_max under the critic that still trains.
 * CAT_PPO_ERR_BAD_ARG, whatever the mode: NULL hyper or sched_active, G outside 1..8, mode outside 1..3, progress outside [0, 1],
 * lr_factor < 1, kl_factor < 1, lr_min > lr_max (a NaN fails each of these too). */
enum { CAT_PPO_SCHED_KL = 1, CAT_PPO_SCHED_ANNEAL = 2 };
enum { CAT_PPO_ANNEAL_LR = 1, CAT_PPO_ANNEAL_ENTROPY = 2, CAT_PPO_ANNEAL_RATIO_CLIP = 4 };
typedef struct cat_ppo_schedule {
    int32_t G, mode, anneal_mask, pad;
    float *hyper;                       /* [G][CAT_PPO_HYPER_STRIDE] */
    const float *sched_active;          /* [G] */
    float kl_target, kl_factor, lr_factor, lr_min, lr_max;
    float progress;
    float lr0, lr1, ent0, ent1, clip0, clip1;
} cat_ppo_schedule;
int cat_ppo_schedule_step(const cat_ppo_schedule *a, void *stream);

#ifdef __cplusplus
}
#endif
#endif
