/*
 * cat_act.h -- C ABI of libcat_learn.so, part 8: the act tick of the stacked recurrent policies in ONE launch.
 *
 * cat_act_step evaluates, for G stacked models.LSTMPolicy networks over N envs, the whole chain
 *   observation (2R) -> Conv1d(2, 64, 5, stride 2) + ReLU -> Conv1d(64, 32, 5, stride 3) + ReLU -> Linear(32 L2, 256) + tanh
 *   -> LSTM(256, 128) cell -> Linear(128, 128) + ReLU -> Linear(128, 64) + ReLU -> Linear(64, 4) -> action
 * straight from the env core's observation buffers (the conversion and scaling of cat_rollout_pack happen inside), updates
 * the recurrent state in place and writes the actions into the env's [N][A] action matrix.  Nothing else goes to memory.
 *
 * Arithmetic contract
 *  - every product runs on the matrix cores with bf16 operands and fp32 accumulation; biases are added in fp32;
 *  - the outputs of the two convolutions, of the 256-wide layer, of the two hidden head layers and the new h are ROUNDED TO
 *    BF16 before the next product reads them (the rounding points of the per-layer kernel chain); the LSTM gate
 *    pre-activations are NOT rounded: W_ih x + W_hh h stays in the fp32 accumulator, both LSTM biases are added to it in fp32;
 *  - the cell is fp32, gate order i, f, g, o (nn.LSTM): c' = sigmoid(f) c + sigmoid(i) tanh(g), h' = sigmoid(o) tanh(c') with
 *    the unrounded c'; h' and c' are stored rounded to bf16;
 *  - the logits are rounded once to bf16; everything after reads those bf16 values;
 *  - mode 0 (sampled) is cat_rollout_sample's rule on the bf16 logits z: masses e_j = __expf(z_j - zmax), sum = e_0 + e_1 +
 *    e_2 + e_3 in that order, u = uniform * sum, action = (u >= e_0) + (u >= e_0 + e_1) + (u >= e_0 + e_1 + e_2), and the
 *    log-probability is z[action] - zmax - __logf(sum);
 *  - mode 1 (greedy) is the largest bf16 logit, the lowest index on ties; its log-probability is the same expression;
 *  - for an agent g whose bit is set in random_mask the action is min(3, (int)(4 * uniform)); no network is evaluated, h / c
 *    and that agent's rows of logits_out / logp_out are left untouched;
 *  - keep[n] == 0 takes h and c of env n as zero before this tick (an episode starts there); keep NULL carries every state.
 *
 * Conventions as in cat_rollout.h: int status, caller-owned device buffers, an explicit stream, no allocation and no
 * synchronisation (the entry can be captured in a HIP graph), arguments by value in one struct.  A workgroup owns its rows of
 * h / c (it reads them before it writes them), rows n >= N are never read or written, and there are no atomics: equal inputs
 * give bit-equal outputs.
 */
#ifndef CAT_ACT_H
#define CAT_ACT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CAT_ACT_ABI_VERSION 1
#define CAT_ACT_MAX_AGENTS 8
#define CAT_ACT_HIDDEN 128
#define CAT_ACT_MAX_SEGMENTS 32

enum { CAT_ACT_OK = 0, CAT_ACT_ERR_BAD_ARG = -1, CAT_ACT_ERR_HIP = -2 };
enum { CAT_ACT_SAMPLE = 0, CAT_ACT_GREEDY = 1 };

typedef struct cat_act_dims {
    int32_t G, N, A, R;                         /* stacked policies (<= 8), envs, agents in the env, rays (64 or 90) */
} cat_act_dims;

/* The parameters of the G stacked LSTMPolicy networks in their own layouts (models.LSTMPolicy.state_dict()), bf16, network g at
   pointer + g * stride (elements).  Every pointer 16-byte aligned, stride a multiple of 8. */
typedef struct cat_act_params {
    const void *conv1_w, *conv1_b;              /* [64][2][5], [64] */
    const void *conv2_w, *conv2_b;              /* [32][64][5], [32] */
    const void *fc_w, *fc_b;                    /* [256][32 * L2] columns in (channel, position) order, [256] */
    const void *w_ih, *w_hh, *b_ih, *b_hh;      /* [512][256], [512][128], [512], [512] */
    const void *head0_w, *head0_b;              /* [128][128], [128] */
    const void *head1_w, *head1_b;              /* [64][128], [64] */
    const void *head2_w, *head2_b;              /* [4][64], [4] */
    int64_t stride;
} cat_act_params;

typedef struct cat_act_args {
    cat_act_dims d;
    int32_t agent[CAT_ACT_MAX_AGENTS];          /* env agent index of policy g: its observation rows and its action column */
    int32_t mode;                               /* CAT_ACT_SAMPLE / CAT_ACT_GREEDY */
    uint32_t random_mask;                       /* bit g: policy g acts uniformly at random */
    int32_t row_tile;                           /* rows of one network per workgroup: 32 or 64; 0 = the library's choice */
    float distance_scale, type_scale;
    int32_t pad;
    const void *obs_distance;                   /* f16 [N][A][R] (cat_outputs.obs_distance) */
    const void *obs_type;                       /* u8  [N][A][R] */
    cat_act_params p;
    void *h, *c;                                /* bf16 [G][N][128], updated in place */
    const float *keep;                          /* [N] or NULL */
    const float *uniform;                       /* [G][N] in [0, 1) */
    int32_t *actions;                           /* [N][A]: column agent[g] receives policy g's action */
    void *logits_out;                           /* bf16 [G][N][4] or NULL */
    float *logp_out;                            /* [G][N] or NULL */
} cat_act_args;

/* The collect form: cat_act_step for a policy the trainer LEARNS.  Next to everything cat_act_step does with ``base`` (base.actions,
   base.h / base.c in place, base.logits_out / base.logp_out where non-NULL: bit for bit what cat_act_step produces from the same
   inputs), the one launch writes what a rollout keeps of the tick, in the rollout's own strided buffers:
    - policy_in[g][n] (bf16 [2R]) and value_in[g][n] (bf16 [4R]): the rows cat_rollout_pack writes for the same agents, scales, n_cops
      and first_agent_state (n_cops, first_agent_state, shared_distance, shared_type: the meanings of cat_rollout_pack_args).  The policy
      row is the observation image the networks read; the workgroup that owns rows of network g writes g's value rows;
    - act_out[g * sa_g + n]: the action as int64; logp_out[g * sl_g + n]: the fp32 log-probability cat_act_step writes to base.logp_out;
    - h0_out / c0_out (bf16 [G][N][128] contiguous, both or neither): h and c as they stood in memory BEFORE the tick -- keep is not
      applied to them -- what a learner keeps as the state at the start of a BPTT window.  They must not overlap base.h / base.c.
   Row (g, n) of policy_in lies at element g * sp_g + n * sp_n, of value_in at g * sv_g + n * sv_n.  Alignment: rows are stored 8 bytes
   at a time ([G, T, N, 2R] with R = 90 aligns its rows to 8 bytes and no more), so policy_in and value_in are 8-byte aligned and sp_g, sp_n,
   sv_g, sv_n are multiples of 4 elements with sp_n >= 2R, sv_n >= 4R; h0_out / c0_out are 16-byte aligned; act_out and logp_out have
   their types' alignment.  base.random_mask must be 0.  Rows n >= N are never read or written, bytes outside the addressed rows of a
   strided buffer are untouched, there are no atomics, equal inputs give bit-equal outputs, and the launch is graph-capturable (no
   allocation, no synchronisation).  The entry uses the LDS of cat_act_step and reads the weights once, as cat_act_step. */
typedef struct cat_act_collect_args {
    cat_act_args base;
    int32_t n_cops;                             /* agents [0, n_cops) are team 0 */
    int32_t first_agent_state;                  /* 1: every critic row is built from env agent 0 */
    const void *shared_distance;                /* f16 [N][2][R] */
    const void *shared_type;                    /* u8  [N][2][R] */
    void *policy_in;                            /* bf16 rows [2R] */
    int64_t sp_g, sp_n;
    void *value_in;                             /* bf16 rows [4R] */
    int64_t sv_g, sv_n;
    int64_t *act_out;                           /* [G][N], row stride sa_g */
    int64_t sa_g;
    float *logp_out;                            /* [G][N], row stride sl_g */
    int64_t sl_g;
    void *h0_out, *c0_out;                      /* bf16 [G][N][128], or both NULL */
} cat_act_collect_args;

/* The league form: the N rows are cut into S contiguous segments and every segment names, per policy, the parameter set of a
   BANK that plays there.  base.p addresses the bank: set k of every block at pointer + k * stride.  Policy g in segment s (rows
   seg_start[s] .. seg_start[s + 1] - 1; seg_start[0] == 0, seg_start[S] == N, strictly increasing) reads set seg_set[g][s] in
   [0, sets); -1: policy g acts uniformly at random there (the random_mask rule: action min(3, (int)(4 * uniform)), its rows of
   h / c / logits_out / logp_out untouched).  base.random_mask must be 0; everything else in base keeps its meaning.  A workgroup's
   rows all lie in one segment, and a row's outputs depend on that row's inputs and its parameter set alone: neither on the tile
   it falls into nor on the segment table around it. */
typedef struct cat_act_league_args {
    cat_act_args base;
    int32_t S;                                  /* segments, 1 .. CAT_ACT_MAX_SEGMENTS */
    int32_t sets;                               /* parameter sets in the bank, >= 1 */
    int32_t seg_start[CAT_ACT_MAX_SEGMENTS + 1];
    int32_t seg_set[CAT_ACT_MAX_AGENTS][CAT_ACT_MAX_SEGMENTS];
} cat_act_league_args;

int cat_act_abi_version(void);
const char *cat_act_last_error(void);
int cat_act_supported(const cat_act_dims *d);   /* 1: cat_act_step takes these dimensions */
int cat_act_step(const cat_act_args *a, void *stream);
int cat_act_collect_step(const cat_act_collect_args *a, void *stream);
int cat_act_league_step(const cat_act_league_args *a, void *stream);

#ifdef __cplusplus
}
#endif
#endif
