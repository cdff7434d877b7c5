/*
 * cat_sim.h -- C ABI of libcat_sim.so, the MI355X (gfx950) batched Cops-and-Thieves env core.
 *
 * The reference has no FFI: its hot path sits behind the PettingZoo ParallelEnv Python API
 * (SURVEY.md section 8b).  This ABI is what a binding for that path binds instead of Pymunk;
 * each entry point names the reference interface it replaces (paths relative to
 * /root/reference).  Conventions: opaque handle, int status (0 ok, <0 error; message from
 * cat_last_error), no exceptions across the boundary, CALLER-OWNED DEVICE buffers, explicit
 * hipStream_t passed as void* (NULL = default stream), one host thread per handle, handles are
 * independent (one per GPU / per process).  There is no CPU fallback: every compute entry fails
 * with CAT_ERR_NO_DEVICE when no HIP device is usable.
 */
#ifndef CAT_SIM_H
#define CAT_SIM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CAT_ABI_VERSION 1
#define CAT_MAX_AGENTS 8
#define CAT_MAX_RAYS 512
#define CAT_MAX_SHAPES 256
#define CAT_MAX_HULL_EDGES 31   /* edges of one convex wall */
#define CAT_MAX_ROLLOUT_TICKS 65536   /* ticks of one cat_rollout_fused launch */
#define CAT_WALL_CACHE 8        /* cached wall arbiters per agent; cat_create refuses a map on which an agent could need more */

enum {
    CAT_OK = 0,
    CAT_ERR_BAD_CONFIG = -1,
    CAT_ERR_BAD_MAP = -2,
    CAT_ERR_BAD_SLOT_MAP = -3,
    CAT_ERR_NO_DEVICE = -4,
    CAT_ERR_HIP = -5,
    CAT_ERR_BAD_ARG = -6
};

/* ObjectType -- src/utils/object_types.py:4-9 */
enum { CAT_WALL = 0, CAT_COP = 1, CAT_THIEF = 2, CAT_MOVABLE = 3, CAT_EMPTY = 4 };

/* Replaces the constructor arguments of SimpleEnv/BaseEnv (src/environments/simple_env.py:14-38,
   base_env.py:51-58), the constants of pyproject.toml:12-19, the sensor literals of
   src/agents/entity.py:84-86,196 and Chipmunk2D's cpSpace defaults (base_env.py:77). */
typedef struct cat_config {
    int32_t n_envs;
    int32_t n_cops;
    int32_t n_thieves;
    int32_t n_rays;
    int32_t max_step_count;
    int32_t iterations;
    int32_t persistence;
    int32_t bbtree_gate;          /* CAT_GATE_*: visiting rule of segment queries (see below) */
    int64_t env_id_offset;        /* global id of env slot 0 (env sharding across GPUs) */
    uint64_t seed;                /* Philox4x32-10 key */
    double dt;
    double bias_coef;             /* 1 - pow(collisionBias, dt), computed by the host */
    double slop;
    double ray_length;
    double ray_radius;
    double agent_radius;
    double agent_mass;
    double impulse;
    double max_speed;
    double termination_radius;
    double wall_radius;
} cat_config;

/* cat_config.bbtree_gate.  Which walls and agents a segment query (ray or line of sight) visits, and in which order:
   CAT_GATE_NONE  every shape, in index order (no spatial-index gate);
   CAT_GATE_INDEX Chipmunk's gate -- a shape is visited iff the thin segment enters its bounding box before the best alpha so far --
                  with the walls visited in index order (the default);
   CAT_GATE_TREE  the same gate with the walls visited in the depth-first order of Chipmunk's static BBTree ([CP SubtreeSegmentQuery],
                  nearer child first, the tree cpBBTreeInsert builds from the walls in index order); the agents follow in index order.
                  Runs the chunk form of the ray fan only; cat_create refuses a map whose tree is deeper than 48 (CAT_ERR_BAD_MAP).
   Other values: CAT_ERR_BAD_CONFIG. */
#define CAT_GATE_NONE 0
#define CAT_GATE_INDEX 1
#define CAT_GATE_TREE 2

/* HOST pointers, copied at create.  ray_dx/dy[k] = ray_length * cos/sin(2*pi*k/R) built with
   NumPy as entity.py:182-193 builds them; reward LUTs indexed by float16 bits (cop.py:69-74,
   thief.py:63-69 evaluated by NumPy per float16 value). */
typedef struct cat_tables {
    const double *ray_dx;         /* [R] */
    const double *ray_dy;         /* [R] */
    const float *cop_reward_lut;  /* [32768] */
    const float *thief_reward_lut;/* [32768] */
} cat_tables;

/* DEVICE pointers; any may be NULL (that output is skipped). */
typedef struct cat_outputs {
    uint16_t *obs_distance;       /* [N,A,R] float16 bits -- Entity.get_observation "distance" */
    uint8_t *obs_type;            /* [N,A,R]              -- "object_type" */
    int32_t *hit_shape;           /* [N,A,R] -1 none, s wall, S+j agent j (parity/debug) */
    uint16_t *shared_distance;    /* [N,2,R] team 0 cops / 1 thieves -- distance_shared */
    uint8_t *shared_type;         /* [N,2,R]                          -- object_type_shared */
    uint16_t *team_positions;     /* [N,A,2] float16 bits             -- team_positions */
    float *reward;                /* [N,A] */
    uint8_t *terminated;          /* [N] capture or timeout (entity.py:146) */
    uint8_t *truncated;           /* [N] timeout only (base_env.py:397) */
    int8_t *winner;               /* [N] -1 none, 0 cop, 1 thief (base_env.py:399-406) */
} cat_outputs;

/* DEVICE pointers for state get/set (env checkpointing, parity tests); any may be NULL. */
typedef struct cat_state {
    double *pos;                  /* [N,A,2] body.position */
    double *vel;                  /* [N,A,2] body.velocity */
    double *vbias;                /* [N,A,2] Chipmunk v_bias */
    double *tc;                   /* [N,A,2] cached circle centre (stale after reset) */
    double *leaf_bb;              /* [N,A,4] BBTree leaf bb */
    int32_t *wall_shape;          /* [N,A,CAT_WALL_CACHE] */
    int32_t *wall_age;            /* [N,A,CAT_WALL_CACHE] */
    double *wall_jn;              /* [N,A,CAT_WALL_CACHE] */
    int32_t *pair_age;            /* [N,A(A-1)/2] */
    double *pair_jn;              /* [N,A(A-1)/2] */
    int32_t *step_count;          /* [N] */
    int32_t *reset_count;         /* [N] */
} cat_state;

typedef struct cat_sim cat_sim;

/* Replaces BaseEnv.__init__ (base_env.py:51-121): pymunk.Space(), Map.populate_space
   (src/maps/map.py:119-128, via compiled map blobs), _init_cops/_init_thieves (:168-214) and
   Entity.__init__ (entity.py:41-124).  map_blobs are HOST pointers to blobs produced by
   as_cops_and_thieves_amd.maps.CompiledMap.to_blob(); slot_map_ids[N] (HOST, NULL = all 0)
   selects the map of each env slot.  device = HIP device ordinal. */
int cat_create(const cat_config *cfg, const cat_tables *tables, const void *const *map_blobs,
               const size_t *blob_sizes, int n_maps, const int32_t *slot_map_ids, int device,
               cat_sim **out);
int cat_destroy(cat_sim *sim);
/* sim may be NULL: message of the last failed cat_create on this thread's library. */
const char *cat_last_error(const cat_sim *sim);

/* Replaces BaseEnv.reset (base_env.py:286-352) incl. _get_non_colliding_position (:123-166),
   Entity.reset (entity.py:148-157) and Space.point_query_nearest (call site :154).  mask
   (DEVICE, [N] u8, NULL = all) selects envs; positions (DEVICE, [N,A,2] f64, NULL = Philox
   spawn sampling) injects spawn positions.  Writes the post-reset observations. */
int cat_reset(cat_sim *sim, const uint8_t *mask, const double *positions, const cat_outputs *out,
              void *stream);
/* Same, with mask = "terminated flag set by the previous cat_step" (kept on device, no host
   sync): the auto-reset of the batched env. */
int cat_reset_done(cat_sim *sim, const cat_outputs *out, void *stream);

/* Replaces BaseEnv.step (base_env.py:354-413): _termination_criterion (:521-554),
   Entity.step/_perform_action/get_observation/_query_body (entity.py:126-241), Cop.reward /
   Thief.reward (cop.py:49-75, thief.py:48-69), get_shared_observations
   (src/environments/observation_spaces.py:67-131) and pymunk Space.step (call site :392).
   actions: DEVICE [N,A] int32 in {0,1,2,3}.  The launch is asynchronous, so an action outside 0..3 (the reference
   raises on it: entity.py:126-134 indexes its impulse table) cannot fail the call: it is applied as "no impulse" and
   raises CAT_DEVERR_BAD_ACTION in the handle's device-side error word -- read it with cat_device_errors. */
int cat_step(cat_sim *sim, const int32_t *actions, const cat_outputs *out, void *stream);

/* Device-side error flags raised by the kernels since the last clear (synchronises `stream`); flags != 0 also sets
   cat_last_error.  CAT_DEVERR_CONTACT_DROPPED: an agent touched more than CAT_WALL_CACHE walls in one step, or an env had
   more simultaneous contacts than cat_create proved possible for its maps (agents x the deepest overlap of wall bounding
   boxes one agent can reach, + agent pairs), and a contact got no constraint (Chipmunk's arbiter hash has no such limit).
   The asynchronous entries cannot fail on these: a caller reads the word where it needs the results to be valid (the
   reference raises at once: entity.py:126-134). */
#define CAT_DEVERR_BAD_ACTION 1u
#define CAT_DEVERR_CONTACT_DROPPED 2u
#define CAT_DEVERR_SCHEDULER 4u   /* internal: a work item of the pooled ray fan never arrived (the launch left instead of hanging); results of that launch are invalid */
int cat_device_errors(cat_sim *sim, uint32_t *flags, int clear, void *stream);

/* One-LAUNCH form of the rollout tick: cat_step, the auto-reset of cat_reset_done (auto_reset != 0) and,
   when actions == NULL, the synthetic Philox actions of cat_random_actions for tick `synth_tick`, all inside
   the step kernel.  Results are identical to the three separate calls: for an episode that ends with this
   tick, reward / terminated / truncated / winner are the terminal tick's and the observation buffers hold
   the first observations of the new episode (the terminal observations, which the separate calls compute
   and then overwrite, are not computed). */
int cat_step_fused(cat_sim *sim, const int32_t *actions, uint64_t synth_tick, int auto_reset,
                   const cat_outputs *out, void *stream);

/* RESIDENT ROLLOUT: T consecutive ticks of cat_step_fused in ONE launch -- the random-action phases of the reference's loops
   (src/driver.py:65-69 steps the env with sampled actions tick after tick; skrl's trainer does so for random_timesteps = 10000
   ticks, src/configs/mappo_config.py:9) and, with an action tape, any replay of fixed actions.  The map geometry is staged into
   LDS once, every env slot's state record stays in LDS for the T ticks and reaches HBM after the last one, and EVERY tick's
   outputs are written: each non-NULL pointer of `out` addresses a buffer with a leading T -- obs_distance [T,N,A,R], reward
   [T,N,A], terminated [T,N] ... -- whose row t holds exactly what cat_step_fused(actions_t, synth_tick0 + t, auto_reset)
   leaves in its [N,...] buffers after tick t.  actions: DEVICE [T,N,A] int32, or NULL = the synthetic Philox actions of
   cat_random_actions for ticks synth_tick0 .. synth_tick0 + T - 1.  1 <= T <= CAT_MAX_ROLLOUT_TICKS.  Bit-identical to T calls
   of cat_step_fused (outputs of every tick and the state afterwards). */
int cat_rollout_fused(cat_sim *sim, int T, const int32_t *actions, uint64_t synth_tick0, int auto_reset,
                      const cat_outputs *out, void *stream);

/* FRAME SKIP (action repeat): ONE decision of up to k ticks per env slot in ONE resident launch (the sim's rollout kernel, T = k).
   For every env slot independently, 1 <= k <= CAT_MAX_ROLLOUT_TICKS:
   1. The slot plays ticks j = 0, 1, ... with the SAME row of actions (DEVICE [N,A] int32, not NULL: synthetic actions are not offered
      here).  Each tick is exactly a cat_step_fused(actions, ., auto_reset) tick of that slot; an action outside 0..3 raises
      CAT_DEVERR_BAD_ACTION as it does there.
   2. Hold rule: the slot stops after the first tick j* at which `terminated` is set, or after tick k - 1 if none is; the rule is checked
      after every tick, the first included.  With auto_reset the auto-reset of tick j* happens inside that tick as in cat_step_fused and
      the slot then does not advance: the new episode has its first observation and step_count 0, and is never stepped with the stale
      action.  Without auto_reset the slot is left as cat_step_fused(..., 0) leaves it after j*.
   3. Outputs: `out` addresses [N,...] buffers, the one-tick layout.  Observations, shared observations, team positions and hit_shape are
      those of the slot's LAST played tick, and so are terminated / truncated / winner (the only tick that can carry them).  reward[n][a] is
      the fp32 left fold ((r_0 + r_1) + r_2) + ... over the played ticks in tick order: plain fp32 adds, no fused multiply-add, no
      discounting.  ticks (DEVICE [N] int32, or NULL): the number of ticks played, 1 .. k.  Ticks before the last store nothing.
   4. The state afterwards is, in every field of cat_state, bit-identical to playing those ticks one launch at a time.
   5. k == 1 is bit-identical to cat_step_fused in every output and in the state.
   6. Asynchronous; no allocation and no synchronisation (capturable in a HIP graph); k out of range and actions == NULL are rejected with
      CAT_ERR_BAD_ARG and a message (cat_last_error) before any device call.
   No reference counterpart (the reference steps one tick per call). */
int cat_step_repeat(cat_sim *sim, int k, const int32_t *actions, int auto_reset,
                    const cat_outputs *out, int32_t *ticks, void *stream);

/* END-OF-EPISODE POSITIONS.  An entry added after ABI version 1 was fixed (cat_outputs and CAT_ABI_VERSION are unchanged: the handle keeps the pointer).
   Under auto-reset a slot that ends an episode is stepped, respawned and traced for its new episode inside the same tick, so the terminal row's
   team_positions already holds the spawn point of the NEXT episode.  While a buffer is bound, every stepping entry -- cat_step, cat_step_fused,
   cat_rollout_fused, cat_step_repeat, auto_reset 0 or 1 -- writes, for every slot-row whose `terminated` flag that tick sets, the float16 bits
   (as team_positions) of the 2A tick-start body positions: the ones the termination check read (base_env.py:521-554) and team_positions would have
   carried without the reset (observation_spaces.py:92-95).  The buffer is addressed exactly like team_positions of the same call: [N,A,2] for the
   one-tick entries and for cat_step_repeat (the window's last played tick: the only one that can be terminal), [T,N,A,2] for cat_rollout_fused (row
   t*N + env), and must be that large.  Rows that are not terminal are NOT TOUCHED: the caller pre-fills them (a NaN pattern such as 0x7E00), and the
   common path gains no store.  cat_reset / cat_reset_done write nothing.  With auto_reset == 0 a terminal row equals team_positions of the same call.
   No allocation, no synchronisation, no device call (capturable); takes effect from the next launch.  The pointer travels in the launch arguments, so
   a HIP graph captured with a buffer bound keeps writing to THAT buffer: rebinding or detaching needs a recapture.
   No reference counterpart (the reference resets in a separate call: its positions at the end of an episode are simply still there). */
int cat_bind_final_positions(cat_sim *sim, uint16_t *buf);   /* DEVICE, or NULL = detach (the default) */

/* Env-state access (the reference cannot checkpoint env state). D2D copies. */
int cat_get_state(cat_sim *sim, const cat_state *dst, void *stream);
int cat_set_state(cat_sim *sim, const cat_state *src, void *stream);

/* Synthetic uniform actions (driver.py:68 samples action_space(agent) per agent):
   Philox(key = seed, counter = (env_global, tick, agent, 0xAC710)) & 3 -> DEVICE [N,A] int32. */
int cat_random_actions(cat_sim *sim, uint64_t tick, int32_t *actions, void *stream);

/* gymnasium-style reseeding (BaseEnv.reset(seed=...), base_env.py:307-311): replaces the Philox key
   used by later spawn sampling / synthetic actions. */
int cat_set_seed(cat_sim *sim, uint64_t seed, void *stream);

/* Measurement aid (bench.py's roofline leg): the NEXT cat_step / cat_step_fused launches its tick kernel with
 * this pair of hipEvent_t attached to the dispatch itself, so hipEventElapsedTime(start, stop) is the kernel's own
 * duration -- the figure rocprofv3 --kernel-trace reports -- without the inter-kernel dispatch gap that events
 * recorded around the call include.  One shot.  No reference counterpart (the reference has no timers on the path). */
int cat_arm_kernel_timing(cat_sim *sim, void *start_event, void *stop_event);

/* Introspection */
int cat_abi_version(void);
/* Names of the kernels cat_step / cat_step_fused and cat_rollout_fused launch ("step_kernel" / "rollout_kernel": one tick / T ticks through the resident
   scheduler; "step_kernel_pooled" / "rollout_kernel_pooled" where cat_create chose the pooled ray fan for that entry): what a profile lists.  No reference
   counterpart. */
const char *cat_one_tick_kernel(const cat_sim *sim);
const char *cat_rollout_kernel(const cat_sim *sim);
/* Chunk form of the ray fan (dense maps): how many 64-ray chunks of an env slot one work unit traces with one shared item list, in the resident launch
   (resident != 0) or the one-tick launch; 1 = chunk by chunk.  A sim of two parts: the chunk-form part's figure.  No reference counterpart. */
int cat_chunks_per_unit(const cat_sim *sim, int resident);
int cat_num_agents(const cat_sim *sim);
int cat_num_shapes(const cat_sim *sim, int map_index);
/* Timing hook for bench.py: seconds spent in the last n recorded step launches are measured by
   the caller with HIP events on `stream`; this returns the stream the handle would use for
   NULL (always the device's default stream). */

/* Test hook: the host copy of the spatial-hash broadphase tables built at cat_create.  k >= 0:
   candidate wall ids of ray k for an origin at (x, y); k < 0: contact candidates of that cell.
   Returns the list length and writes up to max_out ids. */
int cat_debug_grid_lookup(const cat_sim *sim, int map_index, double x, double y, int k, int *out, int max_out);

/* Host-only construction/lookup of one map's tables (no device): lets the CPU test-suite verify that
   the tables are supersets of the exact bb gate.  cell <= 0 selects the default cell size. */
typedef struct cat_grid_host cat_grid_host;
int cat_grid_build_host(const cat_config *cfg, const cat_tables *tables, const void *map_blob, size_t blob_size,
                        double cell, cat_grid_host **out);
int cat_grid_lookup_host(const cat_grid_host *grid, double x, double y, int k, int *out, int max_out);
long long cat_grid_bytes_host(const cat_grid_host *grid);
void cat_grid_free_host(cat_grid_host *grid);

/* The most wall bounding boxes the bb of one agent circle (radius agent_radius) can overlap at once on this map (host only): the
   bound cat_create holds against CAT_WALL_CACHE -- a map where it is larger is refused (CAT_ERR_BAD_MAP) instead of dropping a
   contact at run time (CAT_DEVERR_CONTACT_DROPPED stays as the backstop).  Negative: an error code. */
int cat_map_wall_bb_depth_host(const void *map_blob, size_t blob_size, double agent_radius);

/* Host-only: the static tree cat_create builds for a map in tree order (CAT_GATE_TREE), for the CPU tests.  Node n < S is the leaf of wall n,
   inner nodes follow in creation order.  Writes up to max_nodes nodes: bb_out[4n..4n+3] = l b r t, link_out[4n..4n+3] = child a, child b,
   parent (-1 at the root), wall id (leaf) or -1; *root, *depth (edges from the root to the deepest leaf).  Returns the node count 2S - 1,
   or an error code.  Any output pointer may be NULL. */
int cat_bbtree_host(const void *map_blob, size_t blob_size, double *bb_out, int *link_out, int max_nodes, int *root, int *depth);

/* Host-only: the text cat_create prints under CAT_VERBOSE for these arguments (every decision it takes and a hash of
   every table it would upload), without a device.  Lines of key=value; at most cap - 1 characters and a NUL are written
   to buf (which may be NULL).  Returns the length of the whole text, or a CAT_ERR_* with cat_last_error(NULL) set. */
int cat_plan_describe_host(const cat_config *cfg, const cat_tables *tables, const void *const *map_blobs, const size_t *blob_sizes,
                           int n_maps, const int32_t *slot_map_ids, char *buf, size_t cap);

/* Device arithmetic self-test used by tests: out[i] = op(in_a[i], in_b[i]) evaluated on the GPU
   with the same primitives the kernels use (op 0 sqrt(a), 1 a/b, 2 f64->f16 bits of a,
   3 obs-distance f16 bits of (a,b) relative to the origin (0,0); 4 and 5: a radius test on the squared distance a with the
   square root (bit 0 of the result) and by its threshold (bit 1) -- 4: sqrt(a) < b[0] | a < b[1]; 5: sqrt(a) - b[0] <= b[1] |
   a <= b[2]; in_b then holds those two or three values, not n).  DEVICE pointers. */
int cat_selftest_arith(int op, const double *in_a, const double *in_b, double *out, int n, int device,
                       void *stream);

/* Host-only: the thresholds by which the kernels run their two radius tests on SQUARED distances (csrc/cat_sim_radius.h):
   out2[0] = the double X with sqrt(x) < term_radius <=> x < X, out2[1] = the double E with sqrt(x) - agent_radius <= ray_radius
   <=> x <= E, for every x >= 0 (-1: no such x). */
int cat_radius_thresholds_host(double term_radius, double agent_radius, double ray_radius, double *out2);

/* The non-terminal rewards as arithmetic (csrc/cat_sim_reward.h), a bit-exact restatement of the two reward tables that the kernels do not use (measured
   slower than the table load: DESIGN 4.9) and the tests keep exact.  cat_reward_arith_host (host only, no device): writes the HOST build's value for every
   float16 distance to out[2][32768] (role 0 = cop, 1 = thief; out may be NULL) and returns the largest index m such that it equals both given tables bit
   for bit at every index <= m (-1: none, or a table pointer is NULL).  cat_reward_arith_max: that index for the handle's tables (computed on demand from a copy of them).
   cat_debug_reward_table: the DEVICE build's values, one small launch, out = DEVICE pointer to [2][32768] floats. */
int cat_reward_arith_host(const float *cop_lut, const float *thief_lut, float *out);
int cat_reward_arith_max(const cat_sim *sim);
int cat_debug_reward_table(const cat_sim *sim, float *out, void *stream);

#ifdef __cplusplus
}
#endif
#endif
