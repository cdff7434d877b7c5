// cat_sim_host.h -- part of the env core's single translation unit (included by cat_sim.hip, in this order; not a stand-alone header):
// host side, on the device: the handle, cat_create (plan_sim's plan uploaded), the launches and every other C-ABI entry that needs a device.
// One part of a sim as created: its plan's tables (host copy), parameter block (host and device), launch geometry and kernels.
struct Part {
    GridHost grid;                 // grid.desc[k] belongs to map map_ids[k] of the sim
    std::vector<int> map_ids;
    Params p;
    Params *dev_p = nullptr;
    Prologue pro;
    int n_blocks = 0, wpb = 0, n_envs = 0;
    size_t lds_bytes = 0;
    bool pool_step = false;   // the one-tick entry runs the pooled kernel (the resident one does whenever the ring exists: p.pool_mask)
    KernelChoice kernels;     // the instantiations matching (agents, rays, cops)
};

struct cat_sim {
    std::vector<Part> parts;
    int device;
    hipStream_t side = nullptr;                       // two parts: the second one's stream ...
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;  // ... forked from and joined to the caller's
    hipEvent_t t_start = nullptr, t_stop = nullptr;   // cat_arm_kernel_timing
    uint16_t *final_pos = nullptr;                    // cat_bind_final_positions: copied into the LaunchArgs of every stepping launch
    std::vector<MapDesc> maps;
    std::vector<void *> allocs;
    std::string one_tick_name, rollout_name;
    char err[256];
};

#define HIP_TRY(sim, expr)                                                                     \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess) {                                                                \
            snprintf((sim)->err, sizeof((sim)->err), "%s failed: %s", #expr, hipGetErrorString(e_)); \
            return CAT_ERR_HIP;                                                                \
        }                                                                                      \
    } while (0)

template <typename T>
static int dev_alloc(cat_sim *s, T **ptr, size_t count, const void *init)
{
    void *d = nullptr;
    size_t bytes = (count ? count : 1) * sizeof(T);
    HIP_TRY(s, hipMalloc(&d, bytes));
    s->allocs.push_back(d);
    if (init) HIP_TRY(s, hipMemcpy(d, init, count * sizeof(T), hipMemcpyHostToDevice));
    else HIP_TRY(s, hipMemset(d, 0, bytes));
    *ptr = static_cast<T *>(d);
    return CAT_OK;
}

extern "C" int cat_abi_version(void) { return CAT_ABI_VERSION; }
// (a sim of two parts: both names, "+"-joined, the group-form part first)
extern "C" const char *cat_one_tick_kernel(const cat_sim *sim) { return sim ? sim->one_tick_name.c_str() : ""; }
extern "C" const char *cat_rollout_kernel(const cat_sim *sim) { return sim ? sim->rollout_name.c_str() : ""; }
extern "C" const char *cat_last_error(const cat_sim *sim) { return sim ? sim->err : g_create_err; }
extern "C" int cat_chunks_per_unit(const cat_sim *sim, int resident)
{
    if (!sim) return CAT_ERR_BAD_ARG;
    const Part &pt = sim->parts.back();   // (two parts: the chunk-form part is the second)
    int best = 1;                          // (several maps: the largest figure)
    for (const GridDesc &d : pt.grid.desc) best = std::max(best, resident ? d.span : d.span_tick);
    return best;
}
extern "C" int cat_num_agents(const cat_sim *sim) { return sim ? sim->parts[0].p.A : CAT_ERR_BAD_ARG; }
extern "C" int cat_num_shapes(const cat_sim *sim, int m)
{
    if (!sim || m < 0 || m >= (int)sim->maps.size()) return CAT_ERR_BAD_ARG;
    return sim->maps[m].S;
}

static int check_device(int device, char *err)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1 || device < 0 || device >= ndev)
        PLAN_FAIL(CAT_ERR_NO_DEVICE, "no usable HIP device (count=%d, requested %d): this library has no CPU path", ndev, device);
    if (hipSetDevice(device) != hipSuccess) PLAN_FAIL(CAT_ERR_NO_DEVICE, "hipSetDevice(%d) failed", device);
    return CAT_OK;
}

// The plan on the device: every array of the plan allocated and copied, the pointers of the parameter blocks filled in, the kernels' LDS limit raised,
// the second part's stream.  Takes the candidate tables out of the plan (the handle keeps a host copy for cat_debug_grid_lookup).  Messages: s->err.
static int upload(cat_sim *s, const cat_tables *tab, SimPlan &plan)
{
#define TRY_ALLOC(call) do { const int rc_ = (call); if (rc_ != CAT_OK) return rc_; } while (0)
    s->maps = plan.descs;
    // ---- what every part shares: the env state records, the ray table and reward LUTs, the geometry of all maps, the error word, the static trees
    Params base = plan.base;
    TRY_ALLOC(dev_alloc(s, &base.state, plan.rec0.size(), plan.rec0.data()));
    TRY_ALLOC(dev_alloc(s, const_cast<double **>(&base.ray_dx), (size_t)base.R, tab->ray_dx));
    TRY_ALLOC(dev_alloc(s, const_cast<double **>(&base.ray_dy), (size_t)base.R, tab->ray_dy));
    TRY_ALLOC(dev_alloc(s, const_cast<float **>(&base.cop_lut), 32768, tab->cop_reward_lut));
    TRY_ALLOC(dev_alloc(s, const_cast<float **>(&base.thief_lut), 32768, tab->thief_reward_lut));
    TRY_ALLOC(dev_alloc(s, const_cast<MapDesc **>(&base.maps), plan.descs.size(), plan.descs.data()));
    TRY_ALLOC(dev_alloc(s, const_cast<double **>(&base.geo_f64), plan.geo_f.size(), plan.geo_f.data()));
    TRY_ALLOC(dev_alloc(s, const_cast<int **>(&base.geo_i32), plan.geo_i.size(), plan.geo_i.data()));
    TRY_ALLOC(dev_alloc(s, &base.err_word, 1, nullptr));
    if (plan.tree) {
        TRY_ALLOC(dev_alloc(s, const_cast<double **>(&base.tree_bb), plan.tree_bb.size(), plan.tree_bb.data()));
        TRY_ALLOC(dev_alloc(s, const_cast<int **>(&base.tree_link), plan.tree_link.size(), plan.tree_link.data()));
        TRY_ALLOC(dev_alloc(s, const_cast<int **>(&base.tree_root), plan.tree_root.size(), plan.tree_root.data()));
    }
    s->parts.resize(plan.parts.size());
    for (size_t pi = 0; pi < plan.parts.size(); pi++) {
        PartPlan &pp = plan.parts[pi];
        Part &pt = s->parts[pi];
        pt.map_ids = pp.map_ids;
        pt.n_envs = pp.n_envs; pt.n_blocks = pp.n_blocks; pt.wpb = pp.wpb; pt.lds_bytes = pp.lds_bytes; pt.pool_step = pp.pool_step;
        pt.kernels = pp.kernels;
        Params &p = pt.p;
        p = pp.p;
        p.state = base.state; p.ray_dx = base.ray_dx; p.ray_dy = base.ray_dy; p.cop_lut = base.cop_lut; p.thief_lut = base.thief_lut;
        p.maps = base.maps; p.geo_f64 = base.geo_f64; p.geo_i32 = base.geo_i32; p.err_word = base.err_word;
        p.tree_bb = base.tree_bb; p.tree_link = base.tree_link; p.tree_root = base.tree_root;
        const GridHost &g = pp.grid;
        TRY_ALLOC(dev_alloc(s, const_cast<GridDesc **>(&p.grids), g.desc.size(), g.desc.data()));
        TRY_ALLOC(dev_alloc(s, const_cast<unsigned long long **>(&p.grid_rows), g.rows.size(), g.rows.data()));
        TRY_ALLOC(dev_alloc(s, const_cast<int **>(&p.grid_off), pp.csr ? g.off.size() : 1, pp.csr ? g.off.data() : nullptr));
        TRY_ALLOC(dev_alloc(s, const_cast<unsigned char **>(&p.grid_ent), pp.csr ? g.ent.size() : 1, pp.csr ? g.ent.data() : nullptr));
        TRY_ALLOC(dev_alloc(s, const_cast<int **>(&p.cgrid_off), g.coff.size(), g.coff.data()));
        TRY_ALLOC(dev_alloc(s, const_cast<unsigned char **>(&p.cgrid_ent), g.cent.size(), g.cent.data()));
        TRY_ALLOC(dev_alloc(s, const_cast<unsigned long long **>(&p.cgrid_rows), g.crows.size(), g.crows.data()));
        TRY_ALLOC(dev_alloc(s, const_cast<int **>(&p.work_env), pp.work.size(), pp.work.data()));
        TRY_ALLOC(dev_alloc(s, const_cast<int **>(&p.block_map), pp.block_map.size(), pp.block_map.data()));
        TRY_ALLOC(dev_alloc(s, const_cast<BlockDesc **>(&p.block_desc), pp.block_desc.size(), pp.block_desc.data()));
        if (pt.lds_bytes > 64 * 1024)
            for (KernelFn fn : {pt.kernels.step, pt.kernels.reset, pt.kernels.rollout})
                if (hipFuncSetAttribute(reinterpret_cast<const void *>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)pt.lds_bytes) != hipSuccess) {
                    snprintf(s->err, sizeof s->err, "cannot raise dynamic LDS limit to %zu", pt.lds_bytes);
                    return CAT_ERR_HIP;
                }
        TRY_ALLOC(dev_alloc(s, &pt.dev_p, 1, &p));
        {   // the prologue's copy (third kernel argument)
            Prologue &q = pt.pro;
            memset(&q, 0, sizeof q);
            q.lds_map_bytes = p.lds_map_bytes; q.lds_env_bytes = p.lds_env_bytes; q.lds_union_bytes = p.lds_union_bytes; q.wpb = p.wpb;
            q.A = p.A; q.R = p.R; q.NP = p.NP; q.maxc = p.maxc; q.n_cops = p.n_cops; q.rec_bytes = p.rec_bytes; q.hot_bytes = p.hot_bytes; q.N = p.N;
            q.lds_pool_off = p.lds_pool_off; q.pool_mask = p.pool_mask; q.grp_rays = p.grp_rays;
            q.work_env = p.work_env; q.block_desc = p.block_desc; q.state = p.state; q.geo_f64 = p.geo_f64; q.geo_i32 = p.geo_i32;
            q.ray_dx = p.ray_dx; q.ray_dy = p.ray_dy; q.cop_lut = p.cop_lut; q.thief_lut = p.thief_lut;
            q.uniform = pp.uniform ? 1 : 0;
            q.bd = pp.block_desc[0];
        }
        pt.grid = std::move(pp.grid);
        s->one_tick_name += (pi ? "+" : "") + std::string(pt.pool_step ? "step_kernel_pooled" : "step_kernel");
        s->rollout_name += (pi ? "+" : "") + std::string(pt.p.pool_mask ? "rollout_kernel_pooled" : "rollout_kernel");
    }
#undef TRY_ALLOC
    if (s->parts.size() > 1) {   // the second part's launches run on a stream of the handle, forked from and joined to the caller's (launch_parts)
        if (hipStreamCreateWithFlags(&s->side, hipStreamNonBlocking) != hipSuccess || hipEventCreateWithFlags(&s->ev_fork, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&s->ev_join, hipEventDisableTiming) != hipSuccess) {
            snprintf(s->err, sizeof s->err, "cannot create the second part's stream / events");
            return CAT_ERR_HIP;
        }
    }
    return CAT_OK;
}

// Order of refusals: the arguments, the config, the device, then whatever plan_sim finds in the maps and the sizes.
extern "C" int cat_create(const cat_config *cfg, const cat_tables *tab, const void *const *blobs,
                          const size_t *sizes, int n_maps, const int32_t *slot_map_ids, int device,
                          cat_sim **out)
{
    if (const int rc = check_create_args(cfg, tab, blobs, sizes, n_maps, out != nullptr, g_create_err)) return rc;
    if (const int rc = check_device(device, g_create_err)) return rc;
    SimPlan plan;
    if (const int rc = plan_sim(cfg, tab, blobs, sizes, n_maps, slot_map_ids, plan, g_create_err)) return rc;
    if (plan.knobs.verbose) fputs(describe_plan(plan).c_str(), stderr);
    cat_sim *s = new cat_sim();
    s->err[0] = 0;
    s->device = device;
    const int rc = upload(s, tab, plan);
    if (rc != CAT_OK) {
        strncpy(g_create_err, s->err, sizeof g_create_err - 1);
        cat_destroy(s);
        return rc;
    }
    *out = s;
    return CAT_OK;
}

extern "C" int cat_destroy(cat_sim *s)
{
    if (!s) return CAT_ERR_BAD_ARG;
    (void)hipSetDevice(s->device);
    if (s->side) { (void)hipStreamSynchronize(s->side); (void)hipStreamDestroy(s->side); }
    if (s->ev_fork) (void)hipEventDestroy(s->ev_fork);
    if (s->ev_join) (void)hipEventDestroy(s->ev_join);
    for (void *d : s->allocs) (void)hipFree(d);
    delete s;
    return CAT_OK;
}

// One dispatch per part.  A sim of two parts launches the second on the handle's own stream, forked from the caller's stream by an event and joined back
// to it by another: for the caller the entry stays one stream-ordered operation, and the two kernels share the device.  An armed pair of timing events
// (cat_arm_kernel_timing) is attached to the dispatch itself when there is one, else recorded on the caller's stream around the fork and the join.
enum { kFnReset, kFnStep, kFnRollout };
static int launch_parts(cat_sim *s, const LaunchArgs &la, void *stream, int which)
{
    hipStream_t user = static_cast<hipStream_t>(stream);
    const bool two = s->parts.size() > 1;
    hipEvent_t t0 = nullptr, t1 = nullptr;
    if (which != kFnReset && s->t_start && s->t_stop) { t0 = s->t_start; t1 = s->t_stop; s->t_start = s->t_stop = nullptr; }
    auto launch = [&](const Part &pt, hipStream_t st, bool events) {
        const KernelFn fn = which == kFnReset ? pt.kernels.reset : (which == kFnStep ? pt.kernels.step : pt.kernels.rollout);
        const dim3 grid(pt.n_blocks), block(pt.wpb * kLanes);
        if (events) hipExtLaunchKernelGGL(fn, grid, block, pt.lds_bytes, st, t0, t1, 0, pt.dev_p, la, pt.pro);
        else hipLaunchKernelGGL(fn, grid, block, pt.lds_bytes, st, pt.dev_p, la, pt.pro);
    };
    if (!two) { launch(s->parts[0], user, t0 != nullptr); return CAT_OK; }
    if (t0) HIP_TRY(s, hipEventRecord(t0, user));
    HIP_TRY(s, hipEventRecord(s->ev_fork, user));
    HIP_TRY(s, hipStreamWaitEvent(s->side, s->ev_fork, 0));
    launch(s->parts[1], s->side, false);   // the chunk-form part first: its workgroups are the long ones
    HIP_TRY(s, hipEventRecord(s->ev_join, s->side));
    launch(s->parts[0], user, false);
    HIP_TRY(s, hipStreamWaitEvent(user, s->ev_join, 0));
    if (t1) HIP_TRY(s, hipEventRecord(t1, user));
    return CAT_OK;
}

// What every launching entry shares.  Head: cleared launch arguments with the caller's outputs.  Tail: the handle's device, one dispatch per part, the
// launch's status.
static LaunchArgs launch_args(const cat_outputs *out)
{
    LaunchArgs la;
    memset(&la, 0, sizeof la);
    if (out) la.out = *out;
    return la;
}
static int launch_entry(cat_sim *s, const LaunchArgs &la, void *stream, int which)
{
    HIP_TRY(s, hipSetDevice(s->device));
    const int rc = launch_parts(s, la, stream, which);
    if (rc != CAT_OK) return rc;
    HIP_TRY(s, hipGetLastError());
    return CAT_OK;
}

static int launch_reset(cat_sim *s, const uint8_t *mask, const double *positions, const cat_outputs *out,
                        int use_done, void *stream)
{
    if (!s) return CAT_ERR_BAD_ARG;
    LaunchArgs la = launch_args(out);
    la.mask = mask; la.positions = positions; la.use_done_mask = use_done;
    return launch_entry(s, la, stream, kFnReset);
}

extern "C" int cat_reset(cat_sim *s, const uint8_t *mask, const double *positions, const cat_outputs *out, void *stream)
{
    return launch_reset(s, mask, positions, out, 0, stream);
}

extern "C" int cat_reset_done(cat_sim *s, const cat_outputs *out, void *stream)
{
    return launch_reset(s, nullptr, nullptr, out, 1, stream);
}

extern "C" int cat_arm_kernel_timing(cat_sim *s, void *start_event, void *stop_event)
{
    if (!s || !start_event || !stop_event) return CAT_ERR_BAD_ARG;
    s->t_start = static_cast<hipEvent_t>(start_event); s->t_stop = static_cast<hipEvent_t>(stop_event);
    return CAT_OK;
}

extern "C" int cat_step(cat_sim *s, const int32_t *actions, const cat_outputs *out, void *stream)
{
    if (!s || !actions) { if (s) snprintf(s->err, sizeof s->err, "cat_step: actions is NULL"); return CAT_ERR_BAD_ARG; }
    LaunchArgs la = launch_args(out);
    la.actions = actions; la.final_pos = s->final_pos;
    return launch_entry(s, la, stream, kFnStep);
}

extern "C" int cat_step_fused(cat_sim *s, const int32_t *actions, uint64_t synth_tick, int auto_reset,
                              const cat_outputs *out, void *stream)
{
    if (!s) return CAT_ERR_BAD_ARG;
    LaunchArgs la = launch_args(out);
    la.actions = actions; la.synth_tick = synth_tick;
    la.auto_reset = auto_reset ? 1 : 0;   // finished episodes are reset inside the same launch (no second kernel)
    la.final_pos = s->final_pos;
    return launch_entry(s, la, stream, kFnStep);
}

extern "C" int cat_rollout_fused(cat_sim *s, int T, const int32_t *actions, uint64_t synth_tick0, int auto_reset,
                                 const cat_outputs *out, void *stream)
{
    if (!s) return CAT_ERR_BAD_ARG;
    if (T < 1 || T > CAT_MAX_ROLLOUT_TICKS) { snprintf(s->err, sizeof s->err, "cat_rollout_fused: T = %d outside 1..%d", T, CAT_MAX_ROLLOUT_TICKS); return CAT_ERR_BAD_ARG; }
    LaunchArgs la = launch_args(out);
    la.actions = actions; la.synth_tick = synth_tick0; la.T = T;
    la.auto_reset = auto_reset ? 1 : 0;
    la.final_pos = s->final_pos;
    return launch_entry(s, la, stream, kFnRollout);
}

// One decision of k held-action ticks per env slot in ONE resident launch (the sim's rollout kernel with T = k in repeat mode): see include/cat_sim.h.
extern "C" int cat_step_repeat(cat_sim *s, int k, const int32_t *actions, int auto_reset, const cat_outputs *out, int32_t *ticks, void *stream)
{
    if (!s) return CAT_ERR_BAD_ARG;
    if (k < 1 || k > CAT_MAX_ROLLOUT_TICKS) { snprintf(s->err, sizeof s->err, "cat_step_repeat: k = %d outside 1..%d", k, CAT_MAX_ROLLOUT_TICKS); return CAT_ERR_BAD_ARG; }
    if (!actions) { snprintf(s->err, sizeof s->err, "cat_step_repeat: actions is NULL (synthetic actions are not offered by this entry)"); return CAT_ERR_BAD_ARG; }
    LaunchArgs la = launch_args(out);
    la.actions = actions; la.T = k; la.repeat = 1; la.ticks = ticks;
    la.auto_reset = auto_reset ? 1 : 0;
    la.final_pos = s->final_pos;
    return launch_entry(s, la, stream, kFnRollout);
}

// End-of-episode positions: the handle keeps the pointer, every stepping entry hands it to its launch (see include/cat_sim.h).  No device call.
extern "C" int cat_bind_final_positions(cat_sim *s, uint16_t *buf)
{
    if (!s) return CAT_ERR_BAD_ARG;
    s->final_pos = buf;
    return CAT_OK;
}

extern "C" int cat_random_actions(cat_sim *s, uint64_t tick, int32_t *actions, void *stream)
{
    if (!s || !actions) return CAT_ERR_BAD_ARG;
    HIP_TRY(s, hipSetDevice(s->device));
    const int n = s->parts[0].p.N * s->parts[0].p.A;
    hipLaunchKernelGGL(random_actions_kernel, dim3((n + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream),
                       s->parts[0].dev_p, (unsigned long long)tick, actions);
    HIP_TRY(s, hipGetLastError());
    return CAT_OK;
}

extern "C" int cat_device_errors(cat_sim *s, uint32_t *flags, int clear, void *stream)
{
    if (!s || !flags) return CAT_ERR_BAD_ARG;
    HIP_TRY(s, hipSetDevice(s->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    HIP_TRY(s, hipMemcpyAsync(flags, s->parts[0].p.err_word, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    if (clear) HIP_TRY(s, hipMemsetAsync(s->parts[0].p.err_word, 0, sizeof(uint32_t), st));
    HIP_TRY(s, hipStreamSynchronize(st));
    if (*flags) snprintf(s->err, sizeof s->err, "device-side error flags 0x%x:%s%s%s", *flags,
                         (*flags & CAT_DEVERR_BAD_ACTION) ? " an action outside 0..3 (applied as no impulse)" : "",
                         (*flags & CAT_DEVERR_CONTACT_DROPPED) ? " a contact was dropped (more simultaneous contacts than the cache / contact array holds)" : "",
                         (*flags & CAT_DEVERR_SCHEDULER) ? " a work item of the pooled ray fan never arrived (results of that launch are invalid)" : "");
    return CAT_OK;
}

extern "C" int cat_set_seed(cat_sim *s, uint64_t seed, void *stream)
{
    if (!s) return CAT_ERR_BAD_ARG;
    HIP_TRY(s, hipSetDevice(s->device));
    for (Part &pt : s->parts) {
        pt.p.seed = seed;
        // the 8-byte source lives in the handle, which outlives the async copy
        HIP_TRY(s, hipMemcpyAsync(&pt.dev_p->seed, &pt.p.seed, sizeof(pt.p.seed), hipMemcpyHostToDevice, static_cast<hipStream_t>(stream)));
    }
    return CAT_OK;
}

static int copy_state(cat_sim *s, const cat_state *v, bool get, void *stream)
{
    if (!s || !v) return CAT_ERR_BAD_ARG;
    HIP_TRY(s, hipSetDevice(s->device));
    const Params &p = s->parts[0].p;   // (the record layout and the state pointer are the same in every part)
    const int A = p.A;
    const RecLayout rl(A);
    hipStream_t st = static_cast<hipStream_t>(stream);
    // field <-> strided slice of the per-env records
    auto cp = [&](void *user, size_t rec_off, size_t width) -> hipError_t {
        if (!user || width == 0) return hipSuccess;
        char *recp = p.state + rec_off;
        return get ? hipMemcpy2DAsync(user, width, recp, (size_t)p.rec_bytes, width, (size_t)p.N, hipMemcpyDeviceToDevice, st)
                   : hipMemcpy2DAsync(recp, (size_t)p.rec_bytes, user, width, width, (size_t)p.N, hipMemcpyDeviceToDevice, st);
    };
    const size_t D = 8, I = 4;
    const bool cold_touched = v->wall_jn || v->pair_jn || v->wall_shape || v->wall_age || v->pair_age;
    // a slot whose cache_live flag is 0 keeps STALE bytes in the cold part of its record: make them say "empty" before
    // they are read out, and raise the flag of every slot after cold fields were written from outside
    if (get) hipLaunchKernelGGL(cold_fixup_kernel, dim3((p.N + 255) / 256), dim3(256), 0, st, s->parts[0].dev_p, 0);
    HIP_TRY(s, cp(v->pos, rl.pos(), 2 * A * D));
    HIP_TRY(s, cp(v->vel, rl.vel(), 2 * A * D));
    HIP_TRY(s, cp(v->vbias, rl.vbias(), 2 * A * D));
    HIP_TRY(s, cp(v->tc, rl.tc(), 2 * A * D));
    HIP_TRY(s, cp(v->leaf_bb, rl.leaf_bb(), 4 * A * D));
    HIP_TRY(s, cp(v->step_count, rl.step_count(), I));
    HIP_TRY(s, cp(v->reset_count, rl.reset_count(), I));
    HIP_TRY(s, cp(v->wall_jn, rl.wall_jn(), (size_t)A * kK * D));
    if (p.NP > 0) HIP_TRY(s, cp(v->pair_jn, rl.pair_jn(), (size_t)p.NP * D));
    HIP_TRY(s, cp(v->wall_shape, rl.wall_shape(), (size_t)A * kK * I));
    HIP_TRY(s, cp(v->wall_age, rl.wall_age(), (size_t)A * kK * I));
    if (p.NP > 0) HIP_TRY(s, cp(v->pair_age, rl.pair_age(), (size_t)p.NP * I));
    if (!get && cold_touched) hipLaunchKernelGGL(cold_fixup_kernel, dim3((p.N + 255) / 256), dim3(256), 0, st, s->parts[0].dev_p, 1);
    HIP_TRY(s, hipGetLastError());
    return CAT_OK;
}

extern "C" int cat_get_state(cat_sim *s, const cat_state *dst, void *stream) { return copy_state(s, dst, true, stream); }
extern "C" int cat_set_state(cat_sim *s, const cat_state *src, void *stream) { return copy_state(s, src, false, stream); }

#ifdef CAT_PHASE_TIMING
static unsigned long long g_last_counts[8];
// event counters as of the last cat_debug_phase_cycles call: shape-query rounds / their lanes, classification iterations / lanes,
// exact face iterations / lanes, exact corner iterations / lanes (the counting distorts the cycle marks of the same run)
extern "C" void cat_debug_counts(unsigned long long *out8) { for (int i = 0; i < 8; i++) out8[i] = g_last_counts[i]; }
extern "C" int cat_debug_phase_cycles(unsigned long long *out24, int reset)
{
    unsigned long long h[32];
    if (hipMemcpyFromSymbol(h, HIP_SYMBOL(g_phase_cycles), sizeof h) != hipSuccess) return CAT_ERR_HIP;
    for (int i = 0; i < 24; i++) out24[i] = h[i];
    for (int i = 24; i < 32; i++) g_last_counts[i - 24] = h[i];
    if (reset) { memset(h, 0, sizeof h); if (hipMemcpyToSymbol(HIP_SYMBOL(g_phase_cycles), h, sizeof h) != hipSuccess) return CAT_ERR_HIP; }
    return CAT_OK;
}
#endif

// Host copy of the spatial-hash tables, for tests: candidate walls of ray k (k >= 0) or contact
// candidates (k < 0) for an origin at (x, y) on map `map_index`.  Returns the count (ids in out).
extern "C" int cat_debug_grid_lookup(const cat_sim *s, int map_index, double x, double y, int k, int *out, int max_out)
{
    if (!s || map_index < 0 || map_index >= (int)s->maps.size() || k >= s->parts[0].p.R) return CAT_ERR_BAD_ARG;
    for (const Part &pt : s->parts)
        for (size_t q = 0; q < pt.map_ids.size(); q++)
            if (pt.map_ids[q] == map_index) return grid_lookup(pt.grid, (int)q, pt.p.R, x, y, k, out, max_out);
    return CAT_ERR_BAD_ARG;
}

extern "C" int cat_selftest_arith(int op, const double *a, const double *b, double *out, int n, int device, void *stream)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1 || device < 0 || device >= ndev) {
        snprintf(g_create_err, sizeof g_create_err, "no usable HIP device");
        return CAT_ERR_NO_DEVICE;
    }
    if (hipSetDevice(device) != hipSuccess) return CAT_ERR_NO_DEVICE;
    hipLaunchKernelGGL(selftest_kernel, dim3((n + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), op, a, b, out, n);
    return hipGetLastError() == hipSuccess ? CAT_OK : CAT_ERR_HIP;
}

extern "C" int cat_radius_thresholds_host(double term_radius, double agent_radius, double ray_radius, double *out2)
{
    if (!out2) return CAT_ERR_BAD_ARG;
    out2[0] = radius_lt_threshold(term_radius);
    out2[1] = radius_le_threshold(agent_radius, ray_radius);
    return CAT_OK;
}

extern "C" int cat_reward_arith_host(const float *cop_lut, const float *thief_lut, float *out)
{
    if (out)
        for (int i = 0; i < 2 * 32768; i++) out[i] = (float)ra_host_f16_to_f64(reward_arith_f16(i < 32768, (unsigned)i & 0x7FFFu));
    return cop_lut && thief_lut ? reward_arith_scan(cop_lut, thief_lut) : -1;
}

// (on demand, host only: 64 k evaluations against a copy of the handle's tables -- no kernel and no device structure knows the value)
extern "C" int cat_reward_arith_max(const cat_sim *s)
{
    if (!s) return CAT_ERR_BAD_ARG;
    std::vector<float> lut(2 * 32768);
    if (hipSetDevice(s->device) != hipSuccess) return CAT_ERR_NO_DEVICE;
    if (hipMemcpy(lut.data(), s->parts[0].p.cop_lut, 32768 * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(lut.data() + 32768, s->parts[0].p.thief_lut, 32768 * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) return CAT_ERR_HIP;
    return reward_arith_scan(lut.data(), lut.data() + 32768);
}

extern "C" int cat_debug_reward_table(const cat_sim *s, float *out, void *stream)
{
    if (!s || !out) return CAT_ERR_BAD_ARG;
    if (hipSetDevice(s->device) != hipSuccess) return CAT_ERR_NO_DEVICE;
    hipLaunchKernelGGL(reward_table_kernel, dim3(2 * 32768 / 256), dim3(256), 0, static_cast<hipStream_t>(stream), out);
    return hipGetLastError() == hipSuccess ? CAT_OK : CAT_ERR_HIP;
}
