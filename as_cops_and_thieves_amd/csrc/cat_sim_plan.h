// cat_sim_plan.h -- part of the env core's single translation unit (included by cat_sim.hip, in this order; not a stand-alone header):
// host side, no device needed: the state-record layout, LDS sizing, kernel selection and plan_sim -- every decision cat_create takes and every table it
// uploads, as a SimPlan -- with describe_plan (the text CAT_VERBOSE prints) and cat_plan_describe_host.  No HIP runtime call in this file.

// ---------------------------------------------------------------------- the state record ----
// One env slot's record for a roster of A agents (documented at Params::state), stated once for the host side: byte offsets of every field, the size of
// the hot part and of the whole record.  The fixed-dimension kernels carry the same sizes at compile time (FixDims: take_roster asserts they agree).
struct RecLayout {
    int A, NPs;   // agents; agent pairs, at least one
    constexpr explicit RecLayout(int a) : A(a), NPs(a * (a - 1) / 2 > 0 ? a * (a - 1) / 2 : 1) {}
    // hot: f64 pos[2A] vel[2A] vbias[2A] tc[2A] leaf[4A], i32 step_count reset_count done cache_live
    constexpr int pos() const { return 0; }
    constexpr int vel() const { return 16 * A; }
    constexpr int vbias() const { return 32 * A; }
    constexpr int tc() const { return 48 * A; }
    constexpr int leaf_bb() const { return 64 * A; }
    constexpr int step_count() const { return 96 * A; }
    constexpr int reset_count() const { return 96 * A + 4; }
    constexpr int hot_bytes() const { return 96 * A + 16; }
    // cold: f64 wall_jn[8A] pair_jn[NPs], i32 wall_shape[8A] wall_age[8A] pair_age[NPs]
    constexpr int wall_jn() const { return hot_bytes(); }
    constexpr int pair_jn() const { return hot_bytes() + A * kK * 8; }
    constexpr int wall_shape() const { return hot_bytes() + (A * kK + NPs) * 8; }
    constexpr int wall_age() const { return wall_shape() + A * kK * 4; }
    constexpr int pair_age() const { return wall_shape() + 2 * A * kK * 4; }
    constexpr int cold_bytes() const { return ((A * kK + NPs) * 8 + (2 * A * kK + NPs) * 4 + 15) / 16 * 16; }
    constexpr int rec_bytes() const { return hot_bytes() + cold_bytes(); }
};

// ---------------------------------------------------------------------- LDS carve ----
// LDS carve sizes (must match carve())
struct LdsSizes {
    int map, env, uni;
    int racc;   // offset in an env area of the [A] f32 reward accumulators of cat_step_repeat
    int o16;    // ... of the [A] float16 origins (Lds::o16)
    size_t total(int wpb) const { return (size_t)map + (size_t)ctrl_bytes(wpb) + (size_t)wpb * ((size_t)env + (size_t)uni); }
};
constexpr size_t kLdsBytes = 160 * 1024;   // of a CU (gfx950)
static LdsSizes lds_sizes(int A, int R, int maxS, int maxP, int maxPP, bool group_fan, int maxc, bool env_pad, int grp_rays = 4 * 64)
{
    auto up = [](int x, int a) { return (x + a - 1) / a * a; };
    LdsSizes z;
    const int rest = 8 * maxP + (kPairF / 2) * maxPP;
    z.map = up((kBB * maxS + rest) * 8 + 2 * maxS * 4, 16) + 16 * R;
    const int phys_bytes = kConD * 8 * maxc;   // contact records (physics_env)
    const int fan_bytes = kFanBytes + (group_fan ? grp_rays * (4 + 1 + 1) : 0);   // the rays of an agent group (four chunks unless the ray pool needs the LDS): arow, alist, adyn
    z.uni = up(phys_bytes > fan_bytes ? phys_bytes : fan_bytes, 16);
    int eb = RecLayout(A).rec_bytes() + 8 * A * 8;                 // record, spawn/snapshot
    eb += (3 * A + 2 * A * A + A + A + 4) * 4;                     // acell, anear, dk0, dcnt, adn, dmin, flags
    // cat_step_repeat's reward accumulators ([A] f32) take the bytes the staging's 16-byte alignment leaves free behind the flags where they fit there
    // (2v1: 12 of 12, 1v1: 8 of 8), else the end of the area -- which the padding below absorbs for 3v2: the carve of every instantiated shape keeps its size
    const int gap = up(eb, 16) - eb;
    z.racc = gap >= 4 * A ? eb : -1;
    const int stage0 = eb;
    eb = up(eb, 16) + up(A * R * 2, 16) + up(A * R, 16) + up(2 * R * 2, 16) + up(2 * R, 16);   // output staging
    if (z.racc < 0) { z.racc = eb; eb += up(4 * A, 16); }
    // The float16 origins ([A] words) go where the area has room already: the first gap that the 16-byte alignment leaves behind a staging array (the arrays are
    // written and stored element by element up to their own length: wide_store), else the end -- where the padding below absorbs them for 2v1 at 64 rays, 3v2 and
    // 2v2: none of the instantiated and recorded shapes' areas grows by them.  A roster / ray count with neither a gap nor pad slack grows by 16 bytes per
    // slot, and a ring that only just fitted such a shape drops to the next attempt (exact capacity, smaller group arrays, or no ring).
    z.o16 = -1;
    {
        const int sz[4] = {A * R * 2, A * R, 2 * R * 2, 2 * R};
        int off = up(stage0, 16);
        for (int q = 0; q < 4; q++) {
            const int a4 = up(off + sz[q], 4), next = up(off + sz[q], 16);
            if (z.o16 < 0 && next - a4 >= 4 * A) z.o16 = a4;
            off = next;
        }
    }
    if (z.o16 < 0) { z.o16 = eb; eb += 4 * A; }
    z.env = up(eb, 16);
    // The pooled rounds address env areas PER LANE (a round's rays come from several slots: origin, cached circles, "inside" walls, output staging of the
    // lane's slot).  An area of a multiple of 256 bytes -- 2v1 at 64 rays: exactly 2048 -- puts the same field of every slot on the same LDS banks; with
    // 16 A bytes more (the step between two agents' 16-byte fields) neighbouring slots' fields of any two agents fall on different banks.  env_pad
    // (Knobs::env_pad, CAT_ENV_PAD=0): off.
    const int want = (16 * A) % 256;
    if (env_pad && want != 0 && z.env % 256 != want) z.env += (want - z.env % 256 + 256) % 256;
    return z;
}

// ---------------------------------------------------------------------- kernel selection ----
// Kernel instantiations: fixed dimensions for the rosters / ray counts of the BASELINE configurations and of the
// reference's defaults, the generic one for everything else (Knobs::generic_kernel forces it: A/B tests).
using KernelFn = void (*)(const Params *, const LaunchArgs, const Prologue);
struct KernelChoice {
    KernelFn reset = nullptr, rollout = nullptr, step = nullptr;   // cat_reset*, cat_rollout_fused / cat_step_repeat, cat_step*
    std::string variant;
    // whether chunk-form kernels carry fan_slot -- the fixed-dimension ones at 64 rays (with run-time dimensions, or at 90 rays, a unit of several chunks
    // would need scratch): only then may plan_part give a map several chunks per work unit
    bool carries_slot = false;
};
// what decides the choice.  fan: 0 = chunk by chunk, 1 = agent groups with compacted rays; pool_roll / pool_step: the part's rays fit a workgroup ring and the
// resident / the one-tick entry runs the pooled fan; exact: the ring's capacity is not a power of two; tree: walls in Chipmunk's tree order (chunk form only)
struct KernelQuery { int A, R, n_cops, fan; bool pool_roll, pool_step, exact, tree, generic; bool pooled() const { return (pool_roll || pool_step) && fan == 1; } };

template <class D> static void kernels_of(int fan, KernelChoice &k)
{
    if (fan == 1) { k.reset = reset_kernel<WithFan<D, 1>>; k.rollout = rollout_kernel<WithFan<D, 1>>; k.step = step_kernel<WithFan<D, 1>>; }
    else { k.reset = reset_kernel<WithFan<D, 0>>; k.rollout = rollout_kernel<WithFan<D, 0>>; k.step = step_kernel<WithFan<D, 0>>; }
}
template <class D, bool kExact> static void pooled_of(const KernelQuery &q, KernelChoice &k)
{
    if (q.pool_roll) k.rollout = rollout_kernel_pooled<WithFan<D, 1>, kExact>;
    if (q.pool_step) k.step = step_kernel_pooled<WithFan<D, 1>, kExact>;
}
template <class D> struct RosterOf;
template <int TA, int TR, int TC> struct RosterOf<FixDims<TA, TR, TC>> { static constexpr int A = TA, R = TR, n_cops = TC; };
// One fixed-dimension roster: its unit-form kernels in both forms of the fan, and its pooled kernels for ONE kind of ring -- kExact says which: the ring of
// wpb * A * R entries is a power of two or not at the workgroup size the roster gets.  A sim of the roster whose ring is of the other kind runs the generic
// pooled kernels.  slot: its chunk-form kernels carry fan_slot.
template <class D, bool kExact> static bool take_roster(const KernelQuery &q, bool slot, KernelChoice &k)
{
    using Ro = RosterOf<D>;
    static_assert(RecLayout(Ro::A).hot_bytes() == D::kHotBytes && RecLayout(Ro::A).cold_bytes() == D::kColdBytes, "RecLayout and FixDims describe one record");
    if (q.generic || q.A != Ro::A || q.n_cops != Ro::n_cops || q.R != Ro::R || (q.pooled() && q.exact != kExact)) return false;
    kernels_of<D>(q.fan, k);
    if (q.pooled()) pooled_of<D, kExact>(q, k);
    char name[96];
    snprintf(name, sizeof name, "%d agents (%d cop%s), %d rays%s", Ro::A, Ro::n_cops, Ro::n_cops == 1 ? "" : "s", Ro::R, q.pooled() ? ", pooled fan" : "");
    k.variant = name;
    k.carries_slot = slot && !q.pooled();
    return true;
}
static KernelChoice select_kernels(const KernelQuery &q)
{
    KernelChoice k;
    if (q.tree) {
        k.reset = reset_kernel<WithFan<TreeDims, 0>>; k.rollout = rollout_kernel<WithFan<TreeDims, 0>>; k.step = step_kernel<WithFan<TreeDims, 0>>;
        k.variant = "generic, tree order";
        return k;
    }
    if (take_roster<FixDims<3, 64, 2>, false>(q, true, k)) return k;
#ifndef CAT_QUICK_BUILD   // diagnostic builds (tools/build_variant.sh -DCAT_QUICK_BUILD): the headline instantiation + the generic one only
    if (take_roster<FixDims<3, 90, 2>, true>(q, false, k)) return k;
    if (take_roster<FixDims<5, 64, 3>, true>(q, true, k)) return k;    // BASELINE configs[3]: the ring fits since the contact arrays are sized by the map
    if (take_roster<FixDims<2, 90, 1>, false>(q, false, k)) return k;   // the reference's own defaults: 1v1 (simple_env.py), 90 rays (entity.py:86)
#endif
    kernels_of<DynDims>(q.fan, k);
    if (q.pooled()) { if (q.exact) pooled_of<DynDims, true>(q, k); else pooled_of<DynDims, false>(q, k); }
    k.variant = q.pooled() ? "generic, pooled fan" : "generic";
    return k;
}

// ---------------------------------------------------------------------- the plan ----
// The env slots of a sim whose maps take one form of the ray fan: their candidate tables, parameter block, LDS carve, work list and kernels -- one
// dispatch per entry.  A sim has one part, or two when its maps want both forms (split_parts).
struct PartPlan {
    int fan = 0;                    // 1: group form, 0: chunk form
    std::vector<int> map_ids;       // the part's maps; grid.desc[k] belongs to map map_ids[k] of the sim
    std::vector<int> map_max_row;   // per map of the part: its longest candidate list
    GridHost grid;
    bool csr = false;               // some list overflows its row: the CSR arrays of the ray grid are uploaded (else one-element stand-ins)
    int n_envs = 0, n_blocks = 0, wpb = 0;
    int wall_depth = 0;             // the most wall bbs one agent's bb can overlap at once on a map of the part
    LdsSizes lds{};
    size_t lds_bytes = 0;           // of a workgroup, the ring included
    int pool_cap = 0;               // entries of the workgroup's ray ring (0: none)
    double empty_rows = 0.0;        // share of the (cell, ray) rows sampled around the spawn points that list no wall
    bool pool_step = false;         // the one-tick entry runs the pooled kernel (the resident one does whenever the ring exists)
    std::vector<int> work, block_map;
    std::vector<BlockDesc> block_desc;
    bool uniform = false;           // one map and the identity work list: a workgroup needs neither load (Prologue::uniform)
    Params p;                       // every scalar as uploaded; every pointer null (cat_create's upload fills them)
    KernelChoice kernels;
};
struct SimPlan {
    Knobs knobs;
    int n_maps = 0;
    std::vector<MapDesc> descs;
    std::vector<double> geo_f;
    std::vector<int> geo_i;
    std::vector<int> slot;              // env slot -> map
    std::vector<char> rec0;             // the initial state records
    bool tree = false;                  // tree order: every map's static tree, node indices of the sim (the maps' trees one after the other)
    std::vector<double> tree_bb;
    std::vector<int> tree_link, tree_root;
    Params base;                        // what every part shares; pointers null
    std::vector<PartPlan> parts;
};

constexpr size_t kErrBytes = 256;   // of every message buffer (g_create_err, cat_sim::err)
#define PLAN_FAIL(code, ...) do { snprintf(err, kErrBytes, __VA_ARGS__); return (code); } while (0)

static int check_create_args(const cat_config *cfg, const cat_tables *tab, const void *const *blobs, const size_t *sizes, int n_maps, bool has_out, char *err)
{
    if (!cfg || !tab || !blobs || !sizes || !has_out || n_maps < 1) PLAN_FAIL(CAT_ERR_BAD_ARG, "null argument");
    const int A = cfg->n_cops + cfg->n_thieves;
    if (A < 1 || A > CAT_MAX_AGENTS || cfg->n_cops < 0 || cfg->n_thieves < 0 || cfg->n_rays < 1 ||
        cfg->n_rays > CAT_MAX_RAYS || cfg->n_envs < 1 || A * kK > 64 || cfg->bbtree_gate > CAT_GATE_TREE)
        PLAN_FAIL(CAT_ERR_BAD_CONFIG, "bad config: agents=%d rays=%d envs=%d bbtree_gate=%d", A, cfg->n_rays, cfg->n_envs, cfg->bbtree_gate);
    return CAT_OK;
}

// ---- the blobs into one packed geometry buffer: per map [bb][planes][f32 edge pairs][start][regions] and [first S][count S][region_off A+1][first pair S]
static int plan_geometry(const cat_config *cfg, const void *const *blobs, const size_t *sizes, int n_maps, SimPlan &plan, std::vector<int> &wall_depth, char *err)
{
    const int A = cfg->n_cops + cfg->n_thieves;
    std::vector<double> &geo_f = plan.geo_f;
    std::vector<int> &geo_i = plan.geo_i;
    plan.descs.assign((size_t)n_maps, MapDesc{});
    wall_depth.assign((size_t)n_maps, 0);
    for (int m = 0; m < n_maps; m++) {
        MapBlob mb;
        const int r = read_map_blob(blobs[m], sizes[m], mb);
        if (r == kBlobTooSmall) PLAN_FAIL(CAT_ERR_BAD_MAP, "map blob %d too small", m);
        if (r != kBlobOk || mb.A != A || mb.n_cops != cfg->n_cops)
            PLAN_FAIL(CAT_ERR_BAD_MAP, "map blob %d invalid, roster mismatch or more than %d shapes", m, CAT_MAX_SHAPES);
        MapDesc d{};
        d.S = mb.S; d.P = mb.P; d.A = mb.A; d.n_regions = mb.n_regions;
        const std::vector<double> &f = mb.f;
        const std::vector<int> &iv = mb.iv;
        for (int sidx = 0; sidx < d.S; sidx++)   // feature codes (edge, count + corner) must stay below kFeatNear; circle_poly_contact: lane = edge
            if (iv[d.S + sidx] < 1 || iv[d.S + sidx] > CAT_MAX_HULL_EDGES)
                PLAN_FAIL(CAT_ERR_BAD_MAP, "map blob %d: wall %d has %d hull edges (1..%d supported)", m, sidx, iv[d.S + sidx], CAT_MAX_HULL_EDGES);
        // bb overlap is a loose bound on simultaneous CONTACTS (slanted or star-shaped walls overlap boxes without touching):
        // Knobs::allow_deep_wall_overlap accepts such a map, with CAT_DEVERR_CONTACT_DROPPED as the run-time check
        const int depth = max_wall_bb_depth(mb.bb(), d.S, cfg->agent_radius);
        wall_depth[(size_t)m] = depth;
        if (depth > CAT_WALL_CACHE && !plan.knobs.allow_deep_wall_overlap)
            PLAN_FAIL(CAT_ERR_BAD_MAP, "map blob %d: an agent can touch the bounding boxes of %d walls at once; the state record "
                      "caches %d wall contacts per agent (CAT_WALL_CACHE); CAT_ALLOW_DEEP_WALL_OVERLAP=1 accepts the map", m, depth, CAT_WALL_CACHE);
        d.f64_off = (int)geo_f.size();
        const size_t n_geo = mb.n_geo();
        geo_f.insert(geo_f.end(), f.begin() + 2, f.begin() + 2 + n_geo);  // drop window w,h: [bb][planes]
        std::vector<int> first_pair((size_t)d.S, 0);
        {   // f32 copy of the plane records for the ray fan's conservative pre-classification (poly_query_feat)
            const double rsum = cfg->wall_radius + cfg->ray_radius;
            const double *pl = mb.planes();
            float cmax = 0.0f;
            auto rec8 = [&](int q, float *o) {   // n.x n.y c dtMin | dtMax v0.x v0.y -
                const double *r8 = pl + 8 * (size_t)q;   // n.x n.y v0.x v0.y dot(v0,n) dtMin dtMax -
                o[0] = (float)r8[0]; o[1] = (float)r8[1]; o[2] = (float)(r8[4] + rsum); o[3] = (float)r8[5];
                o[4] = (float)r8[6]; o[5] = (float)r8[2]; o[6] = (float)r8[3];
                cmax = std::fmax(cmax, std::fabs(o[2]));
            };
            std::vector<float> prs;
            int pp = 0;
            for (int sidx = 0; sidx < d.S; sidx++) {
                const int first = iv[sidx], count = iv[d.S + sidx];
                first_pair[sidx] = pp;
                for (int e = 0; e < count; e += 2, pp++) {
                    float a[8] = {0}, b[8] = {0.f, 0.f, 1e30f, 1e30f, -1e30f, 1e18f, 1e18f, 0.f};   // b: an edge nothing can reach
                    rec8(first + e, a);
                    if (e + 1 < count) rec8(first + e + 1, b);
                    const float rec[kPairF] = {a[0], b[0], a[1], b[1], a[2], b[2], a[3], b[3], a[4], b[4], a[5], b[5], a[6], b[6], 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                    prs.insert(prs.end(), rec, rec + kPairF);
                }
            }
            d.PP = pp;
            const size_t at = geo_f.size();
            geo_f.resize(at + (kPairF / 2) * (size_t)pp);
            memcpy(geo_f.data() + at, prs.data(), prs.size() * sizeof(float));
            d.cmax = cmax;
        }
        geo_f.insert(geo_f.end(), f.begin() + 2 + n_geo, f.end());        // [start][regions]
        d.i32_off = (int)geo_i.size();
        geo_i.insert(geo_i.end(), iv.begin(), iv.end());
        geo_i.insert(geo_i.end(), first_pair.begin(), first_pair.end());   // [first S][count S][region_off A+1][first pair S]
        if (geo_f.size() & 1) geo_f.push_back(0.0);  // keep 16-byte alignment of each map's base
        plan.descs[m] = d;
    }
    return CAT_OK;
}

// ---- tree order: every map's static tree (read-only, from global memory: only the rays of fan_chunk's slow path read them)
static int plan_trees(SimPlan &plan, char *err)
{
    for (int m = 0; m < plan.n_maps; m++) {
        std::vector<TreeNode> tn;
        int root = -1, depth = 0;
        build_static_tree(plan.geo_f.data() + plan.descs[m].f64_off, plan.descs[m].S, tn, root, depth);
        if (depth > kMaxTreeDepth)
            PLAN_FAIL(CAT_ERR_BAD_MAP, "map blob %d: its static tree is %d levels deep; tree order (bbtree_gate = %d) supports at most %d", m, depth, CAT_GATE_TREE, kMaxTreeDepth);
        const int base = (int)plan.tree_link.size() / 4;
        auto at = [base](int x) { return x >= 0 ? x + base : x; };
        plan.tree_root.push_back(base + root);
        for (const TreeNode &q : tn) {
            plan.tree_bb.insert(plan.tree_bb.end(), q.bb, q.bb + 4);
            const int link[4] = {at(q.a), at(q.b), at(q.parent), q.wall};
            plan.tree_link.insert(plan.tree_link.end(), link, link + 4);
        }
    }
    return CAT_OK;
}

// ---- env state records as they are before the first reset (layout: RecLayout)
static void plan_initial_records(const cat_config *cfg, SimPlan &plan)
{
    const int A = plan.base.A, N = plan.base.N;
    const RecLayout rl(A);
    plan.rec0.assign((size_t)N * rl.rec_bytes(), 0);
    for (int e = 0; e < N; e++) {
        const MapDesc &d = plan.descs[plan.slot[e]];
        const double *start = plan.geo_f.data() + d.f64_off + 4 * d.S + geo_rest_doubles(d);
        char *rec = plan.rec0.data() + (size_t)e * rl.rec_bytes();
        double *pos = reinterpret_cast<double *>(rec + rl.pos()), *tc = reinterpret_cast<double *>(rec + rl.tc()), *leaf = reinterpret_cast<double *>(rec + rl.leaf_bb());
        int *wall_shape = reinterpret_cast<int *>(rec + rl.wall_shape()), *pair_age = reinterpret_cast<int *>(rec + rl.pair_age());
        for (int i = 0; i < A; i++) {
            // Entity.__init__ + space.add: caches and BBTree leaf at the start position, v = 0
            const double x = start[2 * i], y = start[2 * i + 1], r = cfg->agent_radius;
            pos[2 * i] = x; pos[2 * i + 1] = y;
            tc[2 * i] = x; tc[2 * i + 1] = y;
            const double l = x - r, b = y - r, rr = x + r, t = y + r;
            const double mx = (rr - l) * 0.1, my = (t - b) * 0.1;
            double *lf = leaf + 4 * i;
            lf[0] = l + (-mx < 0.0 ? -mx : 0.0); lf[1] = b + (-my < 0.0 ? -my : 0.0);
            lf[2] = rr + (mx > 0.0 ? mx : 0.0); lf[3] = t + (my > 0.0 ? my : 0.0);
        }
        for (int q = 0; q < A * kK; q++) wall_shape[q] = -1;   // free slots
        for (int q = 0; q < rl.NPs; q++) pair_age[q] = -1;      // none
    }
}

// ---- spatial-hash grids, one GridHost per map (cell size: Knobs::grid_cell px, default 4 ... while the table fits); a map's longest candidate
//      list decides which form of the ray fan can serve it
static void plan_map_grids(const cat_config *cfg, const cat_tables *tab, const SimPlan &plan, std::vector<GridHost> &map_grid)
{
    // Cell size: the smaller the cell, the tighter the three listing rules (agh-map, entries per ray: 16 px 2.1, 8 px 1.56, 4 px 1.35,
    // 2 px: kernel 64.6 -> 63.2 us for four times the table) and the larger the table (rows of 4 - 8 B per cell and ray: labyrinth
    // 48 MB, agh-map 98 MB at 4 px).  4 px while a map's table stays under 384 MB, else 8, 16 ...; Knobs::grid_cell fixes it.
    const int n_maps = plan.n_maps;
    const double reach = cfg->ray_length + cfg->ray_radius + 1e-3;
    map_grid.assign((size_t)n_maps, GridHost());
    for (int m = 0; m < n_maps; m++) {
        const MapDesc &md = plan.descs[m];
        const double *bbm = plan.geo_f.data() + md.f64_off;
        const int *hulls = plan.geo_i.data() + md.i32_off;
        double cell = plan.knobs.grid_cell;
        if (cell == 0.0) {
            double lo[2] = {1e300, 1e300}, hi[2] = {-1e300, -1e300};
            for (int sidx = 0; sidx < md.S; sidx++) {
                lo[0] = std::fmin(lo[0], bbm[4 * sidx]); lo[1] = std::fmin(lo[1], bbm[4 * sidx + 1]);
                hi[0] = std::fmax(hi[0], bbm[4 * sidx + 2]); hi[1] = std::fmax(hi[1], bbm[4 * sidx + 3]);
            }
            for (cell = 4.0; cell < 256.0; cell *= 2.0) {
                const double rows = std::ceil((hi[0] - lo[0] + 2.0 * reach) / cell + 2.0) * std::ceil((hi[1] - lo[1] + 2.0 * reach) / cell + 2.0) * cfg->n_rays;
                // eight bytes per row unless a map's lists need the wide byte format; a sim of several maps shares the budget of two
                if (rows * 8.0 <= 384e6 * std::fmin(1.0, 2.0 / n_maps)) break;
            }
        }
        build_grids(bbm, md.S, cfg->n_rays, tab->ray_dx, tab->ray_dy, reach, cfg->bbtree_gate != 0, cfg->ray_radius + 2e-6, cell, map_grid[(size_t)m],
                    hulls, hulls + md.S, cfg->wall_radius + cfg->ray_radius, cfg->ray_radius, plan.tree, plan.knobs.grid_hulls, plan.knobs.grid_occlusion);
    }
}

// ---- parts: the maps whose rays meet few walls (every candidate list fits a four-byte row -- the labyrinth's six walls of 5 bits --; shape ids and agents
//      fit 6 bits; an agent's rays fit four chunks) take the GROUP form of the ray fan (and its pooled kernels where the ring fits the LDS), every other map
//      the CHUNK form.  A sim whose maps want both runs in ONE part on the chunk form by default; Knobs::split cuts it in two parts -- each with its own
//      candidate tables, LDS carve, workgroup size, work list and kernels -- that every entry launches side by side on two streams.  Measured (round 5, five
//      maps x16384, us per tick one part -> two parts): one launch per tick 167.8 -> 185.6 (the two kernels do overlap -- 130 and 170 us inside a 182 us period by
//      the trace -- but a mixed batch costs the SUM of its workgroups' times either way, the pooled one-tick kernel gains + 1 - 2 % on three of the four box maps and
//      loses 4 % on lbirinth, and the fork / join events add 14 us between launches); resident T = 64 128.7 -> 127.8.  So the split is kept as a tested option, not
//      the default.  Knobs::fan_chunks forces the chunk form everywhere; tree order is carried by the chunk form only (whatever the knobs say).
static void split_parts(const cat_config *cfg, const std::vector<GridHost> &map_grid, SimPlan &plan)
{
    const int A = plan.base.A;
    const bool chunks_only = plan.knobs.fan_chunks || plan.tree;
    std::vector<int> light, dense;
    for (int m = 0; m < plan.n_maps; m++) (map_grid[(size_t)m].max_row <= 7 && cfg->n_rays <= kGroupRays && !chunks_only ? light : dense).push_back(m);
    if (!light.empty()) {   // the four-byte row must hold the longest list of the part in fields of the part's id width
        int S_l = 0, row_l = 0, idb = 1;
        for (int m : light) { S_l = std::max(S_l, plan.descs[m].S); row_l = std::max(row_l, map_grid[(size_t)m].max_row); }
        while ((1 << idb) <= S_l) idb++;
        if (!(row_l * idb <= 32 && S_l + A <= 63)) { dense.insert(dense.end(), light.begin(), light.end()); light.clear(); }
    }
    if (!light.empty() && !dense.empty() && !plan.knobs.split) { dense.insert(dense.end(), light.begin(), light.end()); light.clear(); }
    std::sort(dense.begin(), dense.end());
    auto add = [&](const std::vector<int> &maps, int fan) {
        if (maps.empty()) return;
        plan.parts.emplace_back();
        plan.parts.back().map_ids = maps;
        plan.parts.back().fan = fan;
    };
    add(light, 1);
    add(dense, 0);
}

// waves (= env slots) per workgroup.  Most resident waves per CU first (cap 16 = 4 per SIMD at <= 128 VGPRs); among equals a launch of at most two rounds
// takes the LARGEST workgroup (its waves share ray chunks, which removes the lone-wave tail of a single round), a longer launch the SMALLEST (workgroups
// of a CU overlap each other's drain).  forced (Knobs::waves_per_block) overrides (tuning): any size that fits, also not a power of two.  0: nothing fits.
static int choose_wpb(const LdsSizes &ls, int N, int forced)
{
    const int cu = 256;
    if (forced >= 1 && forced <= kMaxWaves && ls.total(forced) <= kLdsBytes) return forced;
    int best_score = -1, best_w = 0;
    for (int w = 1; w <= kMaxWaves; w *= 2) {
        const size_t bytes = ls.total(w);
        if (bytes > kLdsBytes) continue;
        int resident = (int)(kLdsBytes / bytes) * w;
        if (resident > 16) resident = 16;
        const bool small_launch = (long long)N <= 2LL * 16 * cu;
        if (resident > best_score || (resident == best_score && small_launch)) { best_score = resident; best_w = w; }
    }
    return best_w;
}

// share of the part's (cell, ray) rows without a candidate, sampled where episodes start: five points of every spawn region (the JSON start position of
// an agent without regions), every ray
static double sample_empty_rows(const SimPlan &plan, const PartPlan &pt)
{
    const int R = plan.base.R;
    size_t n_rows = 0, n_empty = 0;
    for (size_t k = 0; k < pt.grid.desc.size(); k++) {
        const MapDesc &md = plan.descs[pt.map_ids[k]];
        const GridDesc &gd = pt.grid.desc[k];
        const double *start = plan.geo_f.data() + md.f64_off + 4 * md.S + geo_rest_doubles(md), *regions = start + 2 * md.A;
        const int *region_off = plan.geo_i.data() + md.i32_off + 2 * md.S;
        auto sample = [&](double x, double y) {
            const int cx = (int)floor((x - gd.x0) * gd.inv_cell), cy = (int)floor((y - gd.y0) * gd.inv_cell);
            if (cx < 0 || cy < 0 || cx >= gd.nx || cy >= gd.ny) return;
            const size_t r0 = (size_t)gd.off_base + ((size_t)cy * gd.nx + cx) * R;
            for (int k2 = 0; k2 < R; k2++) { n_rows++; n_empty += pt.grid.off[r0 + k2 + 1] == pt.grid.off[r0 + k2]; }
        };
        for (int i = 0; i < md.A; i++) {
            const int r0 = region_off[i], nr = region_off[i + 1] - r0;
            if (nr <= 0) { sample(start[2 * i], start[2 * i + 1]); continue; }
            for (int q = 0; q < nr; q++) {
                const double *rg = regions + 4 * (r0 + q);
                sample(rg[0] + rg[2] / 2, rg[1] + rg[3] / 2);
                for (int c = 0; c < 4; c++) sample(rg[0] + rg[2] * ((c & 1) ? 0.75 : 0.25), rg[1] + rg[3] * ((c & 2) ? 0.75 : 0.25));
            }
        }
    }
    return n_rows ? (double)n_empty / (double)n_rows : 0.0;
}

// One part: row format, LDS carve and workgroup size, chunks per work unit, the ray ring, the work list, the parameter block's scalars, the kernels.
// map_grid: the tables of every map of the sim (the part takes its maps').
static int plan_part(const cat_config *cfg, SimPlan &plan, PartPlan &pt, std::vector<GridHost> &map_grid, const std::vector<int> &wall_depth, char *err)
{
    const Knobs &knobs = plan.knobs;
    const Params &base = plan.base;
    const int A = base.A, N = base.N, R = base.R, n_maps = plan.n_maps, fan = pt.fan;
    int maxS = 0, maxP = 0, maxPP = 0;
    std::vector<int> local_of((size_t)n_maps, -1);   // map -> its index among the part's grids
    for (size_t k = 0; k < pt.map_ids.size(); k++) {
        const int m = pt.map_ids[k];
        const MapDesc &md = plan.descs[m];
        local_of[(size_t)m] = (int)k;
        maxS = std::max(maxS, md.S); maxP = std::max(maxP, md.P); maxPP = std::max(maxPP, md.PP);
        pt.wall_depth = std::max(pt.wall_depth, wall_depth[(size_t)m]);
        pt.map_max_row.push_back(map_grid[(size_t)m].max_row);
        append_grid(pt.grid, map_grid[(size_t)m]);
        map_grid[(size_t)m] = GridHost();   // the part owns the tables now
    }
    for (int e = 0; e < N; e++) pt.n_envs += local_of[(size_t)plan.slot[e]] >= 0;
    GridHost &grid = pt.grid;
    int id_bits = 1;   // bits of a wall id + 1
    while ((1 << id_bits) <= maxS) id_bits++;
    // the group form reads four-byte rows; the chunk form eight-byte rows of the same fields where the longest list fits
    // (agh-map: 9 walls of 7 bits), else byte rows of 8 / 16 / 32 bytes with the CSR continuation (Knobs::grid_fields = false forces those)
    const bool wide = fan == 0 && grid.max_row * id_bits <= 64 && knobs.grid_fields;
    finalize_rows(grid, (fan == 1 || wide) ? id_bits : 0, wide);
    // the CSR arrays of the ray grid are only read for lists beyond a row's capacity: not uploaded when no list is that long
    pt.csr = !grid.id_bits && grid.max_row > 8 * grid.row_words - 1;
    // the contact array of a scratch union: what the part's maps make possible (an agent's bb overlaps at most `wall_depth` wall bbs at once -- 2 on the box
    // maps, 5 on agh-map -- and holds at most CAT_WALL_CACHE arbiters), + every agent pair; lane q solves contact q, so never more than a wave's lanes
    const int maxc = std::min(kLanes, A * std::min(pt.wall_depth, kK) + base.NP);
    // ---- LDS carve sizes (must match carve()) and the workgroup size
    LdsSizes ls = lds_sizes(A, R, maxS, maxP, maxPP, fan == 1, maxc, knobs.env_pad);
    const int wpb = choose_wpb(ls, N, knobs.waves_per_block);
    if (wpb == 0) PLAN_FAIL(CAT_ERR_BAD_CONFIG, "LDS budget exceeded: %zu bytes for one env slot", ls.total(1));
    // ---- the kernels of the chunk form are known here (no ring); those of the group form once the ring is decided
    const bool generic = knobs.generic_kernel;
    if (fan == 0) pt.kernels = select_kernels(KernelQuery{A, R, base.n_cops, fan, false, false, false, plan.tree, generic});
    // ---- chunk form: several chunks of a slot per work unit with one item list (fan_slot), where the kernels carry it (fixed dimensions at 64 rays), the rows
    //      are one word of id fields, ids fit seven bits and the LDS left beside the env areas gives every wave's scratch union a list of at least 160 items
    //      (agh-map 2v1: 240 = the 17 KB that are free)
    int item_cap = 0;
    for (GridDesc &d : grid.desc) d.span = d.span_tick = 1;
    const int nch = A * ((R + kLanes - 1) / kLanes);
    if (fan == 0 && pt.kernels.carries_slot && wide && grid.row_words == 1 && maxS + A <= 127 && nch >= 2 && grid.max_row + A - 1 <= 15) {
#ifdef CAT_PHASE_TIMING
        const size_t budget = kLdsBytes - 4096;   // (the diagnostic build keeps its cycle accumulators in static LDS)
#else
        const size_t budget = kLdsBytes;
#endif
        const size_t spare = ls.total(wpb) < budget ? (budget - ls.total(wpb)) / (size_t)wpb : 0;
        int cap = (int)(((size_t)ls.uni + spare) / 18) & ~7;
        if (cap > 768) cap = 768;
        if (knobs.item_cap_set && knobs.item_cap >= 16 && knobs.item_cap <= cap) cap = knobs.item_cap & ~7;   // tests: lists too short for the chunks of a slot
        if (cap >= 160 || knobs.item_cap_set) {
            item_cap = cap;
            const int need = (18 * cap + 15) / 16 * 16;
            if (need > ls.uni) ls.uni = need;
        }
    }
    // How many chunks share a unit, per map: as many as (mostly) fit the list in one turn.  Measured on the dense map (agh-map 2v1 x4096, 86 candidates
    // per chunk before the gate, list of 240; us per tick one-tick / resident): 1 chunk per unit 63.8 / 47.3, 2 chunks 61.2 / 45.2, 3 chunks 65.3 / 49.0 -- three
    // chunks do not fit together, the third is traced in a second turn and the unit is one long serial job; the box maps' rays meet few walls (three chunks
    // = ~120 items): five maps x16384 172.5 / 132.1 -> 164.3 / 126.6 with three.  Knobs::slot_chunks / slot_chunks_tick override (every map).
    for (size_t k = 0; k < grid.desc.size() && item_cap; k++) {
        const int want = pt.map_max_row[k] <= 7 ? 3 : 2;
        auto chunks = [&](int knob) { return knob >= 1 && knob <= kSlotChunks ? std::min(knob, nch) : std::min(want, nch); };
        grid.desc[k].span = chunks(knobs.slot_chunks);
        grid.desc[k].span_tick = chunks(knobs.slot_chunks_tick);
    }
    // ---- the workgroup's ray pool (step_kernel_pooled / rollout_kernel_pooled): a ring of wpb * A * R eight-byte entries beside the env areas, where it fits
    // Where the ring fits, the RESIDENT launch always runs pooled (whole runs from the reset, tools/pool_soak.py, M env-steps/s unit -> pooled: labyrinth 201 -> 229,
    // labyrinth-inside 148 -> 159, squarinth 156 -> 169, grandbyrinth 154 -> 169, lbirinth 123.0 -> 123.6).  The ONE-TICK launch pays the sorting pass in its serial
    // chain and loses on a map whose rays all meet a wall (lbirinth 90.5 -> 87.0; labyrinth 132.5 -> 139.1, the others + 1 - 2 %): it runs pooled unless practically no
    // (cell, ray) row sampled around the spawn points is empty (lbirinth 0.008; labyrinth-inside 0.06, squarinth 0.22, grandbyrinth 0.27, labyrinth 0.41)
    // ... and on rosters of at most four agents: the pooled one-tick launch keeps the whole sorting pass in the slot's serial front, which grows with the roster
    // (3v2 at 64 rays x8192, round 5: 97.4 us unit form, 99.0 pooled; resident 77.6 -> 74.8 us per tick: the resident launch takes the ring whenever it exists).
    // Knobs::pool = 1 / 0 forces both / neither.
    pt.empty_rows = sample_empty_rows(plan, pt);
    const bool pool_forced = knobs.pool >= 0;
    const bool want_ring = pool_forced ? knobs.pool != 0 : true;
    bool pool_step = pool_forced ? knobs.pool != 0 : (pt.empty_rows >= kPoolEmptyRows && A <= 4);
    int pool_cap = 0, grp_rays = 4 * kLanes;
    if (fan == 1 && want_ring) {
        // capacity: the next power of two (ring position by a mask), else wpb * A * R + 64 entries exactly (position by an invariant division); group
        // arrays of the scratch unions: what group_agents() holds at once (two agents up to 128 rays each), else one agent's chunks
        int cap2 = 64;
        while (cap2 < wpb * A * R) cap2 *= 2;
        const int cap_x = (wpb * A * R + 64 + 1) / 2 * 2;
        const int cpa = (R + 63) / 64, gsz = cpa <= 2 ? 2 : 1;
        const int g_full = kLanes * std::min(4, std::min(A, gsz) * cpa), g_one = kLanes * std::min(4, cpa);
        const bool ok_dims = A <= 8 && R <= 256 && wpb <= 16 && cpa <= 4;
        // While the one-tick launch stays on the unit form, the ring may not take the group arrays below what that kernel's units want (rosters whose rays
        // fill more than four chunks: as many agents as fill four -- group_agents_resident).  3v2 at 64 rays x8192, round 5: with the ring (units of
        // 2 + 2 + 1 agents in the one-tick launch instead of 4 + 1) 102.5 us one-tick / 75.2 resident, without 95.9 - 97.4 / 76.1 - 77.6: the one-tick launch
        // is the one this library is measured on, so the ring stays out (Knobs::pool = 1 brings it in: both entries pooled).
        const int g_want = (!pool_step && !pool_forced && A * cpa > 4) ? kLanes * 4 : 0;
        for (int attempt = 0; ok_dims && attempt < 3 && !pool_cap; attempt++) {
            const int cap = attempt == 0 ? cap2 : cap_x, g2 = std::max(attempt < 2 ? g_full : g_one, g_want);
            const LdsSizes l2 = lds_sizes(A, R, maxS, maxP, maxPP, true, maxc, knobs.env_pad, g2);
            if (l2.total(wpb) + 16 + (size_t)cap * 8 <= kLdsBytes) { pool_cap = cap; grp_rays = g2; ls = l2; }
        }
    }
    if (!pool_cap) pool_step = false;
    pt.pool_cap = pool_cap;
    pt.pool_step = pool_step;
    // ---- work list: workgroups are map-homogeneous; env slots grouped by map, padded with -1
    const int helpers = knobs.helpers < 0 || knobs.helpers >= wpb ? 0 : knobs.helpers;   // that many waves of every workgroup own no env slot and only take work units
    const int epb = wpb - helpers;
    for (int m : pt.map_ids) {
        int cnt = 0;
        for (int e = 0; e < N; e++)
            if (plan.slot[e] == m) {
                if (cnt % wpb == 0) pt.block_map.push_back(m);
                pt.work.push_back(e);
                cnt++;
                if (cnt % wpb == epb) for (int h = 0; h < helpers; h++) { pt.work.push_back(-1); cnt++; }
            }
        while (cnt % wpb) { pt.work.push_back(-1); cnt++; }
    }
    pt.n_blocks = (int)pt.block_map.size();
    pt.block_desc.assign(pt.block_map.size(), BlockDesc{});
    for (size_t b = 0; b < pt.block_map.size(); b++) {
        pt.block_desc[b].md = plan.descs[pt.block_map[b]];
        pt.block_desc[b].gd = grid.desc[(size_t)local_of[(size_t)pt.block_map[b]]];
    }
    pt.uniform = n_maps == 1 && (int)pt.work.size() == pt.n_blocks * wpb;
    for (size_t k = 0; pt.uniform && k < pt.work.size(); k++) pt.uniform = pt.work[k] == ((int)k < N ? (int)k : -1);
    // ---- the parameter block
    Params &p = pt.p;
    p = base;
    p.maxc = maxc;
    p.row_words = grid.row_words;
    p.row_id_bits = grid.id_bits;
    if (p.row_id_bits) {
        p.row_cnt_mul = (65536 + p.row_id_bits - 1) / p.row_id_bits;
        for (int b = 0; b < 64; b++)
            if (((b * p.row_cnt_mul) >> 16) != b / p.row_id_bits) PLAN_FAIL(CAT_ERR_BAD_CONFIG, "row field divider");
    }
    p.maxE = maxS + A;
    p.lds_map_bytes = ls.map; p.lds_env_bytes = ls.env; p.lds_union_bytes = ls.uni; p.wpb = wpb;
    p.lds_racc_off = ls.racc;
    p.lds_o16_off = ls.o16;
    p.grp_rays = grp_rays;
    p.item_cap = item_cap;
    p.lds_pool_off = pool_cap ? (int)((ls.total(wpb) + 15) / 16 * 16) : 0;
    p.pool_mask = pool_cap ? pool_cap - 1 : 0;
    p.pool_magic = 0u; p.pool_shift = -1;
    if (pool_cap && (pool_cap & (pool_cap - 1))) {   // not a power of two: floor(i / cap) = (t + ((i - t) >> 1)) >> shift with t = mulhi(magic, i)  [Granlund & Montgomery]
        int l = 0;
        while ((1u << l) < (unsigned)pool_cap) l++;
        p.pool_magic = (unsigned)((((unsigned long long)1 << 32) * ((1ull << l) - (unsigned long long)pool_cap)) / (unsigned long long)pool_cap + 1ull);
        p.pool_shift = l - 1;
    }
    pt.wpb = wpb;
    pt.lds = ls;
    pt.lds_bytes = pool_cap ? (size_t)p.lds_pool_off + (size_t)pool_cap * 8 : ls.total(wpb);
    if (fan == 1) pt.kernels = select_kernels(KernelQuery{A, R, base.n_cops, fan, pool_cap != 0, pool_step, p.pool_shift >= 0, plan.tree, generic});
    return CAT_OK;
}

// Everything cat_create decides and uploads for these arguments and this environment, without touching a device.  err: kErrBytes.
static int plan_sim(const cat_config *cfg, const cat_tables *tab, const void *const *blobs, const size_t *sizes, int n_maps, const int32_t *slot_map_ids,
                    SimPlan &plan, char *err)
{
    plan.knobs = read_knobs();
    plan.n_maps = n_maps;
    plan.tree = cfg->bbtree_gate == CAT_GATE_TREE;
    const int A = cfg->n_cops + cfg->n_thieves, N = cfg->n_envs;
    std::vector<int> wall_depth;   // per map: the most wall bbs one agent's bb can overlap at once (max_wall_bb_depth)
    if (const int rc = plan_geometry(cfg, blobs, sizes, n_maps, plan, wall_depth, err)) return rc;
    if (plan.tree) { if (const int rc = plan_trees(plan, err)) return rc; }
    plan.slot.assign((size_t)N, 0);
    for (int e = 0; e < N; e++) {
        if (slot_map_ids) plan.slot[e] = slot_map_ids[e];
        if (plan.slot[e] < 0 || plan.slot[e] >= n_maps) PLAN_FAIL(CAT_ERR_BAD_SLOT_MAP, "slot_map_ids[%d]=%d out of range", e, plan.slot[e]);
    }
    std::vector<GridHost> map_grid;
    plan_map_grids(cfg, tab, plan, map_grid);
    // ---- what every part shares: the configuration, the record layout, the ray table's cone parameters
    Params &base = plan.base;
    memset(&base, 0, sizeof base);
    base.N = N; base.A = A; base.n_cops = cfg->n_cops; base.R = cfg->n_rays; base.max_step = cfg->max_step_count;
    base.iterations = cfg->iterations; base.persistence = cfg->persistence; base.gate = cfg->bbtree_gate;
    base.NP = A * (A - 1) / 2;
    base.env_id_offset = cfg->env_id_offset; base.seed = cfg->seed;
    base.dt = cfg->dt; base.bias_coef = cfg->bias_coef; base.slop = cfg->slop; base.ray_length = cfg->ray_length;
    base.ray_radius = cfg->ray_radius; base.rc = cfg->agent_radius; base.mass = cfg->agent_mass; base.impulse = cfg->impulse;
    base.max_speed = cfg->max_speed; base.term_radius = cfg->termination_radius; base.wall_r = cfg->wall_radius;
    base.term_d2 = radius_lt_threshold(base.term_radius); base.near_d2 = radius_le_threshold(base.rc, base.ray_radius);
    base.hot_bytes = RecLayout(A).hot_bytes();
    base.rec_bytes = RecLayout(A).rec_bytes();
    if (base.hot_bytes > kLanes * 16) PLAN_FAIL(CAT_ERR_BAD_CONFIG, "state record of %d bytes exceeds the kernels' register staging", base.hot_bytes);   // StateRegs
    split_parts(cfg, map_grid, plan);
    plan_initial_records(cfg, plan);
    {   // ray-direction cone parameters: valid when the table is a uniform full circle
        const double two_pi = 6.283185307179586;
        const double a0 = atan2(tab->ray_dy[0], tab->ray_dx[0]);
        const double step = two_pi / base.R;
        bool ok = base.R >= 4;
        for (int k = 0; k < base.R && ok; k++) {
            double d = atan2(tab->ray_dy[k], tab->ray_dx[k]) - (a0 + k * step);
            d -= two_pi * floor(d / two_pi + 0.5);
            if (fabs(d) > 1e-6) ok = false;
        }
        base.ang_ok = ok ? 1 : 0;  // otherwise every shape is paired with every ray (still exact)
        base.ang0 = (float)a0;
        base.inv_step = (float)(1.0 / step);
    }
    for (PartPlan &pt : plan.parts)
        if (const int rc = plan_part(cfg, plan, pt, map_grid, wall_depth, err)) return rc;
    return CAT_OK;
}

// ---------------------------------------------------------------------- the plan as text ----
static unsigned long long fnv1a64(const void *data, size_t n)
{
    unsigned long long h = 14695981039346656037ull;
    const unsigned char *b = static_cast<const unsigned char *>(data);
    for (size_t i = 0; i < n; i++) { h ^= b[i]; h *= 1099511628211ull; }
    return h;
}
struct PlanText {
    std::string s;
    void kv(const std::string &scope, const char *key, const char *fmt, ...)
    {
        char v[512];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(v, sizeof v, fmt, ap);
        va_end(ap);
        s += scope; s += '.'; s += key; s += '='; s += v; s += '\n';
    }
    // FNV-1a 64 of the bytes of an upload: `count` elements at `data`, or that many zero bytes where the device array is only cleared (data == null)
    void hash(const std::string &scope, const char *key, const void *data, size_t count, size_t elem)
    {
        std::vector<unsigned char> zero;
        if (!data) { zero.assign(count * elem, 0); data = zero.data(); }
        kv(scope, key, "%016llx", fnv1a64(data, count * elem));
    }
    template <class T> void hash(const std::string &scope, const char *key, const std::vector<T> &v) { hash(scope, key, v.data(), v.size(), sizeof(T)); }
};

// key=value lines: every decision of the plan and an FNV-1a 64 hash of every table it uploads (what cat_create prints under CAT_VERBOSE,
// what cat_plan_describe_host returns, what tests/golden/plan pins)
static std::string describe_plan(const SimPlan &plan)
{
    PlanText o;
    const Params &b = plan.base;
    o.kv("sim", "N", "%d", b.N); o.kv("sim", "A", "%d", b.A); o.kv("sim", "n_cops", "%d", b.n_cops); o.kv("sim", "R", "%d", b.R);
    o.kv("sim", "gate", "%d", b.gate); o.kv("sim", "NP", "%d", b.NP); o.kv("sim", "rec_bytes", "%d", b.rec_bytes); o.kv("sim", "hot_bytes", "%d", b.hot_bytes);
    o.kv("sim", "ang_ok", "%d", b.ang_ok); o.kv("sim", "ang0", "%a", (double)b.ang0); o.kv("sim", "inv_step", "%a", (double)b.inv_step);
    o.kv("sim", "n_maps", "%d", plan.n_maps); o.kv("sim", "n_parts", "%zu", plan.parts.size());
    o.hash("sim.hash", "geo_f64", plan.geo_f);
    o.hash("sim.hash", "geo_i32", plan.geo_i);
    o.hash("sim.hash", "maps", plan.descs);
    o.hash("sim.hash", "state", plan.rec0);
    if (plan.tree) { o.hash("sim.hash", "tree_bb", plan.tree_bb); o.hash("sim.hash", "tree_link", plan.tree_link); o.hash("sim.hash", "tree_root", plan.tree_root); }
    else { o.kv("sim.hash", "tree_bb", "-"); o.kv("sim.hash", "tree_link", "-"); o.kv("sim.hash", "tree_root", "-"); }
    for (size_t pi = 0; pi < plan.parts.size(); pi++) {
        const PartPlan &pt = plan.parts[pi];
        const Params &p = pt.p;
        const std::string sc = "part" + std::to_string(pi), hs = sc + ".hash";
        std::string ids;
        for (size_t k = 0; k < pt.map_ids.size(); k++) ids += (k ? "," : "") + std::to_string(pt.map_ids[k]);
        o.kv(sc, "fan", "%s", pt.fan ? "group" : "chunk");
        o.kv(sc, "map_ids", "%s", ids.c_str());
        o.kv(sc, "n_envs", "%d", pt.n_envs);
        o.kv(sc, "n_blocks", "%d", pt.n_blocks);
        o.kv(sc, "wpb", "%d", pt.wpb);
        o.kv(sc, "lds_bytes", "%zu", pt.lds_bytes);
        o.kv(sc, "lds_map", "%d", p.lds_map_bytes);
        o.kv(sc, "lds_env", "%d", p.lds_env_bytes);
        o.kv(sc, "lds_union", "%d", p.lds_union_bytes);
        o.kv(sc, "lds_racc", "%d", p.lds_racc_off);
        o.kv(sc, "lds_pool_off", "%d", p.lds_pool_off);
        o.kv(sc, "wall_bb_depth", "%d", pt.wall_depth);
        o.kv(sc, "maxc", "%d", p.maxc);
        o.kv(sc, "maxE", "%d", p.maxE);
        o.kv(sc, "grp_rays", "%d", p.grp_rays);
        o.kv(sc, "item_cap", "%d", p.item_cap);
        o.kv(sc, "empty_rows", "%.6f", pt.empty_rows);
        o.kv(sc, "pool_mask", "%d", p.pool_mask);
        o.kv(sc, "pool_magic", "%u", p.pool_magic);
        o.kv(sc, "pool_shift", "%d", p.pool_shift);
        o.kv(sc, "pool_step", "%d", pt.pool_step ? 1 : 0);
        o.kv(sc, "row_words", "%d", p.row_words);
        o.kv(sc, "row_id_bits", "%d", p.row_id_bits);
        o.kv(sc, "row_cnt_mul", "%d", p.row_cnt_mul);
        o.kv(sc, "csr", "%d", pt.csr ? 1 : 0);
        o.kv(sc, "kernel_variant", "%s", pt.kernels.variant.c_str());
        o.kv(sc, "one_tick_kernel", "%s", pt.pool_step ? "step_kernel_pooled" : "step_kernel");
        o.kv(sc, "rollout_kernel", "%s", pt.pool_cap ? "rollout_kernel_pooled" : "rollout_kernel");
        o.kv(sc, "uniform", "%d", pt.uniform ? 1 : 0);
        for (size_t k = 0; k < pt.map_ids.size(); k++) {
            const GridDesc &gd = pt.grid.desc[k];
            const std::string ms = sc + ".map" + std::to_string(pt.map_ids[k]);
            o.kv(ms, "nx", "%d", gd.nx);
            o.kv(ms, "ny", "%d", gd.ny);
            o.kv(ms, "inv_cell", "%a", gd.inv_cell);
            o.kv(ms, "span", "%d", gd.span);
            o.kv(ms, "span_tick", "%d", gd.span_tick);
            o.kv(ms, "max_row", "%d", pt.map_max_row[k]);
        }
        o.hash(hs, "grids", pt.grid.desc);
        o.hash(hs, "grid_rows", pt.grid.rows);
        if (pt.csr) { o.hash(hs, "grid_off", pt.grid.off); o.hash(hs, "grid_ent", pt.grid.ent); }
        else { o.hash(hs, "grid_off", nullptr, 1, sizeof(int)); o.hash(hs, "grid_ent", nullptr, 1, 1); }
        o.hash(hs, "cgrid_off", pt.grid.coff);
        o.hash(hs, "cgrid_ent", pt.grid.cent);
        o.hash(hs, "cgrid_rows", pt.grid.crows);
        o.hash(hs, "work_env", pt.work);
        o.hash(hs, "block_map", pt.block_map);
        o.hash(hs, "block_desc", pt.block_desc);
    }
    return o.s;
}

// Host-only: the plan of a sim as text, without a device (include/cat_sim.h).
extern "C" int cat_plan_describe_host(const cat_config *cfg, const cat_tables *tab, const void *const *blobs, const size_t *sizes, int n_maps,
                                      const int32_t *slot_map_ids, char *buf, size_t cap)
{
    if (const int rc = check_create_args(cfg, tab, blobs, sizes, n_maps, true, g_create_err)) return rc;
    SimPlan plan;
    if (const int rc = plan_sim(cfg, tab, blobs, sizes, n_maps, slot_map_ids, plan, g_create_err)) return rc;
    const std::string text = describe_plan(plan);
    if (buf && cap) {
        const size_t n = std::min(text.size(), cap - 1);
        memcpy(buf, text.data(), n);
        buf[n] = 0;
    }
    return (int)text.size();
}
