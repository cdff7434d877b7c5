// cat_sim_grid.h -- part of the env core's single translation unit (included by cat_sim.hip, in this order; not a stand-alone header):
// host side, no device needed: the environment knobs, the map-blob reader, the spatial-hash candidate tables, Chipmunk's static tree, the wall-overlap
// bound and the host-only C-ABI entries built on them.  No HIP runtime call in this file.
// ====================================================================== host side ============
// ---------------------------------------------------------------------- environment knobs ----
// Every knob cat_create obeys (tuning / tests only; INTEGRATION.md lists the same names), read from the environment in ONE place: read_knobs().
struct Knobs {
    bool verbose = false;                   // CAT_VERBOSE (set at all): cat_create prints the plan (describe_plan)
    bool generic_kernel = false;            // CAT_GENERIC_KERNEL=1: no compile-time roster
    bool fan_chunks = false;                // CAT_FAN=chunks: the chunk form of the ray fan everywhere
    bool split = false;                     // CAT_SPLIT=1: a sim whose maps want both forms of the fan runs in two parts
    int pool = -1;                          // CAT_POOL=1 / 0: both entries pooled / neither (-1: unset, cat_create chooses per entry)
    int waves_per_block = 0;                // CAT_WAVES_PER_BLOCK
    int slot_chunks = 0;                    // CAT_SLOT_CHUNKS: chunks per work unit of the chunk form, resident launch (0: per map) ...
    int slot_chunks_tick = 0;               // CAT_SLOT_CHUNKS_TICK: ... and one-tick launch
    bool item_cap_set = false;              // CAT_ITEM_CAP (set at all: the unit's item list is taken however short) ...
    int item_cap = 0;                       // ... and its value
    bool env_pad = true;                    // CAT_ENV_PAD=0: no bank-spreading pad of the env areas
    int helpers = 0;                        // CAT_HELPERS (diagnostic): waves of every workgroup that own no env slot
    double grid_cell = 0.0;                 // CAT_GRID_CELL: spatial-hash cell in px, 2 .. 512 (0: by the size of the table)
    bool grid_fields = true;                // CAT_GRID_FIELDS=0: the chunk form reads byte rows, never rows of id fields
    bool grid_hulls = true;                 // CAT_GRID_HULLS=0: candidate table without its hull rule ...
    bool grid_occlusion = true;             // CAT_GRID_OCCLUSION=0: ... without its occlusion rule
    bool allow_deep_wall_overlap = false;   // CAT_ALLOW_DEEP_WALL_OVERLAP=1: accept a map on which an agent's bb can overlap more than CAT_WALL_CACHE wall bbs
};
static Knobs read_knobs()
{
    Knobs k;
    auto num = [](const char *name, int unset) { const char *e = getenv(name); return e ? atoi(e) : unset; };
    k.verbose = getenv("CAT_VERBOSE") != nullptr;
    k.generic_kernel = num("CAT_GENERIC_KERNEL", 0) != 0;
    if (const char *e = getenv("CAT_FAN")) k.fan_chunks = !strcmp(e, "chunks");
    k.split = num("CAT_SPLIT", 0) != 0;
    if (getenv("CAT_POOL")) k.pool = num("CAT_POOL", 0) != 0 ? 1 : 0;
    k.waves_per_block = num("CAT_WAVES_PER_BLOCK", 0);
    k.slot_chunks = num("CAT_SLOT_CHUNKS", 0);
    k.slot_chunks_tick = num("CAT_SLOT_CHUNKS_TICK", 0);
    k.item_cap_set = getenv("CAT_ITEM_CAP") != nullptr;
    k.item_cap = num("CAT_ITEM_CAP", 0);
    k.env_pad = num("CAT_ENV_PAD", 1) != 0;
    k.helpers = num("CAT_HELPERS", 0);
    if (const char *e = getenv("CAT_GRID_CELL")) { const double v = atof(e); if (v >= 2.0 && v <= 512.0) k.grid_cell = v; }
    k.grid_fields = num("CAT_GRID_FIELDS", 1) != 0;
    k.grid_hulls = num("CAT_GRID_HULLS", 1) != 0;
    k.grid_occlusion = num("CAT_GRID_OCCLUSION", 1) != 0;
    k.allow_deep_wall_overlap = num("CAT_ALLOW_DEEP_WALL_OVERLAP", 0) != 0;
    return k;
}

// ---------------------------------------------------------------------- map blobs ----
// One map as the caller hands it over (CompiledMap.to_blob): a 64-byte header of int32 -- magic, version, S walls, P planes, A agents, cops, thieves,
// regions -- then the f64 section [window 2][bb 4 S][planes 8 P][start 2 A][regions 4 Rg] and the i32 section [first plane S][plane count S][region_off A + 1].
// The one reader of that layout: it accepts a whole blob only (magic, version, exact size, 1 <= S <= CAT_MAX_SHAPES) and copies the two sections out
// (a caller's bytes need not be aligned).  Whether the roster fits a sim is the planner's own question.
struct MapBlob {
    int S = 0, P = 0, A = 0, n_cops = 0, n_regions = 0;
    std::vector<double> f;   // the f64 section
    std::vector<int> iv;     // the i32 section
    const double *bb() const { return f.data() + 2; }
    size_t n_geo() const { return 4 * (size_t)S + 8 * (size_t)P; }   // doubles of [bb][planes]
    const double *planes() const { return bb() + 4 * (size_t)S; }
    const int *hull_first() const { return iv.data(); }
    const int *hull_count() const { return iv.data() + S; }
};
enum { kBlobOk = 0, kBlobTooSmall, kBlobInvalid };
static int read_map_blob(const void *blob, size_t size, MapBlob &mb)
{
    if (!blob || size < 64) return kBlobTooSmall;
    const unsigned char *b = static_cast<const unsigned char *>(blob);
    int32_t h[16];
    memcpy(h, b, 64);
    mb.S = h[2]; mb.P = h[3]; mb.A = h[4]; mb.n_cops = h[5]; mb.n_regions = h[7];
    if ((unsigned)h[0] != kBlobMagic || h[1] != 1 || mb.S < 1 || mb.S > CAT_MAX_SHAPES || mb.P < 0 || mb.A < 0 || mb.n_regions < 0) return kBlobInvalid;
    const size_t nf = 2 + 4 * (size_t)mb.S + 8 * (size_t)mb.P + 2 * (size_t)mb.A + 4 * (size_t)mb.n_regions;
    const size_t ni = 2 * (size_t)mb.S + (size_t)mb.A + 1;
    if (size != 64 + nf * 8 + ni * 4) return kBlobInvalid;
    mb.f.resize(nf);
    mb.iv.resize(ni);
    memcpy(mb.f.data(), b + 64, nf * 8);
    memcpy(mb.iv.data(), b + 64 + nf * 8, ni * 4);
    return kBlobOk;
}
// ... as the host-only entries report it
static int read_map_blob_host(const void *blob, size_t size, MapBlob &mb)
{
    const int r = read_map_blob(blob, size, mb);
    return r == kBlobOk ? CAT_OK : (r == kBlobTooSmall ? CAT_ERR_BAD_ARG : CAT_ERR_BAD_MAP);
}

// ---------------------------------------------------------------------- spatial-hash grids ----
struct GridHost {
    std::vector<GridDesc> desc;
    std::vector<unsigned long long> rows;   // per (cell, ray): count | first ids (row_words 8-byte words), see finalize_rows
    std::vector<int> rows_of;               // rows per map
    std::vector<unsigned long long> crows;  // per cell: count | first 7 contact candidates
    int max_row = 0, row_words = 1;
    int id_bits = 0;                        // > 0: four-byte rows (finalize_rows)
    std::vector<int> off, coff;
    std::vector<unsigned char> ent, cent;
};

// One map.  bb: [S][4] wall bbs (already inflated by the wall radius); the walls' plane records follow them (bb + 4 S:
// n.x n.y v0.x v0.y dot(v0, n) ...; hull_first / hull_count index them).  Three rules decide whether a wall is listed for
// (cell, ray k); all three keep [CP cpSpaceSegmentQueryFirst]'s result for every origin in the cell exactly as the full wall list gives it.
//  1. The visit (always): the wall's bb, grown by 1e-6 (gate off: by the ray radius), meets the region swept by the thin segment origin -> origin + d_k over
//     all origins of the cell: conv(cell, cell + d_k), a hexagon whose edge normals are x, y and perp(d_k) -- a separating-axis
//     test on those three axes is exact.
//  2. The hit (CAT_GRID_HULLS=0 turns it off): some ray of the cell can come within rsum = wall radius + ray radius of the HULL
//     (separating axes: perp(d_k) with the hull's own vertices, every face normal).  A wall whose shape query cannot return a hit
//     leaves no trace whether it is visited or not (agh-map: 21 % fewer entries -- triangles, slanted and merged blocks).
//  3. Occlusion (CAT_GRID_OCCLUSION=0 turns it off): if every ray of the cell is certain to cross the hull of some listed wall W
//     no later than T (in units of the ray), then after W's turn the best alpha is <= T whatever came before; a wall whose bb,
//     grown by the ray radius, is entered later than T by every ray of the cell (so t_bb > T and alpha > T) can then be taken out
//     of the sequence: while the best alpha is above T such a wall can only replace it by another value above T, and every wall
//     that stays is visited or not regardless of such values PROVIDED its own t_bb never exceeds T -- so T is first raised past
//     the latest thin-bb entry of every remaining wall whose range of entries straddles it.  (Agents come after the walls in
//     the visiting order: by then the best alpha is the same with and without the walls taken out.)
struct RotPoly {   // a convex polygon seen from one ray direction: per vertex its depth along the ray in units of the ray, and its offset across it
    int n;
    double al[CAT_MAX_HULL_EDGES + 1], si[CAT_MAX_HULL_EDGES + 1], smin, smax;
    void close() { smin = 1e300; smax = -1e300; for (int i = 0; i < n; i++) { smin = std::fmin(smin, si[i]); smax = std::fmax(smax, si[i]); } }
    // smallest depth among the polygon's points at offset s (s within [smin, smax])
    double entry(double s) const
    {
        double best = 1e300;
        for (int i = 0; i < n; i++) {
            const int j = i + 1 < n ? i + 1 : 0;
            const double s0 = si[i], s1 = si[j];
            if ((s0 <= s && s <= s1) || (s1 <= s && s <= s0))
                best = std::fmin(best, s0 == s1 ? std::fmin(al[i], al[j]) : al[i] + (al[j] - al[i]) * ((s - s0) / (s1 - s0)));
        }
        return best;
    }
    // bounds of entry() over the offsets [a, b] clipped to the polygon: false if they do not meet
    bool entry_range(double a, double b, double &emin, double &emax) const
    {
        const double lo = std::fmax(a, smin), hi = std::fmin(b, smax);
        if (lo > hi) return false;
        const double e0 = entry(lo), e1 = entry(hi);
        emax = std::fmax(e0, e1);            // entry() is convex in s: its maximum over an interval is at an end
        emin = std::fmin(e0, e1);            // its minimum is at an end or at a vertex in between (any vertex there bounds it from below)
        for (int i = 0; i < n; i++) if (lo <= si[i] && si[i] <= hi) emin = std::fmin(emin, al[i]);
        return true;
    }
};

struct GridRowOut { std::vector<int> off, coff; std::vector<unsigned char> ent, cent; int max_row = 0; };

static void build_grids(const double *bb, int S, int R, const double *rdx, const double *rdy, double reach,
                        bool gate, double m_contact, double cell, GridHost &g, const int *hull_first, const int *hull_count,
                        double rsum, double ray_radius, bool tree, bool hull_rule, bool occlusion_rule)   // (the two rules: Knobs::grid_hulls / grid_occlusion)
{
    // Tree order (bbtree_gate = CAT_GATE_TREE): rules 1 and 2 only.  Both are necessary for a wall to change the best alpha under ANY visiting order,
    // and the device's order-free summary needs the alpha of every wall that is entered and hit, which rule 3 (proved for index order) does not keep.
    // A single wall is the root of its tree and visited ungated (DESIGN D6): it is listed by rule 2 alone (rule 1 with the fat ray, which rule 2 implies).
    if (tree && S == 1) gate = false;
    const double m_ray = gate ? 1e-6 : ray_radius + 1e-6;   // gate off: every wall the fat ray can touch counts as visited
    const double *planes = bb + 4 * (size_t)S;
    const bool by_hull = hull_first != nullptr && hull_rule, occlusion = hull_first != nullptr && !tree && occlusion_rule;
    double lo[2] = {1e300, 1e300}, hi[2] = {-1e300, -1e300};
    for (int s = 0; s < S; s++) {
        lo[0] = std::fmin(lo[0], bb[4 * s]); lo[1] = std::fmin(lo[1], bb[4 * s + 1]);
        hi[0] = std::fmax(hi[0], bb[4 * s + 2]); hi[1] = std::fmax(hi[1], bb[4 * s + 3]);
    }
    GridDesc d{};
    d.x0 = std::floor(lo[0] - reach - cell); d.y0 = std::floor(lo[1] - reach - cell);
    d.nx = (int)std::ceil((hi[0] + reach + cell - d.x0) / cell); d.ny = (int)std::ceil((hi[1] + reach + cell - d.y0) / cell);
    d.inv_cell = 1.0 / cell;
    d.off_base = (int)g.off.size(); d.ent_base = (int)g.ent.size();
    d.coff_base = (int)g.coff.size(); d.cent_base = (int)g.cent.size();
    d.row_base = 0;   // set by finalize_rows
    const double eps = 1e-6;   // cell membership is decided in floating point on the device
    const double mt = 1e-7;    // occlusion: slack on every bound, in units of the ray (4e-5 px of a 400-px ray)

    // one row of cells: its part of the CSR arrays, offsets relative to the row
    auto do_row = [&](int cy, GridRowOut &o) {
        std::vector<int> near, list;     // walls within reach of the cell (prefilter); the walls listed for (cell, ray)
        std::vector<double> f_lo, b_hi, cuts;
        std::vector<RotPoly> hulls;
        for (int cx = 0; cx < d.nx; cx++) {
            const double X0 = d.x0 + cx * cell - eps, X1 = d.x0 + (cx + 1) * cell + eps;
            const double Y0 = d.y0 + cy * cell - eps, Y1 = d.y0 + (cy + 1) * cell + eps;
            near.clear();
            o.coff.push_back((int)o.cent.size());
            for (int s = 0; s < S; s++) {
                const double l = bb[4 * s], b = bb[4 * s + 1], r = bb[4 * s + 2], t = bb[4 * s + 3];
                if (l - m_contact <= X1 && X0 <= r + m_contact && b - m_contact <= Y1 && Y0 <= t + m_contact)
                    o.cent.push_back((unsigned char)s);
                if (l - reach <= X1 && X0 <= r + reach && b - reach <= Y1 && Y0 <= t + reach) near.push_back(s);
            }
            // the walls listed for ray k and the origins of the rectangle [X0, X1] x [Y0, Y1] (rules 1 - 3), ascending, into `list`
            auto list_for = [&](int k, double X0, double X1, double Y0, double Y1) {
                const double dx = rdx[k], dy = rdy[k];
                const double hx0 = X0 + std::fmin(0.0, dx) - eps, hx1 = X1 + std::fmax(0.0, dx) + eps;
                const double hy0 = Y0 + std::fmin(0.0, dy) - eps, hy1 = Y1 + std::fmax(0.0, dy) + eps;
                // projections of the cell on n = (-dy, dx)
                const double c0 = -dy * X0 + dx * Y0, c1 = -dy * X1 + dx * Y0, c2 = -dy * X0 + dx * Y1, c3 = -dy * X1 + dx * Y1;
                const double nscale = std::fabs(dx) + std::fabs(dy);
                const double pmin = std::fmin(std::fmin(c0, c1), std::fmin(c2, c3)) - eps * nscale;
                const double pmax = std::fmax(std::fmax(c0, c1), std::fmax(c2, c3)) + eps * nscale;
                list.clear();
                for (int s : near) {
                    const double l = bb[4 * s] - m_ray, b = bb[4 * s + 1] - m_ray, r = bb[4 * s + 2] + m_ray, t = bb[4 * s + 3] + m_ray;
                    if (!(l <= hx1 && hx0 <= r && b <= hy1 && hy0 <= t)) continue;
                    const double q0 = -dy * l + dx * b, q1 = -dy * r + dx * b, q2 = -dy * l + dx * t, q3 = -dy * r + dx * t;
                    const double qmin = std::fmin(std::fmin(q0, q1), std::fmin(q2, q3)), qmax = std::fmax(std::fmax(q0, q1), std::fmax(q2, q3));
                    if (!(qmin <= pmax && pmin <= qmax)) continue;
                    if (by_hull) {
                        const double *pl = planes + 8 * (size_t)hull_first[s];
                        const int ne = hull_count[s];
                        const double grow = (rsum + eps) * std::sqrt(dx * dx + dy * dy);
                        double vmin = 1e300, vmax = -1e300;
                        for (int e = 0; e < ne; e++) {
                            const double v = -dy * pl[8 * e + 2] + dx * pl[8 * e + 3];
                            vmin = std::fmin(vmin, v); vmax = std::fmax(vmax, v);
                        }
                        bool apart = vmin - grow > pmax || vmax + grow < pmin;
                        for (int e = 0; e < ne && !apart; e++) {
                            const double nx = pl[8 * e], ny = pl[8 * e + 1];
                            const double lowest = std::fmin(nx * X0, nx * X1) + std::fmin(ny * Y0, ny * Y1) + std::fmin(0.0, nx * dx + ny * dy);
                            apart = lowest > pl[8 * e + 4] + rsum + eps;
                        }
                        if (apart) continue;
                    }
                    list.push_back(s);
                }
                if (occlusion && list.size() > 1) {
                    const double dd = dx * dx + dy * dy;
                    const double a0 = (X0 * dx + Y0 * dy) / dd, a1 = (X1 * dx + Y0 * dy) / dd, a2 = (X0 * dx + Y1 * dy) / dd, a3 = (X1 * dx + Y1 * dy) / dd;
                    const double amin = std::fmin(std::fmin(a0, a1), std::fmin(a2, a3)), amax = std::fmax(std::fmax(a0, a1), std::fmax(a2, a3));
                    // a margin across the ray, in the units of pmin / pmax: a ray passing that far outside a hull's end vertex still meets the
                    // ROUNDED shape -- which needs a wall radius well above the margin.  With wall_radius ~ 0 the bb coincides with the hull,
                    // a thin ray in that sliver misses the bb and the wall is never visited: no slack then.
                    const double ms = (rsum - ray_radius) > 1e3 * eps ? eps * nscale : 0.0;
                    const size_t n = list.size();
                    f_lo.assign(n, 1e300); b_hi.assign(n, -1e300);
                    hulls.resize(n);
                    cuts.clear();
                    cuts.push_back(pmin); cuts.push_back(pmax);
                    for (size_t q = 0; q < n; q++) {
                        const int s = list[q];
                        RotPoly &H = hulls[q];
                        RotPoly B, F;
                        const double *pl = planes + 8 * (size_t)hull_first[s];
                        H.n = hull_count[s];
                        for (int e = 0; e < H.n; e++) {
                            const double vx = pl[8 * e + 2], vy = pl[8 * e + 3];
                            H.al[e] = (vx * dx + vy * dy) / dd; H.si[e] = -dy * vx + dx * vy;
                            if (pmin < H.si[e] && H.si[e] < pmax) cuts.push_back(H.si[e]);
                        }
                        H.close();
                        const double l = bb[4 * s], b = bb[4 * s + 1], r = bb[4 * s + 2], t = bb[4 * s + 3];
                        const double cxs[4] = {l, r, r, l}, cys[4] = {b, b, t, t};
                        B.n = F.n = 4;
                        for (int e = 0; e < 4; e++) {
                            B.al[e] = (cxs[e] * dx + cys[e] * dy) / dd; B.si[e] = -dy * cxs[e] + dx * cys[e];
                            const double fx = cxs[e] + ((e == 1 || e == 2) ? ray_radius : -ray_radius), fy = cys[e] + (e >= 2 ? ray_radius : -ray_radius);
                            F.al[e] = (fx * dx + fy * dy) / dd; F.si[e] = -dy * fx + dx * fy;
                        }
                        B.close(); F.close();
                        double emin, emax;
                        if (F.entry_range(pmin, pmax, emin, emax)) f_lo[q] = std::fmax(0.0, emin - amax) - mt;
                        if (!gate) b_hi[q] = 0.0;   // every listed wall counts as entered at once
                        else if (B.entry_range(pmin, pmax, emin, emax)) b_hi[q] = std::fmax(0.0, emax - amin) + mt;
                    }
                    // T: by when every ray of the cell has certainly crossed the hull of SOME listed wall.  Between two neighbouring
                    // cuts (the cell's span across the ray, cut at the hull vertices inside it) every hull's entry depth is linear; a
                    // hull counts there if it spans the piece (a ray passing a hair -- ms -- outside its end vertex still meets the
                    // rounded shape before that vertex's depth) and every origin of the cell lies before it; the piece's bound is the
                    // smallest of the hulls' larger end values (max-min <= min-max), T the largest bound of any piece.
                    std::sort(cuts.begin(), cuts.end());
                    double T = -1e300;
                    for (size_t c = 0; c + 1 < cuts.size() && T < 1e299; c++) {
                        const double lft = cuts[c], rgt = cuts[c + 1];
                        if (!(lft < rgt)) continue;
                        double best = 1e300;
                        for (size_t q = 0; q < n; q++) {
                            const RotPoly &H = hulls[q];
                            if (H.n < 3 || !(H.smin - ms <= lft && rgt <= H.smax + ms)) continue;
                            const double e0 = H.entry(std::fmin(std::fmax(lft, H.smin), H.smax)), e1 = H.entry(std::fmin(std::fmax(rgt, H.smin), H.smax));
                            if (!(amax <= std::fmin(e0, e1) - mt)) continue;
                            best = std::fmin(best, std::fmax(e0, e1));
                        }
                        T = std::fmax(T, best);
                    }
                    T = (T > -1e299 && T < 1e299 && T - amin <= 1.0 - 2.0 * mt) ? T - amin + mt : 1e300;
                    if (T < 1e299) {
                        for (bool again = true; again;) {
                            again = false;
                            for (size_t q = 0; q < n; q++)
                                if (f_lo[q] <= T && T < b_hi[q]) { T = b_hi[q]; again = true; }
                        }
                        size_t w = 0;
                        for (size_t q = 0; q < n; q++) if (f_lo[q] <= T) list[w++] = list[q];
                        list.resize(w);
                    }
                }
            };
            for (int k = 0; k < R; k++) {
                o.off.push_back((int)o.ent.size());
                list_for(k, X0, X1, Y0, Y1);
                for (int s : list) o.ent.push_back((unsigned char)s);
                if ((int)list.size() > o.max_row) o.max_row = (int)list.size();
            }
        }
    };
    std::vector<GridRowOut> rows((size_t)d.ny);
    {
        unsigned nt = std::thread::hardware_concurrency();
        {   // the CPUs this process may run on (a container's share), not the machine's
            cpu_set_t set;
            if (sched_getaffinity(0, sizeof set, &set) == 0 && CPU_COUNT(&set) > 0 && (unsigned)CPU_COUNT(&set) < nt) nt = (unsigned)CPU_COUNT(&set);
        }
        if (nt > 16) nt = 16;
        if (nt < 1) nt = 1;
        if ((int)nt > d.ny) nt = (unsigned)d.ny;
        std::atomic<int> next{0};
        auto worker = [&]() { for (int cy = next.fetch_add(1); cy < d.ny; cy = next.fetch_add(1)) do_row(cy, rows[(size_t)cy]); };
        std::vector<std::thread> pool;
        for (unsigned t = 1; t < nt; t++) pool.emplace_back(worker);
        worker();
        for (auto &t : pool) t.join();
    }
    for (int cy = 0; cy < d.ny; cy++) {
        const GridRowOut &o = rows[(size_t)cy];
        const int e0 = (int)g.ent.size() - d.ent_base, c0 = (int)g.cent.size() - d.cent_base;
        for (int v : o.off) g.off.push_back(e0 + v);
        for (int v : o.coff) g.coff.push_back(c0 + v);
        g.ent.insert(g.ent.end(), o.ent.begin(), o.ent.end());
        g.cent.insert(g.cent.end(), o.cent.begin(), o.cent.end());
        if (o.max_row > g.max_row) g.max_row = o.max_row;
    }
    rows.clear();
    g.off.push_back((int)g.ent.size() - d.ent_base);
    g.coff.push_back((int)g.cent.size() - d.cent_base);
    d.crow_base = (int)g.crows.size();
    for (int c = 0; c < d.nx * d.ny; c++) {
        const int o0 = g.coff[d.coff_base + c] + d.cent_base, n = g.coff[d.coff_base + c + 1] + d.cent_base - o0;
        unsigned long long w = (unsigned long long)(n > 255 ? 255 : n);
        for (int q = 0; q < n && q < 7; q++) w |= (unsigned long long)g.cent[o0 + q] << (8 * (q + 1));
        g.crows.push_back(w);
    }
    while (g.ent.size() & 3) g.ent.push_back(0);
    while (g.cent.size() & 3) g.cent.push_back(0);
    g.desc.push_back(d);
    g.rows_of.push_back(d.nx * d.ny * R);
}

// ---------------------------------------------------------------------- Chipmunk's static tree ----
// The tree [CP cpBBTreeInsert] builds when the walls are inserted one after the other in index order (Map.populate_space adds them in file order):
// node s < S is the leaf of wall s (its bb is the wall's bb, the static index has no velocity function); inner nodes follow in creation order.  An
// insertion below an inner node descends into the child with the smaller cost  area(other child) + merged area(this child, new leaf), on equal costs
// into the one nearer by [CP cpBBProximity], into b only if strictly better; where it meets a leaf (or the empty tree) a new inner node takes the
// NEW leaf as child a and what it met as child b; every inner node on the way is merged with the new leaf's bb (exact min / max).  Nothing reorders
// a static tree afterwards.
struct TreeNode { double bb[4]; int a, b, parent, wall; };
constexpr int kMaxTreeDepth = 48;   // cat_create refuses a tree-order map whose tree is deeper (the five maps shipped: 3 - 11)

static void build_static_tree(const double *bb, int S, std::vector<TreeNode> &n, int &root, int &depth)
{
    n.assign(S > 0 ? 2 * (size_t)S - 1 : 0, TreeNode{});
    for (int s2 = 0; s2 < S; s2++) { memcpy(n[s2].bb, bb + 4 * (size_t)s2, 32); n[s2].a = n[s2].b = n[s2].parent = -1; n[s2].wall = s2; }
    auto mn = [](double x, double y) { return x < y ? x : y; };   // [CP cpfmin / cpfmax]
    auto mx = [](double x, double y) { return x > y ? x : y; };
    auto area = [](const double *x) { return (x[2] - x[0]) * (x[3] - x[1]); };
    auto merged_area = [&](const double *x, const double *y) { return (mx(x[2], y[2]) - mn(x[0], y[0])) * (mx(x[3], y[3]) - mn(x[1], y[1])); };
    auto proximity = [](const double *x, const double *y) { return std::fabs(x[0] + x[2] - y[0] - y[2]) + std::fabs(x[1] + x[3] - y[1] - y[3]); };
    auto merge_into = [&](double *d, const double *y) { d[0] = mn(d[0], y[0]); d[1] = mn(d[1], y[1]); d[2] = mx(d[2], y[2]); d[3] = mx(d[3], y[3]); };
    int next = S;
    root = S > 0 ? 0 : -1;
    for (int leaf = 1; leaf < S; leaf++) {
        const double *lb = n[leaf].bb;
        int at = root, up = -1;   // the subtree the leaf meets, and the inner node above it
        bool in_b = false;
        while (n[at].wall < 0) {
            const int ca = n[at].a, cb = n[at].b;
            double cost_a = area(n[cb].bb) + merged_area(n[ca].bb, lb), cost_b = area(n[ca].bb) + merged_area(n[cb].bb, lb);
            if (cost_a == cost_b) { cost_a = proximity(n[ca].bb, lb); cost_b = proximity(n[cb].bb, lb); }
            merge_into(n[at].bb, lb);
            up = at;
            in_b = cost_b < cost_a;
            at = in_b ? cb : ca;
        }
        const int k = next++;
        TreeNode &q = n[k];
        q.a = leaf; q.b = at; q.wall = -1; q.parent = up;
        memcpy(q.bb, lb, 32);
        merge_into(q.bb, n[at].bb);
        n[leaf].parent = k; n[at].parent = k;
        if (up < 0) root = k;
        else if (in_b) n[up].b = k;
        else n[up].a = k;
    }
    depth = 0;
    for (int s2 = 0; s2 < S; s2++) {
        int d = 0;
        for (int x = s2; n[x].parent >= 0; x = n[x].parent) d++;
        depth = std::max(depth, d);
    }
}

// Host-only: the static tree of one map's walls (what cat_create builds in tree order), for the CPU tests.  Writes up to max_nodes nodes:
// bb[4 n ..] (l b r t) and link[4 n ..] = child a, child b, parent, wall id (leaf) or -1; returns the node count (2 S - 1) or an error.
extern "C" int cat_bbtree_host(const void *blob, size_t size, double *bb_out, int *link_out, int max_nodes, int *root, int *depth)
{
    MapBlob mb;
    if (const int rc = read_map_blob_host(blob, size, mb)) return rc;
    std::vector<TreeNode> n;
    int r = -1, d = 0;
    build_static_tree(mb.bb(), mb.S, n, r, d);
    for (int k = 0; k < (int)n.size() && k < max_nodes; k++) {
        if (bb_out) memcpy(bb_out + 4 * (size_t)k, n[k].bb, 32);
        if (link_out) { link_out[4 * k] = n[k].a; link_out[4 * k + 1] = n[k].b; link_out[4 * k + 2] = n[k].parent; link_out[4 * k + 3] = n[k].wall; }
    }
    if (root) *root = r;
    if (depth) *depth = d;
    return (int)n.size();
}

// The most wall bounding boxes the bb of ONE agent circle can overlap at once, anywhere on the map: an upper bound on the wall
// arbiters an agent can hold in one step ([CP cpSpaceCollideShapes] makes one only on a real contact), to be held against the
// CAT_WALL_CACHE slots of the state record at cat_create instead of being discovered at run time (CAT_DEVERR_CONTACT_DROPPED).
// The circle's bb overlaps a wall's iff its centre lies in the wall's bb grown by the radius (closed rectangles): the deepest point
// of such an arrangement is the left edge of one rectangle and the bottom edge of one.
static int max_wall_bb_depth(const double *bb, int S, double rc)
{
    int best = 0;
    for (int a = 0; a < S; a++) {
        const double x = bb[4 * a] - rc;
        for (int b = 0; b < S; b++) {
            const double y = bb[4 * b + 1] - rc;
            int n = 0;
            for (int s = 0; s < S; s++)
                n += (bb[4 * s] - rc <= x && x <= bb[4 * s + 2] + rc && bb[4 * s + 1] - rc <= y && y <= bb[4 * s + 3] + rc) ? 1 : 0;
            best = n > best ? n : best;
        }
    }
    return best;
}

extern "C" int cat_map_wall_bb_depth_host(const void *blob, size_t size, double agent_radius)
{
    MapBlob mb;
    if (const int rc = read_map_blob_host(blob, size, mb)) return rc;
    return max_wall_bb_depth(mb.bb(), mb.S, agent_radius);
}

// Packed rows, one per (cell, ray): byte 0 = count (saturating at 255), then the first 8*row_words - 1
// candidate ids; row_words (1, 2 or 4 eight-byte words) is the smallest that holds the longest list of
// any map of the sim, lists beyond 31 ids continue in the CSR arrays (slow path on the device).
// id_bits > 0 (fan_group sims: S <= 2^id_bits - 1 and every list has at most 32 / id_bits walls): FOUR-byte rows, two per word of
// `rows` -- field q (id_bits bits) = the list's q-th wall id + 1, zero beyond the list, so the count is the highest non-zero field's
// index + 1; d.row_base counts rows either way.
static void finalize_rows(GridHost &g, int id_bits = 0, bool wide = false)
{
    g.row_words = g.max_row <= 7 ? 1 : (g.max_row <= 15 ? 2 : 4);
    g.id_bits = id_bits;
    const int cap = 8 * g.row_words - 1;
    g.rows.clear();
    if (id_bits > 0 && wide) {   // the same fields in ONE eight-byte word per row (fan_chunk sims whose lists fit 64 / id_bits walls)
        g.row_words = 1;
        for (size_t m = 0; m < g.desc.size(); m++) {
            GridDesc &d = g.desc[m];
            d.row_base = (int)g.rows.size();
            for (int r = 0; r < g.rows_of[m]; r++) {
                const int o0 = g.off[d.off_base + r] + d.ent_base, n = g.off[d.off_base + r + 1] + d.ent_base - o0;
                unsigned long long w = 0ull;
                for (int q = 0; q < n; q++) w |= ((unsigned long long)g.ent[o0 + q] + 1ull) << (id_bits * q);
                g.rows.push_back(w);
            }
        }
        return;
    }
    if (id_bits > 0) {
        std::vector<unsigned> r32;
        for (size_t m = 0; m < g.desc.size(); m++) {
            GridDesc &d = g.desc[m];
            d.row_base = (int)r32.size();
            for (int r = 0; r < g.rows_of[m]; r++) {
                const int o0 = g.off[d.off_base + r] + d.ent_base, n = g.off[d.off_base + r + 1] + d.ent_base - o0;
                unsigned w = 0u;                                // n <= max_row <= 32 / id_bits
                for (int q = 0; q < n; q++) w |= ((unsigned)g.ent[o0 + q] + 1u) << (id_bits * q);
                r32.push_back(w);
            }
        }
        if (r32.size() & 1) r32.push_back(0u);
        g.rows.resize(r32.size() / 2);
        memcpy(g.rows.data(), r32.data(), r32.size() * 4);
        return;
    }
    for (size_t m = 0; m < g.desc.size(); m++) {
        GridDesc &d = g.desc[m];
        d.row_base = (int)(g.rows.size() / g.row_words);
        for (int r = 0; r < g.rows_of[m]; r++) {
            const int o0 = g.off[d.off_base + r] + d.ent_base, n = g.off[d.off_base + r + 1] + d.ent_base - o0;
            unsigned long long w[4] = {(unsigned long long)(n > 255 ? 255 : n), 0ull, 0ull, 0ull};
            for (int q = 0; q < n && q < cap; q++) {
                const int byte = q + 1;
                w[byte >> 3] |= (unsigned long long)g.ent[o0 + q] << (8 * (byte & 7));
            }
            for (int q = 0; q < g.row_words; q++) g.rows.push_back(w[q]);
        }
    }
}

// the tables of one map (a GridHost of its own, as build_grids leaves it) appended to a part's
static void append_grid(GridHost &g, const GridHost &m)
{
    GridDesc d = m.desc[0];
    d.off_base = (int)g.off.size(); d.ent_base = (int)g.ent.size();
    d.coff_base = (int)g.coff.size(); d.cent_base = (int)g.cent.size();
    d.crow_base = (int)g.crows.size();
    g.off.insert(g.off.end(), m.off.begin(), m.off.end());
    g.ent.insert(g.ent.end(), m.ent.begin(), m.ent.end());
    g.coff.insert(g.coff.end(), m.coff.begin(), m.coff.end());
    g.cent.insert(g.cent.end(), m.cent.begin(), m.cent.end());
    g.crows.insert(g.crows.end(), m.crows.begin(), m.crows.end());
    g.desc.push_back(d);
    g.rows_of.push_back(m.rows_of[0]);
    if (m.max_row > g.max_row) g.max_row = m.max_row;
}

static int grid_lookup(const GridHost &g, int map_index, int R, double x, double y, int k, int *out, int max_out)
{
    const GridDesc &d = g.desc[map_index];
    const int cx = (int)std::floor((x - d.x0) * d.inv_cell), cy = (int)std::floor((y - d.y0) * d.inv_cell);
    if (cx < 0 || cy < 0 || cx >= d.nx || cy >= d.ny) return 0;
    const int cellid = cy * d.nx + cx;
    int o0, o1;
    const unsigned char *ent;
    if (k >= 0) {
        const int row = cellid * R + k;
        o0 = g.off[d.off_base + row]; o1 = g.off[d.off_base + row + 1];
        ent = g.ent.data() + d.ent_base;
    } else {
        o0 = g.coff[d.coff_base + cellid]; o1 = g.coff[d.coff_base + cellid + 1];
        ent = g.cent.data() + d.cent_base;
    }
    int n = 0;
    for (int i = o0; i < o1 && n < max_out; i++) out[n++] = ent[i];
    return o1 - o0;
}

// Host-only construction of the tables of ONE map (no device needed): used by the CPU tests that
// check the tables are supersets of the exact gate.
struct cat_grid_host { GridHost g; int R; };

extern "C" int cat_grid_build_host(const cat_config *cfg, const cat_tables *tab, const void *blob, size_t size,
                                   double cell, cat_grid_host **out)
{
    if (!cfg || !tab || !out) return CAT_ERR_BAD_ARG;
    MapBlob mb;
    if (const int rc = read_map_blob_host(blob, size, mb)) return rc;
    const Knobs knobs = read_knobs();
    cat_grid_host *gh = new cat_grid_host();
    gh->R = cfg->n_rays;
    build_grids(mb.bb(), mb.S, cfg->n_rays, tab->ray_dx, tab->ray_dy, cfg->ray_length + cfg->ray_radius + 1e-3,
                cfg->bbtree_gate != 0, cfg->ray_radius + 2e-6, cell > 0 ? cell : 8.0, gh->g,
                mb.hull_first(), mb.hull_count(), cfg->wall_radius + cfg->ray_radius, cfg->ray_radius, cfg->bbtree_gate == CAT_GATE_TREE,
                knobs.grid_hulls, knobs.grid_occlusion);
    finalize_rows(gh->g);
    *out = gh;
    return CAT_OK;
}

extern "C" int cat_grid_lookup_host(const cat_grid_host *gh, double x, double y, int k, int *out, int max_out)
{
    if (!gh || k >= gh->R) return CAT_ERR_BAD_ARG;
    return grid_lookup(gh->g, 0, gh->R, x, y, k, out, max_out);
}

extern "C" long long cat_grid_bytes_host(const cat_grid_host *gh)
{
    return gh ? (long long)(gh->g.rows.size() * 8 + gh->g.off.size() * 4 + gh->g.ent.size() + gh->g.coff.size() * 4 + gh->g.cent.size()) : 0;
}

extern "C" void cat_grid_free_host(cat_grid_host *gh) { delete gh; }
