// gi_walk.h -- a ray through the scene octree: the record sources (NodeView, GlobalNodes, GlobalWide), the wide-node walk in its per-lane and
// cooperative forms, the per-node walk (trace_nodes, visible_nodes), trace and visible, the walk counters (GI_DIV*, WalkCnt) and the parity
// tests' diagnostics (leaf_order, kat_eval).  Needs gi_scene.h, gi_math.h and gi_intersect.h.  Included by gi_device.h inside namespace gi,
// behind gi_intersect.h.
//
// Reference semantics followed (file:line relative to moepforfreedom/GI_Raytracer):
//   trace            include/raytracer.h:382-478 + include/octree.cpp:188-211,285-313 + include/bbox.h:47-73
//   visible          include/raytracer.h:280-319 + include/octree.cpp:150-185,256-282 + include/bbox.h:117-138

// Where node records come from: plain global memory here; gi_lds.h adds a source that serves the first nodes from LDS.
struct NodeView { double bmin[3], bmax[3]; int32_t first_ref, n_ref, hit, skip; };
struct GlobalNodes {
    static constexpr bool kWide = false;
    const TNode* g;
    GI_HDM void fetch(int32_t i, int oct, NodeView& v) const
    {
        const TNode& n = g[i];
        v.bmin[0] = n.bmin[0]; v.bmin[1] = n.bmin[1]; v.bmin[2] = n.bmin[2];
        v.bmax[0] = n.bmax[0]; v.bmax[1] = n.bmax[1]; v.bmax[2] = n.bmax[2];
        v.first_ref = n.first_ref; v.n_ref = n.n_ref;
        v.hit = n.link[oct].hit; v.skip = n.link[oct].skip;
    }
    GI_HDM int32_t leaf_id(int32_t i) const { return g[i].leaf_id; }
};

// ------------------------------------------------------------------------------------------------ wide-node walk
// The same walk as trace_nodes / visible_nodes below -- children of every node in the order k ^ a, every child's box tested with
// the reference's slab arithmetic, leaves met in the same order -- but a node's children are tested together from the WNode of
// their parent.  BoundingBox::intersect updates tmin upwards and tmax downwards axis by axis and leaves at the first
// tmax <= tmin (include/bbox.h:47-73); both are monotone, so it returns false exactly when the final tmax <= tmin, and
// `t0 > tmin ? t0 : tmin` is maxNum (a NaN from 0 * inf is ignored), which is what fmax / v_max_f64 compute.
struct WRay { int a; double tc; bool plain; };   // a = direction octant; tc = parameter beyond which no hit can count (content-box culling, the closest-hit walk's cut);
                                                  // plain: a closest-hit walk that asks every entity the reference asks (trace_wide_step): no content culling either
// 8 when the ray runs backwards along an axis (invDir < 0), else 0: the byte offset between a plane pair's near and far side in a wide record.  Read off
// the sign bit of 1/d each time (1/d is never a zero or a NaN) -- three registers a walk does not have to hold
GI_HD int back_off(double inv)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return (int)(((uint32_t)__double2hiint(inv) >> 31) << 3);
#else
    return inv < 0.0 ? 8 : 0;
#endif
}
GI_HD WRay wray_make(const Ray& r)
{
    WRay w;
    w.a = (r.d.x < 0.0 ? 1 : 0) | (r.d.z < 0.0 ? 2 : 0) | (r.d.y < 0.0 ? 4 : 0);
    w.tc = INFINITY;
    w.plain = false;
    return w;
}
// Content-box culling.  The reference's octree cuts space, not content: a leaf that holds a piece of the floor spans its whole octant, and
// a ray passing over the floor has to test every triangle in it.  Next to every child's octant box (the reference's test, unchanged) the
// wide records carry the box of everything REFERENCED in that child's sub-tree -- the union of the entities' own boxes, widened by a margin
// a billion times the rounding of a hit point and rounded outwards to float.  A child whose octant the ray enters is skipped when the ray
// misses that box inside [0, tc]: no entity below it can then report a hit (a hit lies on its entity, at t >= 0 and, for a shadow ray,
// before the light), so every hit the reference records is still recorded, in the same order, and the walk stops after the same leaf --
// same results by construction (frames with and without culling are compared bit for bit, gi_set_content_culling).  What it saves is the
// visits that could not have mattered: in the benchmark 96 % of the reflected rays leave the scene, and their walks shrink to a few nodes.
// m: candidate children in the ray's order (bit k = slot k ^ a); returns m without the children the ray cannot hit anything in.
GI_HD uint32_t content_cull(const float* cboxes, const uint32_t* cuse, int32_t node, uint32_t m, const Ray& r, const WRay& wr, uint32_t* n_tested = nullptr)
{
    uint32_t u = cuse[node];
    if (wr.a & 1) u = ((u & 0x55u) << 1) | ((u >> 1) & 0x55u);      // slot bits -> the ray's order, as wide_hits does
    if (wr.a & 2) u = ((u & 0x33u) << 2) | ((u >> 2) & 0x33u);
    if (wr.a & 4) u = ((u & 0x0fu) << 4) | ((u >> 4) & 0x0fu);
    uint32_t todo = m & u;
    if (n_tested) *n_tested = (uint32_t)__builtin_popcount(todo);
    const double o[3] = {r.o.x, r.o.y, r.o.z}, inv[3] = {r.inv.x, r.inv.y, r.inv.z};
    while (todo) {
        const int kk = __builtin_ctz(todo);
        todo &= todo - 1;
        const float* b = cboxes + ((size_t)node * 8 + (size_t)(kk ^ wr.a)) * 6;
        double tn = 0.0, tf = wr.tc;
        for (int ax = 0; ax < 3; ax++) {
            // entry plane first: a NaN (origin exactly on a plane of an axis the ray does not move along: 0 * inf) is ignored by fmax / fmin,
            // which is the right answer -- the origin is inside that closed slab
            const int back = back_off(inv[ax]) ? 3 : 0;
            tn = fmax(tn, ((double)b[ax + back] - o[ax]) * inv[ax]);
            tf = fmin(tf, ((double)b[ax + 3 - back] - o[ax]) * inv[ax]);
        }
        if (!(tf >= tn)) m &= ~(1u << kk);
    }
    return m;
}
// Entity boxes.  A leaf of the reference's octree holds up to a few dozen entities and RayTracer::trace / visible test every one of them
// (include/raytracer.h:290-305,446-472); a ray through the leaf touches the boxes of one or two.  An entity whose own box -- widened by a margin
// a billion times the rounding of a hit point -- the ray misses inside [0, tc] cannot report a hit (the hit point lies on the entity, at t > 0
// and, for a shadow ray, before the light), so its test is skipped: the same hits in the same order, the same draws.  The lanes of a wave first
// sort their leaf's references into a bit mask (a slab test of 24 flops per reference), then run Entity::intersect (~50 flops and a division)
// on the few that are left -- the wave's loop is as long as its longest lane's, and that is now the lane with the most SURVIVORS.
GI_HD bool entity_box_missed(const double* b, const Ray& r, double tc)
{
    const double o[3] = {r.o.x, r.o.y, r.o.z}, inv[3] = {r.inv.x, r.inv.y, r.inv.z};
    double tn = 0.0, tf = tc;
    for (int ax = 0; ax < 3; ax++) {
        const double t0 = (b[ax] - o[ax]) * inv[ax], t1 = (b[3 + ax] - o[ax]) * inv[ax];
        // a NaN (origin on a plane of an axis the ray does not move along: 0 * inf) is ignored by fmin / fmax: the origin is inside that slab
        tn = fmax(tn, fmin(t0, t1));
        tf = fmin(tf, fmax(t0, t1));
    }
    return !(tf >= tn);
}
// the references [first, first + cnt) of a leaf (cnt <= 32) whose boxes the ray touches, as a bit mask; all of them without the table
GI_HD uint32_t entity_survivors(const double* boxes, int32_t first, int32_t cnt, const Ray& r, double tc)
{
    uint32_t m = cnt >= 32 ? 0xffffffffu : ((1u << cnt) - 1u);
    if (!boxes) return m;
    for (int32_t j = 0; j < cnt; j++)
        if (entity_box_missed(boxes + (size_t)(first + j) * 6, r, tc)) m &= ~(1u << j);
    return m;
}
// bit k of the result: the k-th child in this ray's front-to-back order (slot k ^ a) exists and its box is hit in (tmin0, tmax0)
GI_HD uint32_t wide_hits(const WNode* w, const Ray& r, const WRay& wr, double tmin0, double tmax0)
{
    const char* b = reinterpret_cast<const char*>(w);
    const double o[3] = {r.o.x, r.o.y, r.o.z}, inv[3] = {r.inv.x, r.inv.y, r.inv.z};
    double n[3][3], f[3][3];   // [axis][low side, high side, child 7]: entry and exit parameter
    for (int ax = 0; ax < 3; ax++) {
        const int A = ax * 48, x = back_off(inv[ax]), y = x ^ 8;
        n[ax][0] = (*reinterpret_cast<const double*>(b + A + x) - o[ax]) * inv[ax];
        f[ax][0] = (*reinterpret_cast<const double*>(b + A + y) - o[ax]) * inv[ax];
        n[ax][1] = (*reinterpret_cast<const double*>(b + A + 16 + x) - o[ax]) * inv[ax];
        f[ax][1] = (*reinterpret_cast<const double*>(b + A + 16 + y) - o[ax]) * inv[ax];
        n[ax][2] = (*reinterpret_cast<const double*>(b + A + 32 + y) - o[ax]) * inv[ax];
        f[ax][2] = (*reinterpret_cast<const double*>(b + A + 32 + x) - o[ax]) * inv[ax];
    }
    const double nx[2] = {fmax(n[0][0], tmin0), fmax(n[0][1], tmin0)}, fx[2] = {fmin(f[0][0], tmax0), fmin(f[0][1], tmax0)};
    uint32_t m = 0;
    for (int bz = 0; bz < 2; bz++)
        for (int bx = 0; bx < 2; bx++) {
            const double nA = fmax(nx[bx], n[2][bz]), fA = fmin(fx[bx], f[2][bz]);
            for (int by = 0; by < 2; by++) {
                const double t0 = fmax(nA, n[1][by]), t1 = fmin(fA, f[1][by]);
                if (t1 > t0) m |= 1u << (bx | (bz << 1) | (by << 2));
            }
        }
    {
        const double t0 = fmax(fmax(fmax(n[0][2], tmin0), n[1][2]), n[2][2]), t1 = fmin(fmin(fmin(f[0][2], tmax0), f[1][2]), f[2][2]);
        m = (m & 0x7fu) | (t1 > t0 ? 0x80u : 0u);
    }
    m &= w->exists;
    if (wr.a & 1) m = ((m & 0x55u) << 1) | ((m >> 1) & 0x55u);
    if (wr.a & 2) m = ((m & 0x33u) << 2) | ((m >> 2) & 0x33u);
    if (wr.a & 4) m = ((m & 0x0fu) << 4) | ((m >> 4) & 0x0fu);
    return m;
}
GI_HD void wide_leaf_box(const WNode* w, int slot, double* lmin, double* lmax)   // the box of child `slot` as partition() built it
{
    const int bit[3] = {slot & 1, (slot >> 2) & 1, (slot >> 1) & 1};   // x, y, z
    for (int ax = 0; ax < 3; ax++) {
        if (slot == 7) { lmin[ax] = w->pl[ax][5]; lmax[ax] = w->pl[ax][4]; }
        else { lmin[ax] = w->pl[ax][bit[ax] * 2]; lmax[ax] = w->pl[ax][bit[ax] * 2 + 1]; }
    }
}

// measurement aid (never defined in the product build): lane-level and wave-level step counts of the wide walk, to tell how much of a
// wave's work is lanes waiting for the slowest ray (tools/divergence_probe.py)
#if defined(GI_EXP_DIV) && defined(__HIP_DEVICE_COMPILE__)
#define GI_DIV(W, k) do { (W).ds[(k)]++; if ((uint32_t)__builtin_ctzll(__ballot(1)) == (threadIdx.x & 63u)) (W).ds[(k) + 1]++; } while (0)
#define GI_DIVN(W, k, n) do { (W).ds[(k)] += (n); if ((uint32_t)__builtin_ctzll(__ballot(1)) == (threadIdx.x & 63u)) (W).ds[(k) + 1] += (n); } while (0)
#else
#define GI_DIV(W, k) do { } while (0)
#define GI_DIVN(W, k, n) do { } while (0)
#endif
// Work a walk actually executes (gi_set_counters(ctx, 2): the streaming kernels count it per lane): walks begun (= tests of the root box), wide
// records visited, child boxes tested from them (one per existing child: together with the root tests these are the reference's
// BoundingBox::intersect calls when nothing is culled), content boxes tested, non-empty leaves met, entity tests.  A record source that does
// not count compiles the ticks to nothing.
struct WalkCnt { uint32_t walks, nodes, child_boxes, cull_tests, leaves, tris, ent_boxes; };
struct NoWalkCnt {
    GI_HDM void tick_walk() const {}
    GI_HDM void tick_node(uint32_t) const {}
    GI_HDM void tick_cull(uint32_t) const {}
    GI_HDM void tick_leaf() const {}
    GI_HDM void tick_tri() const {}
    GI_HDM void tick_ebox(uint32_t) const {}
};
struct GlobalWide : NoWalkCnt {
    static constexpr bool kWide = true;
    static constexpr bool kCoop = false;
    const WNode* g;
    const float* cboxes = nullptr;      // content boxes (null: the walk visits every child whose octant the ray enters)
    const uint32_t* cuse = nullptr;
#ifdef GI_EXP_DIV
    mutable uint32_t ds[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#endif
    template <class F> GI_HDM auto with(int32_t i, F&& f) const { return f(g + i); }
    GI_HDM uint32_t cull(int32_t node, uint32_t m, const Ray& r, const WRay& wr) const { return (cboxes && !wr.plain) ? content_cull(cboxes, cuse, node, m, r, wr) : m; }
};
// walk state: the node, the children of it still to visit (bit k = k-th in order), and the same masks of its ancestors, one
// byte per level, in a 128-bit shift register (16 levels; deeper trees keep the per-node walk)
struct WWalk {
    int32_t node;
    uint32_t m;
    unsigned long long lo, hi;
};
GI_HD void wwalk_push(WWalk& k, int32_t child) { k.hi = (k.hi << 8) | (k.lo >> 56); k.lo = (k.lo << 8) | k.m; k.node = child; }
GI_HD void wwalk_pop(WWalk& k, int32_t parent) { k.m = (uint32_t)(k.lo & 0xffull); k.lo = (k.lo >> 8) | (k.hi << 56); k.hi >>= 8; k.node = parent; }
// The children of a record the ray enters, in its order (wide_hits), without those whose contents it misses (content_cull).  A walk that carries ONE
// ray on a group of lanes (WN::kCoop: the finisher's lone paths, where a bounce is a chain of dependent steps and every step's length counts)
// tests the eight children side by side, a lane each -- the same arithmetic per child (max / min of the same numbers: their order does not matter), a
// ballot instead of eight turns of a loop: ~30 instructions a step instead of ~150.
#if defined(__HIP_DEVICE_COMPILE__)
template <int G> __device__ __forceinline__ unsigned long long group_ballot(bool pred);
template <class WN>
__device__ __forceinline__ uint32_t walk_hits_coop(const WN& W, int32_t node, const Ray& r, const WRay& wr, double tmin0, double tmax0)
{
    constexpr int G = WN::kGroup;
    const int c = (int)(threadIdx.x & 7u);                        // this lane's child slot (lanes 8 .. G-1 of a group repeat the work of 0 .. 7; their votes are not looked at)
    const double o[3] = {r.o.x, r.o.y, r.o.z}, inv[3] = {r.inv.x, r.inv.y, r.inv.z};
    uint32_t exists = 0;
    const bool hit = W.with(node, [&](const WNode* w) {
        exists = w->exists;
        const char* b = reinterpret_cast<const char*>(w);
        const int bit[3] = {c & 1, (c >> 2) & 1, (c >> 1) & 1};   // x = bit 0, z = bit 1, y = bit 2 of a slot
        double t0 = tmin0, t1 = tmax0;
        for (int ax = 0; ax < 3; ax++) {
            const int A = ax * 48, x = back_off(inv[ax]), y = x ^ 8;
            // child 7 has planes of its own (wide_hits: n[ax][2] from the far-side entry, f[ax][2] from the near-side one)
            const int en = c == 7 ? A + 32 + y : A + 16 * bit[ax] + x, ex = c == 7 ? A + 32 + x : A + 16 * bit[ax] + y;
            t0 = fmax(t0, (*reinterpret_cast<const double*>(b + en) - o[ax]) * inv[ax]);
            t1 = fmin(t1, (*reinterpret_cast<const double*>(b + ex) - o[ax]) * inv[ax]);
        }
        return t1 > t0;
    });
    uint32_t m = (uint32_t)(group_ballot<G>(hit) & 0xffull) & exists;
    if (wr.a & 1) m = ((m & 0x55u) << 1) | ((m >> 1) & 0x55u);
    if (wr.a & 2) m = ((m & 0x33u) << 2) | ((m >> 2) & 0x33u);
    if (wr.a & 4) m = ((m & 0x0fu) << 4) | ((m >> 4) & 0x0fu);
    const float* cb = W.cbox_table(node);
    if (m == 0u || !cb || wr.plain) return m;
    // content boxes: lane k looks at the k-th child in the ray's order (content_cull's loop, a turn per lane)
    uint32_t u = W.cuse_of(node);
    if (wr.a & 1) u = ((u & 0x55u) << 1) | ((u >> 1) & 0x55u);
    if (wr.a & 2) u = ((u & 0x33u) << 2) | ((u >> 2) & 0x33u);
    if (wr.a & 4) u = ((u & 0x0fu) << 4) | ((u >> 4) & 0x0fu);
    const uint32_t todo = m & u;
    if (todo == 0u) return m;
    bool miss = false;
    if ((todo >> c) & 1u) {
        const float* b = cb + ((size_t)node * 8 + (size_t)(c ^ wr.a)) * 6;
        double tn = 0.0, tf = wr.tc;
        for (int ax = 0; ax < 3; ax++) {
            const int back = back_off(inv[ax]) ? 3 : 0;
            tn = fmax(tn, ((double)b[ax + back] - o[ax]) * inv[ax]);
            tf = fmin(tf, ((double)b[ax + 3 - back] - o[ax]) * inv[ax]);
        }
        miss = !(tf >= tn);
    }
    return m & ~(uint32_t)(group_ballot<G>(miss) & 0xffull);
}
#endif
template <class WN>
GI_HD uint32_t walk_hits(const WN& W, int32_t node, const Ray& ray, const WRay& wr, double tmin0, double tmax0)
{
#if defined(__HIP_DEVICE_COMPILE__)
    if constexpr (WN::kCoop) return walk_hits_coop(W, node, ray, wr, tmin0, tmax0);
    else
#endif
    {
        uint32_t m = W.with(node, [&](const WNode* w) { W.tick_node(w->exists); return wide_hits(w, ray, wr, tmin0, tmax0); });
        if (m) m = W.cull(node, m, ray, wr);
        return m;
    }
}
// next non-empty leaf whose box the ray touches, or false when the tree is exhausted; leaf = (its parent's record, slot)
template <class WN>
GI_HD bool wwalk_next_leaf(const WN& W, WWalk& k, const Ray& ray, const WRay& wr, double tmin0, double tmax0, int32_t& lnode, int& lslot, int32_t& first, int32_t& cnt)
{
    for (;;) {
        // leave exhausted nodes first, in a loop of its own: the lanes of a wave then reach the box tests below together instead of
        // one lane's ascent making the whole wave step through them
        while (k.m == 0) {
            if (k.node == 0) return false;
            const int32_t par = W.with(k.node, [&](const WNode* w) { return w->parent; });
            wwalk_pop(k, par);
        }
        const int kk = __builtin_ctz(k.m);
        k.m &= k.m - 1;
        const int slot = kk ^ wr.a;
        int32_t ca = 0, cb = 0;
        W.with(k.node, [&](const WNode* w) { ca = w->ca[slot]; cb = w->cb[slot]; return 0; });
        if (cb < 0) {
            GI_DIV(W, 0);
            wwalk_push(k, ca);
            k.m = walk_hits(W, ca, ray, wr, tmin0, tmax0);
            continue;
        }
        lnode = k.node; lslot = slot; first = ca; cnt = cb;
        return true;
    }
}
// One turn of the same walk for callers that interleave the turns of different rays (k_st_shadow): WALK_MOVED = went down one level (the box
// tests of the new node are done), WALK_LEAF = stands on a non-empty leaf, WALK_END = the tree is exhausted.  Ascents are folded into the turn.
enum { WALK_MOVED = 0, WALK_LEAF = 1, WALK_END = 2 };
template <class WN>
GI_HD int wwalk_turn(const WN& W, WWalk& k, const Ray& ray, const WRay& wr, double tmin0, double tmax0, int32_t& lnode, int& lslot, int32_t& first, int32_t& cnt)
{
    while (k.m == 0) {
        if (k.node == 0) return WALK_END;
        const int32_t par = W.with(k.node, [&](const WNode* w) { return w->parent; });
        wwalk_pop(k, par);
    }
    const int kk = __builtin_ctz(k.m);
    k.m &= k.m - 1;
    const int slot = kk ^ wr.a;
    int32_t ca = 0, cb = 0;
    W.with(k.node, [&](const WNode* w) { ca = w->ca[slot]; cb = w->cb[slot]; return 0; });
    if (cb < 0) {
        GI_DIV(W, 0);
        wwalk_push(k, ca);
        k.m = walk_hits(W, ca, ray, wr, tmin0, tmax0);
        return WALK_MOVED;
    }
    lnode = k.node; lslot = slot; first = ca; cnt = cb;
    return WALK_LEAF;
}
template <class WN>
GI_HD bool wwalk_begin(const Scene& S, const WN& W, WWalk& k, const Ray& ray, const WRay& wr, double tmin0, double tmax0)
{
    k.node = 0; k.m = 0; k.lo = 0; k.hi = 0;
    W.tick_walk();
    if (!box_hit(S.root_bmin, S.root_bmax, ray, tmin0, tmax0)) return false;
    k.m = walk_hits(W, 0, ray, wr, tmin0, tmax0);
    return true;
}
// RayTracer::trace over the wide records, one leaf per call: the streaming trace kernel keeps a wave's lanes on different rays and hands a
// finished lane its next ray while the others walk on (k_st_trace), everybody else runs the loop in trace_wide.
struct TraceWalk {
    WRay wr;
    WWalk k;
    bool intersected;
    bool tie;          // two entities at the very same distance were met (trace_wide_step, trace_wide_over)
    double best_d2;
    double uv[2];    // the reference's `glm::dvec2 uv` of trace(), carried across entities (ent_accepts)
};
// a ray that runs exactly along an axis plane may lie IN the face two leaves share and touch both all the way: leaves then do not follow
// each other along it, which the short cuts of the closest-hit walk (trace_wide_over) take for granted -- such a ray walks the plain way.
// trace_wide_begin and the probe ray_leaves_scene ask this one function: the probe is only sound while the two walks agree
GI_HD bool ray_walks_plain(const Ray& ray) { return !(fabs(ray.inv.x) < INFINITY && fabs(ray.inv.y) < INFINITY && fabs(ray.inv.z) < INFINITY); }
template <int FEAT, class WN>
GI_HD bool trace_wide_begin(const Scene& S, const WN& W, const Ray& ray, TraceWalk& t)   // false: the ray misses the scene's box
{
    t.wr = wray_make(ray);
    t.intersected = false; t.tie = false;
    t.wr.plain = ray_walks_plain(ray);
    t.best_d2 = 0; t.uv[0] = 0; t.uv[1] = 0;
    return wwalk_begin(S, W, t.k, ray, t.wr, 0.0, INFINITY);
}
// Two short cuts of the closest-hit walk, both leaving the hit RayTracer::trace returns (include/raytracer.h:446-472) as it is:
//  * the reference ends a walk only when the best hit lies inside the leaf it was found from; a hit found from an earlier leaf (a large
//    entity sticks out of it) lets it walk on to the end of the ray, testing entities that cannot win (it takes a hit only when it is
//    strictly nearer).  Here nothing that begins more than `cut_margin` behind the best hit is looked at: nodes, leaves, entities.
//  * trace_boxes: for an entity of a scene without textures, the box of the part of it INSIDE the leaf (widened): a hit outside the
//    leaf is found again from the leaf it lies in, with the same arithmetic, so asking for it here only brings the answer forward.
// Both widen by 1e-5 of the scene, a hundred times what the float arithmetic of the tree builder can misplace an entity by.  What the second
// could change is WHICH of two entities at exactly the same distance is met first; such a walk (t.tie) is made again the plain way.
// Both hold only while no entity of the scene has an alpha test (flag 2 clear): that test draws per (leaf, entity), so an entity that failed from
// an early leaf is drawn again from every later leaf that refers to it and may win there with a NEARER hit -- behind the cut, or behind the point
// where a leaf-cut opaque box ends the walk.  layout_scene gives such a scene cut_margin = -1 and trace_boxes == leaf_boxes (gi_layout.h).
template <class WN>
GI_HD bool trace_wide_over(const Scene& S, const WN& W, const Ray& ray, TraceWalk& t)   // the walk ended: true when it has to be made again
{
    if (!t.tie || t.wr.plain || S.trace_boxes == S.leaf_boxes) return false;   // (whole boxes: the entities were met in the reference's order anyway)
    t.wr.tc = INFINITY;
    t.intersected = false; t.tie = false; t.wr.plain = true;
    t.best_d2 = 0; t.uv[0] = 0; t.uv[1] = 0;
    return wwalk_begin(S, W, t.k, ray, t.wr, 0.0, INFINITY);
}
// nothing that begins behind the best hit (at squared distance d2) can be nearer: the first short cut above
GI_HD void cut_behind_hit(const Scene& S, WRay& wr, double d2) { if (S.cut_margin >= 0 && !wr.plain) wr.tc = sqrt(d2) + S.cut_margin; }
template <int FEAT, class WN>
GI_HD bool trace_wide_step(const Scene& S, const WN& W, const Ray& ray, const Rng& rng, uint32_t alpha_purpose, TraceWalk& t, HitRec& best)   // false: the walk is over
{
    int32_t lnode = 0, first = 0, cnt = 0;
    int lslot = 0;
    bool term = false;
    if (wwalk_next_leaf(W, t.k, ray, t.wr, 0.0, t.wr.tc, lnode, lslot, first, cnt)) {
    GI_DIV(W, 2);
    W.tick_leaf();
    // an entity beyond the best hit cannot replace it (strict <): without textures its test changes nothing; with them a successful intersect
    // leaves its uv behind for the alpha look-up of the next flat entity (t.uv), so every entity of a visited leaf is still asked
#define GI_TCE ((FEAT & GI_FEAT_TEX) ? INFINITY : t.wr.tc)
    auto test = [&](const LeafTri& g) {
        const int32_t ti = g.tri;
        double u, v;
        V3 hp;
        W.tick_tri();
        if (!ent_hit<FEAT>(g, g.matflags, ray, u, v, hp)) return;
        if (FEAT & GI_FEAT_TEX) ent_uv(S, g, g.matflags, ti, u, v, hp, t.uv[0], t.uv[1]);
        if (!(g.matflags & 2u)) {
            const Mat& m = S.mats[g.matflags >> 3];
            const double alpha = (FEAT & GI_FEAT_TEX) ? mat_alpha(S, m, t.uv[0], t.uv[1]) : m.opacity * 1.0;
            if (!(rng_draw(rng, alpha_purpose, (uint32_t)S.wleaf_id[lnode * 8 + lslot], (uint32_t)ti) < alpha || m.ior != 1)) return;
        }
        double d2 = len2(hp - ray.o);
        if (t.intersected && d2 == t.best_d2 && ti != best.tri) t.tie = true;
        if (!t.intersected || d2 < t.best_d2) {
            best.pos = hp; best.u = u; best.v = v; best.tri = ti; best.mf = g.matflags;
            if (FEAT & GI_FEAT_TEX) { best.tu = t.uv[0]; best.tv = t.uv[1]; }
            t.best_d2 = d2;
            t.intersected = true;
            if (S.cut_margin >= 0 && !t.wr.plain) t.wr.tc = sqrt(d2) + S.cut_margin;   // nothing that begins behind this can be nearer
            double lmin[3], lmax[3];
            W.with(lnode, [&](const WNode* w) { wide_leaf_box(w, lslot, lmin, lmax); return 0; });
            if (box_contains(lmin, lmax, hp)) term = true;
        }
    };
#ifdef GI_WAVE_UNIFORM_LEAVES
    int32_t first_u, cnt_u;
    if (leaf_is_wave_uniform(first, cnt, first_u, cnt_u)) {
        if (S.leaf_boxes) {
            // every lane holds its own ray against the same entity: the record is only fetched when some lane's ray touches the entity's box
            W.tick_ebox((uint32_t)cnt_u);
            for (int32_t j = 0; j < cnt_u; j++) {
                const Box6 bx = leaf_box_scalar(S.trace_boxes + (size_t)(first_u + j) * 6);
                const bool touch = t.wr.plain || !entity_box_missed(bx.b, ray, GI_TCE);
                if (__ballot(touch) == 0ull) continue;
                const LeafTri g = leaf_tri_scalar(S.leaf_tris + first_u + j);
                GI_DIV(W, 4);
                if (touch) test(g);
            }
        } else
            for (int32_t j = 0; j < cnt_u; j++) { GI_DIV(W, 4); test(leaf_tri_scalar(S.leaf_tris + first_u + j)); }
    } else
#endif
    if (S.leaf_boxes && cnt <= 32) {
        // the references whose boxes the ray touches, in leaf order (one or two per leaf: a single record in flight)
        uint32_t m = cnt >= 32 ? 0xffffffffu : ((1u << cnt) - 1u);
        if (!t.wr.plain) m = entity_survivors(S.trace_boxes, first, cnt, ray, GI_TCE);
        W.tick_ebox((uint32_t)cnt);
        while (m) {
            const int j = __builtin_ctz(m);
            m &= m - 1;
            GI_DIV(W, 6);
            test(S.leaf_tris[first + j]);
        }
    } else
        for (int32_t j = 0; j < cnt; j += 2) {
            const LeafTri g0 = S.leaf_tris[first + j];
            const LeafTri g1 = S.leaf_tris[first + (j + 1 < cnt ? j + 1 : j)];
            GI_DIV(W, 6);
            test(g0);
            if (j + 1 < cnt) { GI_DIV(W, 6); test(g1); }
        }
#undef GI_TCE
    if (!term) return true;
    }
    return trace_wide_over(S, W, ray, t);
}
template <int FEAT, class WN>
GI_HD bool trace_wide(const Scene& S, const WN& W, const Ray& ray, const Rng& rng, uint32_t alpha_purpose, HitRec& best)
{
    TraceWalk t;
    if (!trace_wide_begin<FEAT>(S, W, ray, t)) return false;
    while (trace_wide_step<FEAT>(S, W, ray, rng, alpha_purpose, t, best)) { }
    return t.intersected;
}
// Does the ray leave the scene without its walk ever standing on a non-empty leaf?  The first turns of trace_wide's own walk -- the same WRay
// (trace_wide_begin, `plain` for an axis-parallel ray included), the same box tests in the same order (wwalk_begin, wwalk_turn: walk_hits and the
// content boxes W carries), tc = INFINITY as trace_wide has it until its first hit, and a hit is only ever found from a leaf -- so when the walk
// ends here without a leaf, trace_wide over the same W meets no leaf either: it tests no entity, draws no alpha number, leaves no uv behind and
// returns false.  true is therefore a SUFFICIENT condition for a miss; false (a leaf was met, or max_turns turns did not end the walk) says nothing
// and the ray is traced as usual.  No entity is looked at here.  k_st_shade asks this about the next ray of a vertex: in an open scene most
// reflected rays are decided within a few records and never become a path record, a queue entry, a sort key or an item of the trace stage.
template <class WN>
GI_HD bool ray_leaves_scene(const Scene& S, const WN& W, const Ray& ray, int max_turns)
{
    WRay wr = wray_make(ray);
    wr.plain = ray_walks_plain(ray);
    WWalk k;
    if (!wwalk_begin(S, W, k, ray, wr, 0.0, INFINITY)) return true;   // misses the scene's box
    for (int turn = 0; turn < max_turns; turn++) {
        int32_t lnode = 0, first = 0, cnt = 0;
        int lslot = 0;
        const int r = wwalk_turn(W, k, ray, wr, 0.0, INFINITY, lnode, lslot, first, cnt);
        if (r == WALK_END) return true;
        if (r == WALK_LEAF) return false;
    }
    return false;
}
// RayTracer::visible over the wide records, one leaf per call (k_st_shadow hands idle lanes new shadow rays; everybody else loops in visible_wide)
struct VisWalk {
    WRay wr;
    WWalk k;
    double tmax;
};
// the any-hit walk's cut for a segment of squared length mt: a blocker lies before the light, 0 < |hit - o|^2 < mt
GI_HD double shadow_cut(double mt) { return sqrt(mt) * (1.0 + 1e-9); }
template <int FEAT, class WN>
GI_HD bool visible_wide_begin(const Scene& S, const WN& W, const Ray& ray, double mt, VisWalk& v)   // false: the segment misses the scene's box
{
    v.wr = wray_make(ray);
    v.tmax = sqrt(mt) - GI_SHADOW_BIAS;
    v.wr.tc = shadow_cut(mt);
    return wwalk_begin(S, W, v.k, ray, v.wr, 0.0, v.tmax);
}
enum { VIS_DONE = 0, VIS_MORE = 1, VIS_BLOCKED = 2 };
// does anything in this leaf block the segment?  (the triangle loop of RayTracer::visible for one leaf of the walk)
template <int FEAT, class WN>
GI_HD bool visible_leaf_blocks(const Scene& S, const WN& W, const Ray& ray, double mt, const Rng& rng, uint32_t light_index, int32_t lnode, int lslot, int32_t first, int32_t cnt, const double* boxes)
{
    GI_DIV(W, 2);
    W.tick_leaf();
    auto blocks = [&](const LeafTri& g) -> bool {
        const int32_t ti = g.tri;
        double u, vv;
        V3 hp;
        W.tick_tri();
        if (!ent_hit<FEAT>(g, g.matflags, ray, u, vv, hp)) return false;
        if (!(g.matflags & 2u)) {
            const Mat& m = S.mats[g.matflags >> 3];
            double alpha = m.opacity * 1.0;
            if (FEAT & GI_FEAT_TEX) { double cu = 0, cv = 0; ent_uv(S, g, g.matflags, ti, u, vv, hp, cu, cv); alpha = mat_alpha(S, m, cu, cv); }
            if (!(rng_draw(rng, P_SHADOW_ALPHA | (light_index << 8), (uint32_t)S.wleaf_id[lnode * 8 + lslot], (uint32_t)ti) < alpha || m.ior != 1)) return false;
        }
        const double ts = len2(hp - ray.o);
        return (ts < mt) && (ts > 0);
    };
#ifdef GI_WAVE_UNIFORM_LEAVES
    int32_t first_u, cnt_u;
    if (leaf_is_wave_uniform(first, cnt, first_u, cnt_u)) {
        bool hit = false;
        const double tc = shadow_cut(mt);
        if (boxes) W.tick_ebox((uint32_t)cnt_u);
        for (int32_t j = 0; j < cnt_u; j++) {     // wave-uniform trip count: the record address stays scalar
            bool touch = !hit;
            if (boxes) {                          // (wave-uniform branch) fetch the record only when a lane that still looks for a blocker touches the entity's box
                const Box6 bx = leaf_box_scalar(boxes + (size_t)(first_u + j) * 6);
                touch = touch && !entity_box_missed(bx.b, ray, tc);
                if (__ballot(touch) == 0ull) continue;
            }
            const LeafTri g = leaf_tri_scalar(S.leaf_tris + first_u + j);
            GI_DIV(W, 4);
            if (touch) hit = blocks(g);
            if (__ballot(!hit) == 0ull) break;
        }
        return hit;
    }
#endif
    if (boxes && cnt <= 32) {
        uint32_t m = entity_survivors(boxes, first, cnt, ray, shadow_cut(mt));
        W.tick_ebox((uint32_t)cnt);
        while (m) {
            const int j = __builtin_ctz(m);
            m &= m - 1;
            GI_DIV(W, 6);
            if (blocks(S.leaf_tris[first + j])) return true;
        }
        return false;
    }
    for (int32_t j = 0; j < cnt; j++) {
        GI_DIV(W, 6);
        if (blocks(S.leaf_tris[first + j])) return true;
    }
    return false;
}
template <int FEAT, class WN>
GI_HD int visible_wide_step(const Scene& S, const WN& W, const Ray& ray, double mt, const Rng& rng, uint32_t light_index, VisWalk& v)
{
    int32_t lnode = 0, first = 0, cnt = 0;
    int lslot = 0;
    if (!wwalk_next_leaf(W, v.k, ray, v.wr, 0.0, v.tmax, lnode, lslot, first, cnt)) return VIS_DONE;
    return visible_leaf_blocks<FEAT>(S, W, ray, mt, rng, light_index, lnode, lslot, first, cnt, S.leaf_boxes) ? VIS_BLOCKED : VIS_MORE;
}
// what visible() asks of the medium once nothing solid blocks the segment: include/raytracer.h:308-316 (the reference bounds this march by the SQUARED length)
template <int FEAT>
GI_HD bool visible_through_fog(const Scene& S, const Ray& ray, double mt, const Rng& rng, uint32_t light_index)
{
    if ((FEAT & GI_FEAT_FOG) && S.n_fog > 0) {
        double tmin = 0, tmx = mt;
        if (atmosphere_bounds(S, ray, tmin, tmx)) {
            V3 fh, fc;
            if (raymarch(S, ray, fh, fc, tmin, tmx, rng, P_FOG_SHADOW + 16u * light_index)) return false;
        }
    }
    return true;
}
template <int FEAT, class WN>
GI_HD bool visible_wide(const Scene& S, const WN& W, const Ray& ray, double mt, const Rng& rng, uint32_t light_index)
{
    VisWalk v;
    if (visible_wide_begin<FEAT>(S, W, ray, mt, v)) {
        for (;;) {
            const int r = visible_wide_step<FEAT>(S, W, ray, mt, rng, light_index, v);
            if (r == VIS_BLOCKED) return false;
            if (r == VIS_DONE) break;
        }
    }
    return visible_through_fog<FEAT>(S, ray, mt, rng, light_index);
}

#if defined(__HIPCC__)
// ---- one ray per WAVE (the finisher's last stages: a handful of depth-65 paths, each a chain of dependent bounces).  All 64 lanes
// carry the same ray and walk the nodes together; at a leaf every lane tests its own triangle.  The reference's sequential loop
// (include/raytracer.h:447-468: take a hit when it is the first or strictly nearer than the best so far; remember if any taken hit
// lay inside the leaf's box) is reproduced from an exclusive prefix minimum over the lanes: lane j "takes" its hit exactly when
// d2_j < min(best before the leaf, d2_i of the accepted hits i < j).  The last taking lane holds the final best.
// The lanes of a wave form 64 / G groups of G lanes (G = WN::kGroup: 64 or 16); a group carries one ray.  Groups walk different rays through
// the same loops (a group whose ray needs fewer turns sits them out), every collective stays inside the group: shuffles of width G, ballots
// masked to the group's lanes.
template <int G> __device__ __forceinline__ unsigned long long group_ballot(bool pred)
{
    const unsigned long long b = __ballot(pred);
    if constexpr (G == 64) return b;
    else return (b >> ((threadIdx.x & 63u) & ~(unsigned)(G - 1))) & ((1ull << G) - 1ull);
}
template <int FEAT, class WN>
__device__ __forceinline__ bool trace_wide_coop(const Scene& S, const WN& W, const Ray& ray, const Rng& rng, uint32_t alpha_purpose, HitRec& best)
{
    if constexpr ((FEAT & GI_FEAT_TEX) != 0) return trace_wide<FEAT>(S, W, ray, rng, alpha_purpose, best);   // the carried uv is sequential: every lane walks alone
    else {
    constexpr int G = WN::kGroup;
    const int lane = (int)(threadIdx.x & 63u), gl = lane & (G - 1), gb = lane - gl;
    WRay wr = wray_make(ray);
    bool intersected = false;
    double best_d2 = 0;
    WWalk k;
    if (!wwalk_begin(S, W, k, ray, wr, 0.0, INFINITY)) return false;
    for (;;) {
        int32_t lnode = 0, first = 0, cnt = 0;
        int lslot = 0;
        if (!wwalk_next_leaf(W, k, ray, wr, 0.0, wr.tc, lnode, lslot, first, cnt)) break;
        bool term = false;
        double lmin[3], lmax[3];
        W.with(lnode, [&](const WNode* w) { wide_leaf_box(w, lslot, lmin, lmax); return 0; });
        for (int32_t base = 0; base < cnt; base += G) {
            const int32_t j = base + gl;
            bool ok = false;
            double u = 0, v = 0, d2 = INFINITY;
            V3 hp = v3(0, 0, 0);
            int32_t ti = 0;
            uint32_t mf = 0;
            if (j < cnt) {
                const LeafTri g = S.leaf_tris[first + j];
                ti = g.tri; mf = g.matflags;
                ok = ent_accepts<FEAT>(S, g, ray, rng, alpha_purpose, S.wleaf_id + lnode * 8 + lslot, nullptr, u, v, hp);
                if (ok) d2 = len2(hp - ray.o);
            }
            double pm = ok ? d2 : INFINITY;   // inclusive prefix minimum over the group's lanes
            for (int off = 1; off < G; off <<= 1) {
                const double t = __shfl_up(pm, (unsigned)off, G);
                if (gl >= off) pm = fmin(pm, t);
            }
            double ex = __shfl_up(pm, 1u, G);
            if (gl == 0) ex = INFINITY;
            if (intersected) ex = fmin(ex, best_d2);
            const bool take = ok && d2 < ex;
            const unsigned long long tm = group_ballot<G>(take);
            if (tm != 0ull) {
                if (group_ballot<G>(take && box_contains(lmin, lmax, hp)) != 0ull) term = true;
                const int last = gb + 63 - __clzll((long long)tm);
                best.pos = v3(__shfl(hp.x, last), __shfl(hp.y, last), __shfl(hp.z, last));
                best.u = __shfl(u, last); best.v = __shfl(v, last);
                best.tri = __shfl(ti, last); best.mf = (uint32_t)__shfl((int)mf, last);
                best_d2 = __shfl(d2, last);
                intersected = true;
                cut_behind_hit(S, wr, best_d2);   // (wr.plain stays false here: wray_make, and this walk has no re-walk) the reference walks on to the end of the ray when the hit was found from an earlier leaf -- a lone path inside a glass body does that at every bounce
            }
        }
        if (term) break;
    }
    return intersected;
    }
}
template <int FEAT, class WN>
__device__ __forceinline__ bool visible_wide_coop(const Scene& S, const WN& W, const Ray& ray, double mt, const Rng& rng, uint32_t light_index)
{
    if constexpr ((FEAT & GI_FEAT_TEX) != 0) return visible_wide<FEAT>(S, W, ray, mt, rng, light_index);
    else {
    constexpr int G = WN::kGroup;
    const int gl = (int)(threadIdx.x & (unsigned)(G - 1));
    WRay wr = wray_make(ray);
    const double tmax = sqrt(mt) - GI_SHADOW_BIAS;
    wr.tc = shadow_cut(mt);
    WWalk k;
    if (wwalk_begin(S, W, k, ray, wr, 0.0, tmax)) {
        for (;;) {
            int32_t lnode = 0, first = 0, cnt = 0;
            int lslot = 0;
            if (!wwalk_next_leaf(W, k, ray, wr, 0.0, tmax, lnode, lslot, first, cnt)) break;
            for (int32_t base = 0; base < cnt; base += G) {
                const int32_t j = base + gl;
                const bool blocks = j < cnt && ent_blocks<FEAT>(S, S.leaf_tris[first + j], ray, mt, rng, light_index, S.wleaf_id + lnode * 8 + lslot);
                if (group_ballot<G>(blocks) != 0ull) return false;
            }
        }
    }
    return visible_through_fog<FEAT>(S, ray, mt, rng, light_index);
    }
}
#else
template <int FEAT, class WN> bool trace_wide_coop(const Scene&, const WN&, const Ray&, const Rng&, uint32_t, HitRec&) { return false; }        // host builds never
template <int FEAT, class WN> bool visible_wide_coop(const Scene&, const WN&, const Ray&, double, const Rng&, uint32_t) { return false; }    // select kCoop sources
#endif

// RayTracer::trace.  Leaves are met in the order the reference's t0-sorted list has them because the hit/skip links of a
// direction octant visit the children of every node front to back; the walk stops after the first leaf that contains a new
// nearest hit.  Control flow is "while-while": an inner loop walks nodes until THIS lane stands on a non-empty leaf, then the
// leaf's triangles are tested; the 64 lanes of a wave therefore do their node steps together and their triangle tests together
// instead of one lane's triangle loop stalling 63 lanes that want to take a node step.
template <int FEAT, class Nodes>
GI_HD bool trace_nodes(const Scene& S, const Nodes& N, const Ray& ray, const Rng& rng, uint32_t alpha_purpose, HitRec& best, Counters* c)
{
    if constexpr (Nodes::kWide) {
        if constexpr (Nodes::kCoop) return trace_wide_coop<FEAT>(S, N, ray, rng, alpha_purpose, best);
        else return trace_wide<FEAT>(S, N, ray, rng, alpha_purpose, best);
    }
    else {
    const int oct = dir_octant(ray);
    bool intersected = false;
    double best_d2 = 0;
    double cu = 0, cv = 0;
    int32_t node = 0;
    if (c) c->traces++;
    for (;;) {
        // ---- next non-empty leaf the ray touches
        int32_t first = 0, cnt = 0, leaf = -1;
        double lmin[3], lmax[3];
        while (node < S.n_node) {
            NodeView nd;
            N.fetch(node, oct, nd);
            if (c) c->v_trace++;
            if (!box_hit(nd.bmin, nd.bmax, ray, 0.0, INFINITY)) { node = nd.skip; continue; }
            if (nd.n_ref < 0) { node = nd.hit; continue; }
            if (nd.n_ref == 0) { node = nd.skip; continue; }
            leaf = node; first = nd.first_ref; cnt = nd.n_ref;
            lmin[0] = nd.bmin[0]; lmin[1] = nd.bmin[1]; lmin[2] = nd.bmin[2];
            lmax[0] = nd.bmax[0]; lmax[1] = nd.bmax[1]; lmax[2] = nd.bmax[2];
            node = nd.skip;
            break;
        }
        if (leaf < 0) break;
        // ---- its triangles, two records in flight at a time (the fetch of the second overlaps the test of the first)
        bool term = false;
        auto test = [&](const LeafTri& g) {
            const int32_t ti = g.tri;
            double u, v;
            V3 hp;
            if (c) c->tri++;
            if (!ent_hit<FEAT>(g, g.matflags, ray, u, v, hp)) return;
            if (FEAT & GI_FEAT_TEX) ent_uv(S, g, g.matflags, ti, u, v, hp, cu, cv);
            if (!(g.matflags & 2u)) {
                const Mat& m = S.mats[g.matflags >> 3];
                const double alpha = (FEAT & GI_FEAT_TEX) ? mat_alpha(S, m, cu, cv) : m.opacity * 1.0;
                if (!(rng_draw(rng, alpha_purpose, (uint32_t)N.leaf_id(leaf), (uint32_t)ti) < alpha || m.ior != 1)) return;
            }
            double d2 = len2(hp - ray.o);
            if (!intersected || d2 < best_d2) {
                best.pos = hp; best.u = u; best.v = v; best.tri = ti; best.mf = g.matflags;
                if (FEAT & GI_FEAT_TEX) { best.tu = cu; best.tv = cv; }
                best_d2 = d2;
                intersected = true;
                if (box_contains(lmin, lmax, hp)) term = true;
            }
        };
        for (int32_t k = 0; k < cnt; k += 2) {
            const LeafTri g0 = S.leaf_tris[first + k];
            const LeafTri g1 = S.leaf_tris[first + (k + 1 < cnt ? k + 1 : k)];
            test(g0);
            if (k + 1 < cnt) test(g1);
        }
        if (term) break;
    }
    return intersected;
    }
}
GI_HD bool trace(const Scene& S, const Ray& ray, const Rng& rng, uint32_t alpha_purpose, HitRec& best, Counters* c)
{
    best.tu = 0; best.tv = 0;
    if (S.wnodes && !c) {   // the work counters count the reference's per-node box tests: counted runs take the per-node walk
        GlobalWide W;
        W.g = S.wnodes; W.cboxes = S.tcboxes; W.cuse = S.tcuse;   // a closest-hit walk and nothing else: its own content boxes
        return S.n_tex > 0 ? trace_nodes<7>(S, W, ray, rng, alpha_purpose, best, nullptr) : trace_nodes<3>(S, W, ray, rng, alpha_purpose, best, nullptr);
    }
    GlobalNodes N;
    N.g = S.tnodes;
    return S.n_tex > 0 ? trace_nodes<7>(S, N, ray, rng, alpha_purpose, best, c) : trace_nodes<3>(S, N, ray, rng, alpha_purpose, best, c);
}

// RayTracer::visible: any accepted hit with 0 < |hit-o|^2 < mt among the entities of every leaf the segment touches.
template <int FEAT, class Nodes>
GI_HD bool visible_nodes(const Scene& S, const Nodes& N, const Ray& ray, double mt, const Rng& rng, uint32_t light_index, Counters* c)
{
    if constexpr (Nodes::kWide) {
        if constexpr (Nodes::kCoop) return visible_wide_coop<FEAT>(S, N, ray, mt, rng, light_index);
        else return visible_wide<FEAT>(S, N, ray, mt, rng, light_index);
    }
    else {
    const int oct = dir_octant(ray);
    const double tmax = sqrt(mt) - GI_SHADOW_BIAS;
    int32_t node = 0;
    if (c) c->shadows++;
    for (;;) {
        int32_t first = 0, cnt = 0, leaf = -1;
        while (node < S.n_node) {
            NodeView nd;
            N.fetch(node, oct, nd);
            if (c) c->v_shadow++;
            if (!box_hit(nd.bmin, nd.bmax, ray, 0.0, tmax)) { node = nd.skip; continue; }
            if (nd.n_ref < 0) { node = nd.hit; continue; }
            if (nd.n_ref == 0) { node = nd.skip; continue; }
            leaf = node; first = nd.first_ref; cnt = nd.n_ref;
            node = nd.skip;
            break;
        }
        if (leaf < 0) break;
        for (int32_t k = 0; k < cnt; k++) {
            const LeafTri& g = S.leaf_tris[first + k];
            const int32_t ti = g.tri;
            double u, v;
            V3 hp;
            if (c) c->tri++;
            if (!ent_hit<FEAT>(g, g.matflags, ray, u, v, hp)) continue;
            if (!(g.matflags & 2u)) {
                const Mat& m = S.mats[g.matflags >> 3];
                double alpha = m.opacity * 1.0;
                if (FEAT & GI_FEAT_TEX) { double cu = 0, cv = 0; ent_uv(S, g, g.matflags, ti, u, v, hp, cu, cv); alpha = mat_alpha(S, m, cu, cv); }
                if (!(rng_draw(rng, P_SHADOW_ALPHA | (light_index << 8), (uint32_t)N.leaf_id(leaf), (uint32_t)ti) < alpha || m.ior != 1)) continue;
            }
            double ts = len2(hp - ray.o);
            if ((ts < mt) && (ts > 0)) return false;
        }
    }
    if ((FEAT & GI_FEAT_FOG) && S.n_fog > 0) {   // include/raytracer.h:308-316 (the reference bounds this march by the SQUARED length)
        double tmin = 0, tmx = mt;
        if (atmosphere_bounds(S, ray, tmin, tmx)) {
            V3 fh, fc;
            if (raymarch(S, ray, fh, fc, tmin, tmx, rng, P_FOG_SHADOW + 16u * light_index)) return false;
        }
    }
    return true;
    }
}
GI_HD bool visible(const Scene& S, const Ray& ray, double mt, const Rng& rng, uint32_t light_index, Counters* c)
{
    if (S.wnodes && !c) {
        GlobalWide W;
        W.g = S.wnodes; W.cboxes = S.cboxes; W.cuse = S.cuse;
        return S.n_tex > 0 ? visible_nodes<7>(S, W, ray, mt, rng, light_index, nullptr) : visible_nodes<3>(S, W, ray, mt, rng, light_index, nullptr);
    }
    GlobalNodes N;
    N.g = S.tnodes;
    return S.n_tex > 0 ? visible_nodes<7>(S, N, ray, mt, rng, light_index, c) : visible_nodes<3>(S, N, ray, mt, rng, light_index, c);
}

// ------------------------------------------------------------------------------------------------ diagnostics (parity tests)
// The sequence of non-empty leaves the walk of trace() meets for a ray, as canonical (pre-order) node indices, without the early
// stop of trace: what Octree::intersectSorted (include/octree.cpp:188-211,285-313) returns as its t0-sorted list.  Runs the very
// walk the kernels run (wide records when the scene has them, else the per-node links).
GI_HD int leaf_order(const Scene& S, const Ray& ray, int cap, int32_t* out)
{
    int n = 0;
    if (S.wnodes) {
        GlobalWide W;
        W.g = S.wnodes;
        const WRay wr = wray_make(ray);
        WWalk k;
        if (!wwalk_begin(S, W, k, ray, wr, 0.0, INFINITY)) return 0;
        for (;;) {
            int32_t lnode = 0, first = 0, cnt = 0;
            int lslot = 0;
            if (!wwalk_next_leaf(W, k, ray, wr, 0.0, INFINITY, lnode, lslot, first, cnt)) break;
            if (n < cap) out[n] = S.wleaf_id[lnode * 8 + lslot];
            n++;
        }
        return n;
    }
    GlobalNodes N;
    N.g = S.tnodes;
    const int oct = dir_octant(ray);
    int32_t node = 0;
    while (node < S.n_node) {
        NodeView nd;
        N.fetch(node, oct, nd);
        if (!box_hit(nd.bmin, nd.bmax, ray, 0.0, INFINITY)) { node = nd.skip; continue; }
        if (nd.n_ref < 0) { node = nd.hit; continue; }
        if (nd.n_ref > 0) { if (n < cap) out[n] = N.leaf_id(node); n++; }
        node = nd.skip;
    }
    return n;
}
// Known-answer access to the scalar building blocks (include/util.h:100-188, include/util.cpp:27-107) and to the libm calls the path
// makes, as the device evaluates them.  in: up to 9 doubles, out: 3 doubles.
enum { KAT_FAST_POW = 0, KAT_FAST_PRECISE_POW = 1, KAT_HEMI_COS_N = 2, KAT_SAMPLE_PHONG = 3, KAT_SPHERE_CAP = 4, KAT_UNIT_VEC = 5, KAT_REFR = 6, KAT_REFLECT = 7, KAT_RNG = 8,
       KAT_SIN = 16, KAT_COS = 17, KAT_ACOS = 18, KAT_ASIN = 19, KAT_ATAN2 = 20, KAT_POW = 21, KAT_SQRT = 22 };
GI_HD void kat_eval(int what, const double* in, double* out)
{
    V3 r = v3(0, 0, 0);
    switch (what) {
    case KAT_FAST_POW: r.x = fast_pow(in[0], in[1]); break;
    case KAT_FAST_PRECISE_POW: r.x = fast_precise_pow(in[0], in[1]); break;
    case KAT_HEMI_COS_N: r = hemi_cos_n(ld3(in), (float)in[3], (float)in[4], in[5]); break;
    case KAT_SAMPLE_PHONG: r = sample_phong(ld3(in), in[3], in[4], in[5]); break;
    case KAT_SPHERE_CAP: r = sphere_cap_cos(ld3(in), (float)in[3], (float)in[4], in[5], in[6]); break;
    case KAT_UNIT_VEC: r = random_unit_vec(in[0], in[1]); break;
    case KAT_REFR: r = refr(ld3(in), ld3(in + 3), in[6]); break;
    case KAT_REFLECT: r = reflect(ld3(in), ld3(in + 3)); break;
    case KAT_RNG: {   // the counter RNG (a-16): seed hi, seed lo, stream, depth, purpose, a, b -> draw, stream key hi, stream key lo
        Rng g = rng_make(((uint64_t)(uint32_t)in[0] << 32) | (uint64_t)(uint32_t)in[1], (uint32_t)in[2]);
        g.depth = (uint32_t)in[3];
        r.x = rng_draw(g, (uint32_t)in[4], (uint32_t)in[5], (uint32_t)in[6]);
        r.y = (double)(uint32_t)(g.hs >> 32); r.z = (double)(uint32_t)g.hs;
        break;
    }
    case KAT_SIN: r.x = sin(in[0]); break;
    case KAT_COS: r.x = cos(in[0]); break;
    case KAT_ACOS: r.x = acos(in[0]); break;
    case KAT_ASIN: r.x = asin(in[0]); break;
    case KAT_ATAN2: r.x = atan2(in[0], in[1]); break;
    case KAT_POW: r.x = pow(in[0], in[1]); break;
    case KAT_SQRT: r.x = sqrt(in[0]); break;
    default: break;
    }
    out[0] = r.x; out[1] = r.y; out[2] = r.z;
}
