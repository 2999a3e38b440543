// gi_gather.h -- the photon gather (RayTracer::samplePhotons), the part that compiles for host and device.  Included by gi_device.h inside
// namespace gi, behind the vectors, the boxes and the Scene tables; the wave-level forms and the gather kernels are in gi_gather.inc.
//
// One selection, three ways of bringing candidates to it.  The selection is written once, here: the float key ((float)g_d2), a photon's
// contribution (g_contrib), the sum below tau and the tie group at tau (g_add_lt, g_add_eq), the end rule (g_end) and the exact pass for float
// keys tied across rank 32 (g_exact).  The forms differ in how a candidate reaches it:
//   a lane per query with an LDS heap     gather_in_leaf, here (k_gather, the megakernel, the finisher, the waves of k_st_gather that span too many leaves)
//   a wave of queries, leaf by leaf       k_st_gather, gi_gather.inc: a leaf's candidates staged in LDS for its run of lanes, tau by ksel_tau
//   a wave per query                      gather_wave, gi_gather.inc: a candidate per lane
// Every form takes its sums in candidate order, so the three return the same bits (tests/test_gpu_gather_kernels.py).

// Lane-private max-heap of GI_GATHER_K *float* keys; element i of this lane lives at hp[i * stride] (LDS, bank-conflict free
// for any per-lane i because the lane index is the fastest-varying address component).  Keys are (float)d2: rounding is
// monotone, so key(a) < key(b) implies d2(a) < d2(b); only candidates whose key EQUALS the 32nd key are ambiguous and those
// are resolved with exact doubles below.  8 KB of LDS per wave instead of 16.
struct Heap { float* hp; int stride; int n; };
GI_HD void heap_push(Heap& h, float x)
{
    int i = h.n++;
    while (i > 0) {
        int p = (i - 1) >> 1;
        float pv = h.hp[p * h.stride];
        if (pv >= x) break;
        h.hp[i * h.stride] = pv;
        i = p;
    }
    h.hp[i * h.stride] = x;
}
GI_HD void heap_replace_root(Heap& h, float x)
{
    int i = 0;
    for (;;) {
        int l = 2 * i + 1;
        if (l >= h.n) break;
        int cidx = l;
        float cv = h.hp[l * h.stride];
        if (l + 1 < h.n) {
            float rv = h.hp[(l + 1) * h.stride];
            if (rv > cv) { cidx = l + 1; cv = rv; }
        }
        if (cv <= x) break;
        h.hp[i * h.stride] = cv;
        i = cidx;
    }
    h.hp[i * h.stride] = x;
}
GI_HD bool boxes_touch(const double* amin, const double* amax, const double* qmin, const double* qmax)  // include/bbox.h:33-38
{
    return (amin[0] <= qmax[0] && amax[0] >= qmin[0]) && (amin[1] <= qmax[1] && amax[1] >= qmin[1]) && (amin[2] <= qmax[2] && amax[2] >= qmin[2]);
}
// RayTracer::samplePhotons(pos, dir, 32): candidates = photons of every leaf touching the (+-EPSILON) box of the leaf that
// contains pos; the 32 nearest of them; sum col*dot(photon.dir, dir) / (pi * r32^2).
//   pass 1: 32nd smallest float key tau (heap);   pass 2: exact sums of everything with key < tau, and of the key == tau group;
//   if the tie group is larger than what is still needed (float ties straddling rank 32: rare) pass 3 picks the needed ones by
//   exact distance.
// PhotonMap::Node::getBounds (include/photonMap.cpp:115-134): the leaf whose half-open box contains pos, or -1.  The children
// are the 8 octants around `mid`, so the only child that can contain pos is the one on pos's side of mid on every axis
// (x = bit0, z = bit1, y = bit2); its contains() test is still made, because the upper children end at mid + .5*extent, which
// may fall an ulp short of the parent's box.
GI_HD int32_t gather_find_leaf(const Scene& S, V3 pos)
{
    if (S.n_pnode <= 0) return -1;
    int32_t node = 0;
    if (S.pn_planes) {
        // one record per level: the child's box is made of the parent's planes (checked bit for bit against the children's stored boxes
        // when the map was laid out), so the child's own record is only fetched to go on
        for (;;) {
            const PNode& nd = S.pnodes[node];
            if (nd.first_child < 0) return node;
            const int bx = pos.x >= nd.mid[0] ? 1 : 0, bz = pos.z >= nd.mid[2] ? 1 : 0, by = pos.y >= nd.mid[1] ? 1 : 0;
            const int k = bx | (bz << 1) | (by << 2);
            const int bit[3] = {bx, by, bz};
            double lo[3], hi[3];
            for (int ax = 0; ax < 3; ax++) {
                if (k == 7) { lo[ax] = nd.mid[ax]; hi[ax] = nd.bmax[ax]; }
                else if (bit[ax]) { lo[ax] = nd.u.in.lo2[ax]; hi[ax] = nd.u.in.hi2[ax]; }
                else { lo[ax] = nd.bmin[ax]; hi[ax] = nd.mid[ax]; }
            }
            if (!box_contains(lo, hi, pos)) return -1;   // no child contains pos: box of -inf, nothing is collected
            node = nd.first_child + k;
        }
    }
    while (S.pnodes[node].first_child >= 0) {
        const PNode& nd = S.pnodes[node];
        const int k = (pos.x >= nd.mid[0] ? 1 : 0) | (pos.z >= nd.mid[2] ? 2 : 0) | (pos.y >= nd.mid[1] ? 4 : 0);
        const int32_t ch = nd.first_child + k;
        const PNode& cn = S.pnodes[ch];
        if (!box_contains(cn.bmin, cn.bmax, pos)) return -1;   // no child contains pos: box of -inf, nothing is collected
        node = ch;
    }
    return node;
}
// The same descent for the bulk of the queries (k_st_compact: one per gather query of a pass).  PhotonMap::Node::getBounds picks the child by comparing the
// position with the split point and then asks whether that child's box contains it (include/photonMap.cpp:115-134).  The child's box is made of the
// parent's planes, so the answer can only be "no" when the position lies within rounding (an ulp of the box's size) of the split point or of the map's own
// faces -- the three forms of "the middle" the reference computes differ in the last bit.  A query that keeps clear of every split plane on its way by
// 1e-12 of the map's extent, and of the map's faces, is inside every box on the way: it needs the 32-byte split records only (2.3 MB for the benchmark's
// map: L2-resident, where the 128-byte nodes are not).  Any other query, and every query of a map without these tables, gets -2: "ask gather_find_leaf".
// Same leaf by construction.
GI_HD int32_t gather_find_leaf_fast(const Scene& S, V3 pos)
{
    if (!S.pdescent) return -2;
    const double p[3] = {pos.x, pos.y, pos.z};
    double ext = 0.0;
    for (int ax = 0; ax < 3; ax++) ext = fmax(ext, S.pmap_bmax[ax] - S.pmap_bmin[ax]);
    const double eps = 1e-12 * ext;
    for (int ax = 0; ax < 3; ax++) if (!(p[ax] > S.pmap_bmin[ax] + eps && p[ax] < S.pmap_bmax[ax] - eps)) return -2;
    int32_t node = 0;
    if (S.pjump) {
        // the first GI_PJUMP_BITS levels at once: the cell of a grid over the map's box the position lies in names the node its descent reaches (the split
        // planes of those levels were checked against the grid's when the table was made: within 1e-12 of the extent); a position within 4 eps of a cell's
        // face starts at the root instead
        int cell[3];
        bool clear = true;
        for (int ax = 0; ax < 3; ax++) {
            const double f = (p[ax] - S.pmap_bmin[ax]) * S.pjump_inv[ax];
            int i = (int)f;
            i = i < 0 ? 0 : (i > GI_PJUMP_N - 1 ? GI_PJUMP_N - 1 : i);
            const double lo = S.pmap_bmin[ax] + (double)i * S.pjump_cell[ax];
            if (!(p[ax] - lo > 4.0 * eps && lo + S.pjump_cell[ax] - p[ax] > 4.0 * eps)) clear = false;
            cell[ax] = i;
        }
        if (clear) node = S.pjump[(cell[1] * GI_PJUMP_N + cell[2]) * GI_PJUMP_N + cell[0]];
    }
    for (;;) {
        const PDescent nd = S.pdescent[node];
        if (nd.first_child < 0) return node;
        int k = 0;
        for (int ax = 0; ax < 3; ax++) {
            const double dlt = p[ax] - nd.mid[ax];
            if (!(fabs(dlt) > eps)) return -2;                       // too close to a split plane to skip the box test (NaN lands here too)
            if (dlt > 0.0) k |= ax == 0 ? 1 : (ax == 2 ? 2 : 4);     // x = bit 0, z = bit 1, y = bit 2
        }
        node = nd.first_child + k;
    }
}
// The leaf around a position as every query of the stream passes looks it up: the quick descent, the full one where that declines
GI_HD int32_t gather_leaf_of(const Scene& S, V3 pos)
{
    const int32_t leaf = gather_find_leaf_fast(S, pos);
    return leaf == -2 ? gather_find_leaf(S, pos) : leaf;
}
// The sort key of a gather query (k_st_compact's gather queue, gi_debug_gather_pass): the rank of the photon-map leaf around the position among the
// leaves with candidates; n_pleaf, the key past the last leaf, when there is nothing to gather (outside the map, a leaf without candidates)
GI_HD uint32_t gather_key(const Scene& S, V3 pos)
{
    const int32_t leaf = gather_leaf_of(S, pos);
    const int32_t rank = leaf < 0 ? -1 : S.pleaf_rank[leaf];
    return rank < 0 ? (uint32_t)S.n_pleaf : (uint32_t)rank;
}
// Visit every candidate photon of a leaf's range list.  Positions are fetched four at a time before any of them is used, so the
// four loads are in flight together instead of one L2 round trip per photon (the loop is latency-bound otherwise).
template <class F>
GI_HD void for_each_candidate(const Scene& S, const PRange* ranges, int n_ranges, F&& f)
{
    for (int r = 0; r < n_ranges; r++) {
        const PRange rg = ranges[r];
        const double* base = S.ph_pos + (size_t)rg.first * 3;
        for (int32_t j = 0; j < rg.count; j += 4) {
            const int32_t last = rg.count - 1;
            const int32_t j1 = j + 1 < last ? j + 1 : last, j2 = j + 2 < last ? j + 2 : last, j3 = j + 3 < last ? j + 3 : last;
            const double* p0 = base + (size_t)j * 3;
            const double* p1 = base + (size_t)j1 * 3;
            const double* p2 = base + (size_t)j2 * 3;
            const double* p3 = base + (size_t)j3 * 3;
            const V3 a = v3(p0[0], p0[1], p0[2]), b = v3(p1[0], p1[1], p1[2]), cc = v3(p2[0], p2[1], p2[2]), d = v3(p3[0], p3[1], p3[2]);
            f(rg.first + j, a);
            if (j + 1 <= last) f(rg.first + j + 1, b);
            if (j + 2 <= last) f(rg.first + j + 2, cc);
            if (j + 3 <= last) f(rg.first + j + 3, d);
        }
    }
}

// ---- the selection.  Every form fills one GatherAcc through the steps below, so all of them run the very same arithmetic.
struct GatherAcc {
    V3 pos, dir;
    Heap h;          // the per-lane form's pass 1 only
    float tau;       // the K-th smallest float key, K = min(GI_GATHER_K, ncand)
    int ncand;
    V3 s_lt, s_eq;   // contributions of the candidates with key < tau / key == tau, each summed in candidate order
    int c_lt, c_eq;
    double r_eq;     // largest exact squared distance of the tie group
};
GI_HD void g_begin(GatherAcc& a, V3 pos, V3 dir, float* heap_mem, int heap_stride, int ncand)
{
    a.pos = pos; a.dir = dir;
    a.h.hp = heap_mem; a.h.stride = heap_stride; a.h.n = 0;
    a.tau = 0; a.ncand = ncand;
    a.s_lt = v3(0, 0, 0); a.s_eq = v3(0, 0, 0);
    a.c_lt = 0; a.c_eq = 0; a.r_eq = 0;
}
// exact squared distance of a photon at pp; its key is (float)g_d2
GI_HD double g_d2(const GatherAcc& a, V3 pp) { return len2(pp - a.pos); }
// what a photon adds: colour * dot(photon direction, gather direction); dc = its direction and colour, six doubles
GI_HD V3 g_contrib(const GatherAcc& a, const double* dc) { return v3(dc[3], dc[4], dc[5]) * dot(v3(dc[0], dc[1], dc[2]), a.dir); }
GI_HD void g_key(GatherAcc& a, V3 pp)   // pass 1 with the heap
{
    float key = (float)g_d2(a, pp);
    if (a.h.n < GI_GATHER_K) { heap_push(a.h, key); a.tau = a.h.hp[0]; }
    else if (key < a.tau) { heap_replace_root(a.h, key); a.tau = a.h.hp[0]; }
}
// pass 2, the two halves: a candidate below tau, a candidate of the tie group at tau (d2 = its exact distance)
GI_HD void g_add_lt(GatherAcc& a, V3 contrib) { a.s_lt = a.s_lt + contrib; a.c_lt++; }
GI_HD void g_add_eq(GatherAcc& a, V3 contrib, double d2) { a.s_eq = a.s_eq + contrib; a.c_eq++; a.r_eq = d2 > a.r_eq ? d2 : a.r_eq; }
GI_HD void g_acc(GatherAcc& a, V3 pp, const double* dc)
{
    double d2 = g_d2(a, pp);
    float key = (float)d2;
    if (key <= a.tau) {
        V3 contrib = g_contrib(a, dc);
        if (key < a.tau) g_add_lt(a, contrib);
        else g_add_eq(a, contrib, d2);
    }
}
// Pass 1 of the wave-cooperative gather (k_st_gather): tau = the K-th smallest float key, K = min(GI_GATHER_K, ncand), without the heap.
// A lane keeps its 32 smallest keys sorted in 32 registers and folds the candidates in 32 at a time: sort the 32 new keys, take
// min(best[i], new[31 - i]) -- the 32 smallest of the 64, as a bitonic sequence -- and merge.  tau is a property of the SET of keys, so
// any order of groups gives the same number.  The groups are taken from the last candidate back to the first, which puts the one short
// group (ncand % 32 keys) first: it is sorted on its own by an 8- or 16-key network, its keys become best[0..], the rest stays INFINITY.
GI_HD void kce(float& a, float& b) { const float lo = fminf(a, b), hi = fmaxf(a, b); a = lo; b = hi; }
// Batcher's odd-even merge sort of N = 8, 16, 32 keys: 19, 63, 191 compare-exchanges (the bitonic sorter takes 24, 80, 240)
template <int N>
GI_HD void ksort(float (&v)[N])
{
#pragma unroll
    for (int p = 1; p < N; p <<= 1)
#pragma unroll
        for (int k = p; k >= 1; k >>= 1)
#pragma unroll
            for (int j = k % p; j <= N - 1 - k; j += 2 * k)
#pragma unroll
                for (int i = 0; i <= (k - 1 < N - 1 - j - k ? k - 1 : N - 1 - j - k); i++)
                    if ((i + j) / (2 * p) == (i + j + k) / (2 * p)) kce(v[i + j], v[i + j + k]);
}
GI_HD void kmerge32(float (&v)[32])   // bitonic sequence -> ascending
{
#pragma unroll
    for (int j = 16; j > 0; j >>= 1)
#pragma unroll
        for (int i = 0; i < 32; i++) {
            const int l = i ^ j;
            if (l > i) kce(v[i], v[l]);
        }
}
// the first group: keys [k0, k0 + t) of the current chunk, t <= N, padded with INFINITY to N and sorted into best[0, N)
template <int N, class Key>
GI_HD void ksel_first(float (&best)[32], Key key, int k0, int t)
{
    float nk[N];
#pragma unroll
    for (int k = 0; k < N; k++) {
        const int kk = k < t ? k0 + k : k0 + t - 1;   // wave-uniform clamp: no read past the chunk
        const float v = key(kk);
        nk[k] = k < t ? v : INFINITY;
    }
    ksort<N>(nk);
#pragma unroll
    for (int k = 0; k < N; k++) best[k] = nk[k];
}
// tau of pass 1.  stage(c0, m) brings candidates [c0, c0 + m) of the leaf in (m <= 64), key(k) is the float key of the k-th of them.
// Chunks of 64 go from the last to the first, so chunk 0 is the one staged last; within a chunk the groups of 32 go from the last to the first.
template <class Stage, class Key>
GI_HD float ksel_tau(int ncand, Stage stage, Key key)
{
    float best[32];
#pragma unroll
    for (int k = 0; k < 32; k++) best[k] = INFINITY;
    bool first = true;
    for (int c0 = (ncand - 1) & ~63; c0 >= 0; c0 -= 64) {
        const int m = ncand - c0 < 64 ? ncand - c0 : 64;
        stage(c0, m);
        for (int k0 = (m - 1) & ~31; k0 >= 0; k0 -= 32) {
            if (first) {
                const int t = m - k0;   // 1 .. 32: ncand % 32 keys, or 32
                if (t <= 8) ksel_first<8>(best, key, k0, t);
                else if (t <= 16) ksel_first<16>(best, key, k0, t);
                else ksel_first<32>(best, key, k0, t);
                first = false;
                continue;
            }
            float nk[32];
#pragma unroll
            for (int k = 0; k < 32; k++) nk[k] = key(k0 + k);
            ksort<32>(nk);
#pragma unroll
            for (int k = 0; k < 32; k++) best[k] = fminf(best[k], nk[31 - k]);
            // after the last group only the largest of the 32 smallest is wanted, which does not need them in order
            if (c0 != 0 || k0 != 0) kmerge32(best);
        }
    }
    // (what the heap's root holds after pass 1 of gather_in_leaf)
    float tau = 0.0f;
    if (ncand < 32) {
#pragma unroll
        for (int k = 0; k < 32; k++) tau = best[k] < INFINITY ? fmaxf(tau, best[k]) : tau;
    } else {
#pragma unroll
        for (int k = 0; k < 32; k++) tau = fmaxf(tau, best[k]);   // keys are squared distances: >= 0
    }
    return tau;
}
// the estimate: the sum of the K nearest over the disc through the farthest of them (r2 = its squared distance)
GI_HD V3 g_density(V3 sum, double r2) { return sum / (GI_PI * r2); }
// K, the number of photons an estimate is made of; and how many of them the tie group still has to give once everything below tau is in
// (>= 1: the K-th smallest key itself belongs to a candidate with key == tau)
GI_HD int g_k(const GatherAcc& a) { return a.ncand < GI_GATHER_K ? a.ncand : GI_GATHER_K; }
GI_HD int g_need(const GatherAcc& a) { return g_k(a) - a.c_lt; }
// false: float keys tie across rank 32 -- the caller has to resolve the tie group with exact distances (g_exact)
GI_HD bool g_end(const GatherAcc& a, V3& res)
{
    if (a.c_eq > g_need(a)) return false;
    res = g_density(a.s_lt + a.s_eq, a.r_eq);
    return true;
}
// Pass 3 (rare), for every form: the g_need nearest of the tie group by exact distance, one extraction per scan of the leaf's range list, added
// to the sum below tau.  Reads a.pos, a.dir, a.tau, a.ncand, a.s_lt and a.c_lt -- which every form computes to the same bits -- and nothing else.
// The group is taken in the order (d2, candidate number), so each extraction takes exactly one photon: bit-equal distances (copies of a photon,
// symmetric layouts) are resolved in candidate order, and every copy counts
GI_HD V3 g_exact(const Scene& S, const PRange* ranges, int n_ranges, const GatherAcc& a)
{
    const int need = g_need(a);
    V3 res = a.s_lt;
    double last = -1.0;
    int32_t last_seq = -1;
    for (int j = 0; j < need; j++) {
        double best = INFINITY;
        int32_t best_seq = -1, seq = 0;
        V3 bc = v3(0, 0, 0);
        for (int r = 0; r < n_ranges; r++) {
            const PRange rg = ranges[r];
            const double* pp = S.ph_pos + (size_t)rg.first * 3;
            for (int32_t k = 0; k < rg.count; k++, pp += 3, seq++) {
                double d2 = g_d2(a, v3(pp[0], pp[1], pp[2]));
                if ((float)d2 == a.tau && (d2 > last || (d2 == last && seq > last_seq)) && d2 < best) {
                    best = d2; best_seq = seq;
                    bc = g_contrib(a, S.ph_dircol + (size_t)(rg.first + k) * 6);
                }
            }
        }
        if (best == INFINITY) break;   // (not reached: pass 3 runs only when the group holds at least need + 1 photons)
        res = res + bc;
        last = best; last_seq = best_seq;
    }
    return g_density(res, last);
}
GI_HD V3 g_exact(const Scene& S, int32_t leaf, const GatherAcc& a)
{
    const PNode& lf = S.pnodes[leaf];
    return g_exact(S, S.pranges + lf.nb_off, lf.u.lf.nb_cnt, a);
}
// ---- the per-lane form
GI_HD V3 gather_in_leaf(const Scene& S, int32_t node, V3 pos, V3 dir, float* heap_mem, int heap_stride, int* n_cand_out, Counters* c)
{
    V3 res = v3(0, 0, 0);
    if (n_cand_out) *n_cand_out = 0;
    if (node < 0) return res;
    // PhotonMap::Node::get (include/photonMap.cpp:71-92) for this leaf's (+-EPSILON) box was run once per leaf when the map was
    // laid out (gi_layout.h): its result is the list of photon ranges [nb_off, nb_off + nb_cnt)
    const PNode& lf = S.pnodes[node];
    const PRange* ranges = S.pranges + lf.nb_off;
    const int n_ranges = lf.u.lf.nb_cnt;
    const int ncand = lf.u.lf.nb_photons;
    if (n_cand_out) *n_cand_out = ncand;
    if (c) c->pcand += (unsigned long long)ncand;
    if (ncand == 0) return res;
    GatherAcc a;
    g_begin(a, pos, dir, heap_mem, heap_stride, ncand);
    for_each_candidate(S, ranges, n_ranges, [&](int32_t, V3 pp) { g_key(a, pp); });                                       // pass 1
    for_each_candidate(S, ranges, n_ranges, [&](int32_t idx, V3 pp) { g_acc(a, pp, S.ph_dircol + (size_t)idx * 6); });    // pass 2
    if (!g_end(a, res)) res = g_exact(S, ranges, n_ranges, a);                                                            // pass 3
    return res;
}
GI_HD V3 gather(const Scene& S, V3 pos, V3 dir, float* heap_mem, int heap_stride, int* n_cand_out, Counters* c)
{
    if (c) c->gathers++;
    return gather_in_leaf(S, gather_find_leaf(S, pos), pos, dir, heap_mem, heap_stride, n_cand_out, c);
}
// the caustic term of a vertex into its path's radiance: L += (T * colour) * caustic.  The one place a gather's result is written
GI_HD void gather_add(double* Lp, const double* gcoef, V3 caustic)
{
    const V3 L = ld3(Lp) + ld3(gcoef) * caustic;
    Lp[0] = L.x; Lp[1] = L.y; Lp[2] = L.z;
}
