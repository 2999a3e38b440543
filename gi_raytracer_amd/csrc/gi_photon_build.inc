// gi_photon_build.inc -- the photon octree built on the device (included by gi_kernels.hip behind gi_sort.inc: needs gi_ctx, gi_context.inc).
//
// Replaces PhotonMap::push_back x n + PhotonMap::rebuild / PhotonMap::Node::partition (include/photonMap.cpp:24-47,137-192) and the
// flattening that gi_upload_photons does on the host, for photons that are already on the device (RayTracer::tracePhotons -> k_emit) or
// that a caller hands in.  The tables it leaves are the ones gi_upload_photons would have produced from gih_build_photon_map, byte for
// byte (tests: test_device_photon_map_build_*): PNode records in breadth-first order with consecutive children, photons leaf by leaf in
// the reference's depth-first order (insertion order inside a leaf), and per leaf the merged photon ranges of PhotonMap::Node::get(leaf
// box +- EPSILON).
//
// Division of labour.  Everything that is per photon runs on the device, level by level: which child of its node contains a photon
// (the eight boxes with the reference's corner expressions, half-open contains()), a stable radix sort of the photon order by
// (segment, child) -- a photon only ever moves inside the range of its node, so the array is in depth-first leaf order at every level --
// and the per-child counts; at the end the gather of the photon records into leaf order and, per leaf, the walk that collects its
// candidate ranges.  What is per NODE (a few bytes of bookkeeping per split: counts -> new segments, new node boxes, who splits next;
// 73 k nodes for the benchmark's 200 k photons) is done by the host between the levels from the downloaded counts.
namespace {

struct PBSeg {                  // a run of the photon order that belongs to one node (or to the photons a split dropped: node < 0)
    double lo[3], hi[3];        // box of the node (used while it is being split)
    uint32_t start, cnt;
    int32_t node;               // breadth-first record index, -1 = dropped photons
    uint32_t active;            // splits at this level
};

// the eight octants with the reference's corner expressions (include/photonMap.cpp:139-149; the host builder's octants()): x is bit 0,
// z bit 1, y bit 2; low side [min, mid), high side [min + .5 d, mid + .5 d), child 7 [mid, max)
__host__ __device__ inline void pb_child_box(const double* lo, const double* hi, int c, double* clo, double* chi)
{
    const int bit[3] = {c & 1, (c >> 2) & 1, (c >> 1) & 1};   // x, y, z
    for (int ax = 0; ax < 3; ax++) {
        const double mid = lo[ax] + (hi[ax] - lo[ax]) * .5, h = .5 * (hi[ax] - lo[ax]);
        if (c == 0) { clo[ax] = lo[ax]; chi[ax] = mid; }
        else if (c == 7) { clo[ax] = mid; chi[ax] = hi[ax]; }
        else { clo[ax] = bit[ax] ? lo[ax] + h : lo[ax]; chi[ax] = bit[ax] ? mid + h : mid; }
    }
}

__global__ __launch_bounds__(256) void k_pb_init(uint32_t* order, uint32_t n)
{
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) order[i] = i;
}

// key of position k = segment * 16 + child (0..7; 8 = in no child) for photons of a splitting node, segment * 16 otherwise: a stable sort
// by it moves a photon only inside its node's range, behind the photons of lower children and in front of the dropped ones
__global__ __launch_bounds__(256) void k_pb_keys(const double* ph, const uint32_t* order, const PBSeg* segs, const uint32_t* seg_start, uint32_t n_seg, uint32_t n, uint32_t* keys)
{
    for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < n; k += gridDim.x * blockDim.x) {
        uint32_t lo = 0, hi = n_seg;                          // last segment with start <= k (empty segments precede the one they share a start with)
        while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (seg_start[mid] <= k) lo = mid; else hi = mid; }
        const PBSeg& sg = segs[lo];
        uint32_t c = 0;
        if (sg.active) {
            const double* p = ph + (size_t)order[k] * 9;
            c = 8;
            for (int i = 0; i < 8; i++) {                     // the reference tests every child; a photon can be in at most one
                double clo[3], chi[3];
                pb_child_box(sg.lo, sg.hi, i, clo, chi);
                if (p[0] >= clo[0] && p[1] >= clo[1] && p[2] >= clo[2] && p[0] < chi[0] && p[1] < chi[1] && p[2] < chi[2]) { c = (uint32_t)i; break; }
            }
        }
        keys[k] = lo * 16u + c;
    }
}

// counts[a][c] = photons of active segment a (index act[a]) that went to child c (c = 8: dropped), from the sorted keys
__global__ __launch_bounds__(256) void k_pb_counts(const uint32_t* keys, const PBSeg* segs, const uint32_t* act, uint32_t n_act, uint32_t* counts)
{
    for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < n_act * 9u; t += gridDim.x * blockDim.x) {
        const uint32_t a = t / 9u, c = t % 9u, s = act[a];
        const uint32_t beg = segs[s].start, end = beg + segs[s].cnt, key = s * 16u + c;
        uint32_t lo = beg, hi = end;                          // first position with keys >= key
        while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (keys[mid] < key) lo = mid + 1; else hi = mid; }
        uint32_t lo2 = lo, hi2 = end;                         // first position with keys > key
        while (lo2 < hi2) { const uint32_t mid = (lo2 + hi2) >> 1; if (keys[mid] <= key) lo2 = mid + 1; else hi2 = mid; }
        counts[t] = lo2 - lo;
    }
}

// photons into leaf order: final position f takes the photon at position src[f] of the sorted order
__global__ __launch_bounds__(256) void k_pb_gather(const double* ph, const uint32_t* order, const uint32_t* src, uint32_t n_final, double* pos, double* dircol)
{
    for (uint32_t f = blockIdx.x * blockDim.x + threadIdx.x; f < n_final; f += gridDim.x * blockDim.x) {
        const double* p = ph + (size_t)order[src[f]] * 9;
        for (int k = 0; k < 3; k++) pos[(size_t)f * 3 + k] = p[k];
        for (int k = 0; k < 6; k++) dircol[(size_t)f * 6 + k] = p[3 + k];
    }
}

// PhotonMap::Node::get(leaf box +- EPSILON) for every leaf (include/photonMap.cpp:71-92): the leaves whose closed box touches it, in
// depth-first child order, as merged photon ranges.  write = 0: count ranges and photons; write = 1: fill pranges at the leaf's nb_off.
// leaf_first / leaf_cnt: photon range of every record (leaves), indexed by record.
__global__ __launch_bounds__(256) void k_pb_neighbours(PNode* nodes, const int32_t* leaf_rec, uint32_t n_leaf, const int32_t* leaf_first, const int32_t* leaf_cnt, PRange* ranges, int write)
{
    for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < n_leaf; t += gridDim.x * blockDim.x) {
        PNode& lf = nodes[leaf_rec[t]];
        double qlo[3], qhi[3];
        for (int k = 0; k < 3; k++) { qlo[k] = lf.bmin[k] - GI_EPSILON; qhi[k] = lf.bmax[k] + GI_EPSILON; }
        int n_rng = 0, total = 0;
        int32_t last_first = 0, last_cnt = 0;
        PRange* out = write ? ranges + lf.nb_off : nullptr;
        if (!(qhi[0] - qlo[0] <= 0)) {                        // include/photonMap.cpp:73-74
            // explicit stack of (record of child 0, next child to look at); the root itself is not tested (getInRange calls _root.get directly)
            int32_t st_first[64];
            int8_t st_next[64];
            int sp = 0;
            if (nodes[0].first_child < 0) {                   // the root is a leaf: it is what get() returns
                if (leaf_cnt[0] > 0) { last_first = leaf_first[0]; last_cnt = leaf_cnt[0]; n_rng = 1; total = last_cnt; }
            } else { st_first[0] = nodes[0].first_child; st_next[0] = 0; sp = 1; }
            while (sp > 0) {
                if (st_next[sp - 1] >= 8) { sp--; continue; }
                const int32_t rec = st_first[sp - 1] + st_next[sp - 1];
                st_next[sp - 1]++;
                const PNode& nd = nodes[rec];
                if (!((nd.bmin[0] <= qhi[0] && nd.bmax[0] >= qlo[0]) && (nd.bmin[1] <= qhi[1] && nd.bmax[1] >= qlo[1]) && (nd.bmin[2] <= qhi[2] && nd.bmax[2] >= qlo[2]))) continue;   // include/bbox.h:33-38
                if (nd.first_child >= 0) { if (sp < 64) { st_first[sp] = nd.first_child; st_next[sp] = 0; sp++; } continue; }
                const int32_t first = leaf_first[rec], count = leaf_cnt[rec];
                if (count <= 0) continue;
                if (n_rng > 0 && last_first + last_cnt == first) last_cnt += count;
                else {
                    if (n_rng > 0 && write) { out[n_rng - 1].first = last_first; out[n_rng - 1].count = last_cnt; }
                    last_first = first; last_cnt = count; n_rng++;
                }
                total += count;
            }
            if (n_rng > 0 && write) { out[n_rng - 1].first = last_first; out[n_rng - 1].count = last_cnt; }
        }
        if (!write) { lf.u.lf.nb_cnt = n_rng; lf.u.lf.nb_photons = total; }
    }
}

// prefix of the stored flags of k_emit in (photon index, light) order, and the compaction of the stored photons
__global__ __launch_bounds__(256) void k_pb_compact_emitted(const PhotonOut* out, const int32_t* stored, const int32_t* excl, uint32_t total, double* ph)
{
    for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < total; j += gridDim.x * blockDim.x)
        if (stored[j]) for (int k = 0; k < 9; k++) ph[(size_t)excl[j] * 9 + k] = out[j].v[k];
}

struct PBHostNode { double lo[3], hi[3]; int32_t first_child; int32_t seg; };   // seg: index into the final segment list (leaves)

int build_photon_map_on_device(gi_ctx* c, const double* d_ph, int32_t n, const double* box6)
{
    hipStream_t st = c->stream;
    clear_photon_map(c);
    if (n <= 0) return GI_OK;
    const int grid = c->n_cu * 4;
    DevBuf<uint32_t> d_order[2], d_keys[2], d_seg_start, d_act, d_counts;
    DevBuf<PBSeg> d_segs;
    HIP_TRY(c, d_order[0].alloc((size_t)n)); HIP_TRY(c, d_order[1].alloc((size_t)n)); HIP_TRY(c, d_keys[0].alloc((size_t)n)); HIP_TRY(c, d_keys[1].alloc((size_t)n));
    DevBuf<uint32_t> d_tmp, d_hist;          // gi_sort.inc: one more copy of keys and values to ping-pong through, the digit counters of a pass
    HIP_TRY(c, d_tmp.alloc((size_t)n * 2)); HIP_TRY(c, d_hist.alloc((size_t)GI_RS_MAXBINS * GI_MAX_PRODUCER_BLOCKS));
    hipLaunchKernelGGL(k_pb_init, dim3(grid), dim3(256), 0, st, d_order[0].p, (uint32_t)n);

    std::vector<PBSeg> segs(1);
    std::vector<PBHostNode> nodes(1);
    for (int k = 0; k < 3; k++) { segs[0].lo[k] = box6[k]; segs[0].hi[k] = box6[3 + k]; nodes[0].lo[k] = box6[k]; nodes[0].hi[k] = box6[3 + k]; }
    segs[0].start = 0; segs[0].cnt = (uint32_t)n; segs[0].node = 0; segs[0].active = n > 16 ? 1u : 0u;   // PhotonMap::rebuild: the root splits when it holds more than MAX_PHOTONS_PER_LEAF
    nodes[0].first_child = -1; nodes[0].seg = 0;
    int cur = 0;
    for (int level = 0; level < 4096; level++) {
        std::vector<uint32_t> act, starts(segs.size());
        for (size_t s = 0; s < segs.size(); s++) { starts[s] = segs[s].start; if (segs[s].active) act.push_back((uint32_t)s); }
        if (act.empty()) break;
        if (segs.size() * 16ull > 0xffffffffull) return fail(c, GI_E_INVALID, "photon map: too many segments for 32-bit sort keys");
        HIP_TRY(c, d_segs.upload(segs)); HIP_TRY(c, d_seg_start.upload(starts)); HIP_TRY(c, d_act.upload(act));
        HIP_TRY(c, d_counts.alloc(act.size() * 9));
        hipLaunchKernelGGL(k_pb_keys, dim3(grid), dim3(256), 0, st, d_ph, d_order[cur].p, d_segs.p, d_seg_start.p, (uint32_t)segs.size(), (uint32_t)n, d_keys[0].p);
        int bits = 1;
        while ((1ull << bits) < segs.size() * 16ull) bits++;
        {   // stable: photons keep their order inside a (node, octant) group, as PhotonMap::Node::partition's push_backs do
            const int rc = rs_sort_pairs(c, d_keys[0].p, d_keys[1].p, d_order[cur].p, d_order[cur ^ 1].p, d_tmp.p, d_tmp.p + n, (uint32_t)n, nullptr, 0, bits, d_hist.p);
            if (rc) return rc;
        }
        cur ^= 1;
        hipLaunchKernelGGL(k_pb_counts, dim3(grid), dim3(256), 0, st, d_keys[1].p, d_segs.p, d_act.p, (uint32_t)act.size(), d_counts.p);
        std::vector<uint32_t> counts(act.size() * 9);
        HIP_TRY(c, hipMemcpyAsync(counts.data(), d_counts.p, counts.size() * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipStreamSynchronize(st));
        // per-node bookkeeping of this level (PhotonMap::Node::partition, include/photonMap.cpp:137-192): eight children per split node,
        // consecutive records in breadth-first order; a child splits next when it holds more than 16 photons and the split was not
        // "skipped" (mean child count above MAX_SUBDIV_RATIO of the parent's)
        std::vector<PBSeg> next;
        next.reserve(segs.size() + act.size() * 9);
        size_t a = 0;
        for (size_t s = 0; s < segs.size(); s++) {
            if (!segs[s].active) { if (segs[s].node >= 0) nodes[(size_t)segs[s].node].seg = (int32_t)next.size(); next.push_back(segs[s]); continue; }
            const uint32_t* cn = &counts[a * 9];
            a++;
            double mean = 0;
            for (int i = 0; i < 8; i++) mean += (double)cn[i];
            mean /= 8;
            const bool frozen = mean > 0.75 * (double)segs[s].cnt;
            const int32_t first_child = (int32_t)nodes.size();
            nodes[(size_t)segs[s].node].first_child = first_child;
            uint32_t at = segs[s].start;
            for (int i = 0; i < 9; i++) {
                PBSeg ch;
                memset(&ch, 0, sizeof ch);
                ch.start = at; ch.cnt = cn[i]; at += cn[i];
                if (i < 8) {
                    pb_child_box(segs[s].lo, segs[s].hi, i, ch.lo, ch.hi);
                    ch.node = first_child + i;
                    ch.active = (!frozen && cn[i] > 16u) ? 1u : 0u;
                    PBHostNode hn;
                    for (int k = 0; k < 3; k++) { hn.lo[k] = ch.lo[k]; hn.hi[k] = ch.hi[k]; }
                    hn.first_child = -1; hn.seg = (int32_t)next.size();
                    nodes.push_back(hn);
                } else { ch.node = -1; ch.active = 0; if (ch.cnt == 0) continue; }   // photons no child contains: they leave the map here
                next.push_back(ch);
            }
        }
        segs.swap(next);
    }
    // ---- final layout: leaves in depth-first order = segment order; dropped segments are skipped
    const int N = (int)nodes.size();
    std::vector<PNode> recs((size_t)N);
    std::vector<int32_t> leaf_first((size_t)N, 0), leaf_cnt((size_t)N, 0), leaf_rec;
    std::vector<uint32_t> src;
    src.reserve((size_t)n);
    for (size_t s = 0; s < segs.size(); s++) {
        if (segs[s].node < 0) continue;
        leaf_first[(size_t)segs[s].node] = (int32_t)src.size();
        leaf_cnt[(size_t)segs[s].node] = (int32_t)segs[s].cnt;
        leaf_rec.push_back(segs[s].node);
        for (uint32_t k = 0; k < segs[s].cnt; k++) src.push_back(segs[s].start + k);
    }
    const int n_final = (int)src.size();
    bool planes_ok = true;
    for (int r = 0; r < N; r++) {
        PNode& t = recs[(size_t)r];
        memset(&t, 0, sizeof t);
        for (int k = 0; k < 3; k++) { t.bmin[k] = nodes[(size_t)r].lo[k]; t.bmax[k] = nodes[(size_t)r].hi[k]; }
        t.first_child = nodes[(size_t)r].first_child;
        if (t.first_child >= 0) {     // the planes the eight children's boxes are made of (gi_layout.h: layout_photons)
            const PBHostNode* ch = &nodes[(size_t)t.first_child];
            for (int k = 0; k < 3; k++) t.mid[k] = ch[7].lo[k];
            for (int ax = 0; ax < 3; ax++) {
                const int bitpos = ax == 0 ? 0 : (ax == 1 ? 2 : 1);
                t.u.in.lo2[ax] = ch[1 << bitpos].lo[ax]; t.u.in.hi2[ax] = ch[1 << bitpos].hi[ax];
            }
            for (int cc = 0; cc < 8; cc++)
                for (int ax = 0; ax < 3; ax++) {
                    const int bitpos = ax == 0 ? 0 : (ax == 1 ? 2 : 1);
                    const double wlo = cc == 7 ? t.mid[ax] : (((cc >> bitpos) & 1) ? t.u.in.lo2[ax] : t.bmin[ax]);
                    const double whi = cc == 7 ? t.bmax[ax] : (((cc >> bitpos) & 1) ? t.u.in.hi2[ax] : t.mid[ax]);
                    if (ch[cc].lo[ax] != wlo || ch[cc].hi[ax] != whi) planes_ok = false;
                }
        }
    }
    if (n_final <= 0) return GI_OK;   // every photon fell outside the box: an empty map, as gi_upload_photons leaves it
    DevBuf<uint32_t> d_src;
    DevBuf<int32_t> d_leaf_rec, d_leaf_first, d_leaf_cnt;
    HIP_TRY(c, d_src.upload(src)); HIP_TRY(c, d_leaf_rec.upload(leaf_rec)); HIP_TRY(c, d_leaf_first.upload(leaf_first)); HIP_TRY(c, d_leaf_cnt.upload(leaf_cnt));
    HIP_TRY(c, c->photons.d_ph_pos.alloc((size_t)n_final * 3)); HIP_TRY(c, c->photons.d_ph_dircol.alloc((size_t)n_final * 6));
    hipLaunchKernelGGL(k_pb_gather, dim3(grid), dim3(256), 0, st, d_ph, d_order[cur].p, d_src.p, (uint32_t)n_final, c->photons.d_ph_pos.p, c->photons.d_ph_dircol.p);
    HIP_TRY(c, c->photons.d_pnodes.upload(recs));
    // candidate ranges: count per leaf, offsets in depth-first leaf order (the order layout_photons assigns them in), fill
    hipLaunchKernelGGL(k_pb_neighbours, dim3(grid), dim3(256), 0, st, c->photons.d_pnodes.p, d_leaf_rec.p, (uint32_t)leaf_rec.size(), d_leaf_first.p, d_leaf_cnt.p, (PRange*)nullptr, 0);
    HIP_TRY(c, hipMemcpyAsync(recs.data(), c->photons.d_pnodes.p, recs.size() * sizeof(PNode), hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    // layout_photons visits the leaves in the builder's pre-order; the segment order is the same depth-first order
    int32_t n_rng = 0;
    for (int32_t r : leaf_rec) { recs[(size_t)r].nb_off = n_rng; n_rng += recs[(size_t)r].u.lf.nb_cnt; }
    HIP_TRY(c, hipMemcpyAsync(c->photons.d_pnodes.p, recs.data(), recs.size() * sizeof(PNode), hipMemcpyHostToDevice, st));
    HIP_TRY(c, c->photons.d_pranges.alloc((size_t)std::max(n_rng, 1)));
    HIP_TRY(c, hipMemsetAsync(c->photons.d_pranges.p, 0, (size_t)std::max(n_rng, 1) * sizeof(PRange), st));
    hipLaunchKernelGGL(k_pb_neighbours, dim3(grid), dim3(256), 0, st, c->photons.d_pnodes.p, d_leaf_rec.p, (uint32_t)leaf_rec.size(), d_leaf_first.p, d_leaf_cnt.p, c->photons.d_pranges.p, 1);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(st));
    return install_photon_map(c, N, n_final, std::max(n_rng, 1), planes_ok);
}

}  // namespace
