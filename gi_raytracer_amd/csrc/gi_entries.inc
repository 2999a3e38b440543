// gi_entries.inc -- the function-level and debug entries of the C ABI: host arrays in, one kernel (or one pass), host arrays out.  Included by
// gi_kernels.hip behind the passes.  Each reads: argument and state checks, buffers (Entry, gi_context.inc:
// element counts once per buffer), the launch, and Entry::run copies the outputs back in the order they were named.
// The kernels come first (nothing outside this file launches them), outside the anonymous namespace; the entries follow them.

__global__ __launch_bounds__(GI_BLOCK) void k_trace(Scene S, int n, const double* rays, int32_t* hit, int32_t* ent, double* res)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double* r = rays + (size_t)i * 6;
    Ray ray = make_ray_exact(v3(r[0], r[1], r[2]), v3(r[3], r[4], r[5]));
    Rng rng = rng_make(0, (uint32_t)i);
    HitRec h;
    bool ok = trace(S, ray, rng, P_TRACE_ALPHA, h, nullptr);
    hit[i] = ok ? 1 : 0;
    ent[i] = ok ? h.tri : -1;
    double* o = res + (size_t)i * 8;
    if (ok) {
        V3 nn = shading_normal(S, h);
        o[0] = h.pos.x; o[1] = h.pos.y; o[2] = h.pos.z; o[3] = nn.x; o[4] = nn.y; o[5] = nn.z; o[6] = h.u; o[7] = h.v;
    } else
        for (int k = 0; k < 8; k++) o[k] = 0;
}

__global__ __launch_bounds__(GI_BLOCK) void k_visible(Scene S, int n, const double* q, int32_t* vis)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double* p = q + (size_t)i * 6;
    V3 o = v3(p[0], p[1], p[2]), t = v3(p[3], p[4], p[5]);
    V3 ld = t - o;
    double maxt = len2(ld);
    Ray sr = make_ray(o, ld);
    Rng rng = rng_make(0, (uint32_t)i);
    vis[i] = visible(S, sr, maxt, rng, 0, nullptr) ? 1 : 0;
}

__global__ __launch_bounds__(GI_BLOCK) void k_visible_rays(Scene S, int n, const double* rays, const double* mt, int32_t* vis)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double* r = rays + (size_t)i * 6;
    Ray sr = make_ray_exact(v3(r[0], r[1], r[2]), v3(r[3], r[4], r[5]));
    Rng rng = rng_make(0, (uint32_t)i);
    vis[i] = visible(S, sr, mt[i], rng, 0, nullptr) ? 1 : 0;
}

// gi_debug_walk: caller rays through the walk forms the passes run, with k_trace's / k_visible_rays' keys (rng_make(0, i), P_TRACE_ALPHA, light 0) and
// k_trace's output.  FORM 0: a ray per lane over the records and content boxes k_st_trace (closest hit) / a shadow kernel without lights to end at
// (any hit) stages; FORM 1, 2: a ray per wave / per group of 16 lanes over what k_st_finish stages (ray i = group i, every lane of the group holds
// it, the first writes).  lds = 0: the same source with nothing staged (n_l = n_lc = 0), every record and box from global memory.
#define GI_DEBUG_WALK_BLOCK 256
template <int FEAT, int FORM, bool ANY>
__global__ __launch_bounds__(GI_DEBUG_WALK_BLOCK) void k_debug_walk(Scene S, int n, const double* rays, const double* mt, int lds, int32_t* hit, int32_t* ent, double* res)
{
    constexpr uint32_t G = FORM == 1 ? 64u : (FORM == 2 ? 16u : 1u);
    typedef typename std::conditional<FORM == 0, LdsWide, LdsWideCoop<FORM == 2 ? 16 : 64>>::type Src;
    const LdsWide L = FORM == 0 ? stage_wide_in_lds(S, true, GI_LDS_WNODES_BIG, ANY ? 0 : 1) : stage_wide_in_lds(S, true, GI_FINISH_COOP_RECORDS);   // ends with a barrier
    Src N;
    N.g = L.g; N.cboxes = L.cboxes; N.cuse = L.cuse; N.box_off = L.box_off; N.use_off = L.use_off;
    N.n_l = lds ? L.n_l : 0; N.n_lc = lds ? L.n_lc : 0;
    const uint32_t n_groups = gridDim.x * blockDim.x / G;
    for (uint32_t i = (blockIdx.x * blockDim.x + threadIdx.x) / G; i < (uint32_t)n; i += n_groups) {   // uniform over a group: its lanes stay together
        const double* r = rays + (size_t)i * 6;
        const Ray ray = make_ray_exact(v3(r[0], r[1], r[2]), v3(r[3], r[4], r[5]));
        const Rng rng = rng_make(0, i);
        const bool writes = (threadIdx.x & (G - 1u)) == 0u;
        if constexpr (ANY) {
            const bool vis = visible_nodes<FEAT>(S, N, ray, mt[i], rng, 0, nullptr);
            if (writes) hit[i] = vis ? 1 : 0;
        } else {
            HitRec h;
            h.tu = 0; h.tv = 0;
            const bool ok = trace_nodes<FEAT>(S, N, ray, rng, P_TRACE_ALPHA, h, nullptr);
            if (!writes) continue;
            hit[i] = ok ? 1 : 0;
            ent[i] = ok ? h.tri : -1;
            double* o = res + (size_t)i * 8;
            if (ok) {
                const V3 nn = shading_normal(S, h);
                o[0] = h.pos.x; o[1] = h.pos.y; o[2] = h.pos.z; o[3] = nn.x; o[4] = nn.y; o[5] = nn.z; o[6] = h.u; o[7] = h.v;
            } else
                for (int k = 0; k < 8; k++) o[k] = 0;
        }
    }
}

__global__ __launch_bounds__(GI_BLOCK) void k_radiance(Scene S, int n, const double* rays, const uint32_t* stream, uint64_t seed, double* out3)
{
    __shared__ float heap[GI_GATHER_K * GI_BLOCK];
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double* r = rays + (size_t)i * 6;
    Ray ray = make_ray_exact(v3(r[0], r[1], r[2]), v3(r[3], r[4], r[5]));
    V3 L = radiance_path(S, ray, stream[i], seed, heap + threadIdx.x, GI_BLOCK, nullptr);
    out3[(size_t)i * 3] = L.x; out3[(size_t)i * 3 + 1] = L.y; out3[(size_t)i * 3 + 2] = L.z;
}

__global__ __launch_bounds__(GI_BLOCK) void k_emit(Scene S, int count, int max_depth, uint64_t seed, PhotonOut* out, int32_t* stored, int32_t* tries)
{
    int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= count * S.n_light) return;
    int i = j / S.n_light, li = j % S.n_light;
    PhotonOut po;
    int32_t t = 0;
    bool ok = emit_photon(S, i, li, count, max_depth, seed, po, t);
    stored[j] = ok ? 1 : 0;
    tries[j] = t;
    if (ok) out[j] = po;
}

__global__ __launch_bounds__(GI_BLOCK) void k_leaf_order(Scene S, int n, const double* rays, int cap, int32_t* leaf_out, int32_t* n_out)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double* r = rays + (size_t)i * 6;
    n_out[i] = leaf_order(S, make_ray_exact(v3(r[0], r[1], r[2]), v3(r[3], r[4], r[5])), cap, leaf_out + (size_t)i * cap);
}
__global__ __launch_bounds__(GI_BLOCK) void k_kat(int what, int n, const double* in, int in_stride, double* out)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double a[9], o[3];
    for (int k = 0; k < 9; k++) a[k] = k < in_stride ? in[(size_t)i * in_stride + k] : 0.0;
    kat_eval(what, a, o);
    for (int k = 0; k < 3; k++) out[(size_t)i * 3 + k] = o[k];
}

__global__ void k_halton(Scene S, int n, const uint32_t* dim, const uint32_t* index, float* out)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = halton_sample(S, dim[i], index[i]);
}
__global__ void k_halton_index(HaltonEnumD he, int n, const uint32_t* sxy, uint32_t* out)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = halton_index(he, sxy[i * 3], sxy[i * 3 + 1], sxy[i * 3 + 2]);
}

namespace {

// The photon map's box: the caller's, or the scene's
void frame_box(const gi_ctx* c, const double* box6, double* out)
{
    for (int k = 0; k < 3; k++) { out[k] = box6 ? box6[k] : c->S.root_bmin[k]; out[3 + k] = box6 ? box6[3 + k] : c->S.root_bmax[k]; }
}

}  // namespace

extern "C" {

#define GI_GRID(n) dim3((unsigned)(((n) + GI_BLOCK - 1) / GI_BLOCK)), dim3(GI_BLOCK)

int gi_trace(gi_ctx* c, int32_t n, const double* rays, int32_t* hit, int32_t* ent, double* res)
{
    if (!c || n < 0 || (n && (!rays || !hit || !ent || !res))) return GI_E_INVALID;
    if (!c->scene.have_scene) return fail(c, GI_E_STATE, "trace: no scene uploaded");
    if (n == 0) return GI_OK;
    const size_t N = (size_t)n;
    Entry e(c, "trace");
    const double* d_r = e.in(rays, N * 6);
    int32_t* d_h = e.out(hit, N);
    int32_t* d_e = e.out(ent, N);
    double* d_o = e.out(res, N * 8);
    return e.run([&] { hipLaunchKernelGGL(k_trace, GI_GRID(n), 0, c->stream, c->S, n, d_r, d_h, d_e, d_o); });
}

int gi_visible(gi_ctx* c, int32_t n, const double* q, int32_t* vis)
{
    if (!c || n < 0 || (n && (!q || !vis))) return GI_E_INVALID;
    if (!c->scene.have_scene) return fail(c, GI_E_STATE, "visible: no scene uploaded");
    if (n == 0) return GI_OK;
    const size_t N = (size_t)n;
    Entry e(c, "visible");
    const double* d_q = e.in(q, N * 6);
    int32_t* d_v = e.out(vis, N);
    return e.run([&] { hipLaunchKernelGGL(k_visible, GI_GRID(n), 0, c->stream, c->S, n, d_q, d_v); });
}

int gi_visible_rays(gi_ctx* c, int32_t n, const double* rays, const double* mt, int32_t* vis)
{
    if (!c || n < 0 || (n && (!rays || !mt || !vis))) return GI_E_INVALID;
    if (!c->scene.have_scene) return fail(c, GI_E_STATE, "visible: no scene uploaded");
    if (n == 0) return GI_OK;
    const size_t N = (size_t)n;
    Entry e(c, "visible_rays");
    const double* d_r = e.in(rays, N * 6);
    const double* d_m = e.in(mt, N);
    int32_t* d_v = e.out(vis, N);
    return e.run([&] { hipLaunchKernelGGL(k_visible_rays, GI_GRID(n), 0, c->stream, c->S, n, d_r, d_m, d_v); });
}

int gi_gather(gi_ctx* c, int32_t n, const double* q, double* res3, int32_t* n_cand)
{
    if (!c || n < 0 || (n && (!q || !res3))) return GI_E_INVALID;
    if (!c->scene.have_scene) return fail(c, GI_E_STATE, "gather: no scene uploaded");
    if (n == 0) return GI_OK;
    const size_t N = (size_t)n;
    Entry e(c, "gather");
    const double* d_q = e.in(q, N * 6);
    double* d_r = e.out(res3, N * 3);
    int32_t* d_n = e.out(n_cand, N);          // optional
    return e.run([&] { hipLaunchKernelGGL(k_gather, GI_GRID(n), 0, c->stream, c->S, n, d_q, d_r, d_n); });
}

int gi_radiance(gi_ctx* c, int32_t n, const double* rays, const uint32_t* stream, uint64_t seed, double* out3)
{
    if (!c || n < 0 || (n && (!rays || !stream || !out3))) return GI_E_INVALID;
    if (!c->scene.have_scene) return fail(c, GI_E_STATE, "radiance: no scene uploaded");
    if (n == 0) return GI_OK;
    const size_t N = (size_t)n;
    Entry e(c, "radiance");
    const double* d_r = e.in(rays, N * 6);
    const uint32_t* d_s = e.in(stream, N);
    double* d_o = e.out(out3, N * 3);
    return e.run([&] { hipLaunchKernelGGL(k_radiance, GI_GRID(n), 0, c->stream, c->S, n, d_r, d_s, seed, d_o); });
}

int gi_emit_photons(gi_ctx* c, int32_t count, int32_t max_depth, uint64_t seed, double* photons_out, int32_t cap, int64_t* tries_out)
{
    if (!c || count < 0 || cap < 0 || (cap && !photons_out)) return GI_E_INVALID;
    if (!c->scene.have_scene) return fail(c, GI_E_STATE, "emit_photons: no scene uploaded");
    const long long total = (long long)count * c->S.n_light;
    if (tries_out) *tries_out = 0;
    if (total == 0) return 0;
    if (total > 0x7fffffffLL) return fail(c, GI_E_INVALID, "emit_photons: count too large");
    const size_t N = (size_t)total;
    std::vector<PhotonOut> hp(N);
    std::vector<int32_t> hs(N), ht(N);
    Entry e(c, "emit_photons");
    PhotonOut* d_p = e.out(hp.data(), N);
    int32_t* d_s = e.out(hs.data(), N);
    int32_t* d_t = e.out(ht.data(), N);
    const int rc = e.run([&] { hipLaunchKernelGGL(k_emit, GI_GRID(total), 0, c->stream, c->S, count, max_depth, seed, d_p, d_s, d_t); });
    if (rc) return rc;
    // compaction in (photon index, light) order = the order one reference thread appends them (include/raytracer.h:593-706)
    int stored = 0;
    int64_t tries = 0;
    for (size_t j = 0; j < N; j++) {
        tries += ht[j];
        if (!hs[j]) continue;
        if (stored < cap) memcpy(photons_out + (size_t)stored * 9, hp[j].v, 72);
        stored++;
    }
    if (tries_out) *tries_out = tries;
    if (stored > cap) return fail(c, GI_E_INVALID, "emit_photons: output capacity too small");
    return stored;
}

int gi_build_photon_map(gi_ctx* c, int32_t n, const double* photons, const double* box6)
{
    if (!c || n < 0 || (n && !photons)) return GI_E_INVALID;
    c->prog.open = false;
    if (!c->scene.have_scene) return fail(c, GI_E_STATE, "build_photon_map: no scene uploaded");
    HIP_TRY(c, hipSetDevice(c->device));
    double box[6];
    frame_box(c, box6, box);
    DevBuf<double> d_ph;
    if (n) HIP_TRY(c, d_ph.upload(photons, (size_t)n * 9));
    return build_photon_map_on_device(c, d_ph.p, n, box);
}

int gi_trace_photons(gi_ctx* c, int32_t count, int32_t max_depth, uint64_t seed, const double* box6, int64_t* tries_out)
{
    if (!c || count < 0) return GI_E_INVALID;
    c->prog.open = false;
    if (!c->scene.have_scene) return fail(c, GI_E_STATE, "trace_photons: no scene uploaded");
    const long long total = (long long)count * c->S.n_light;
    if (tries_out) *tries_out = 0;
    if (total > 0x7fffffffLL) return fail(c, GI_E_INVALID, "trace_photons: count too large");
    HIP_TRY(c, hipSetDevice(c->device));
    double box[6];
    frame_box(c, box6, box);
    if (total == 0) { const int rc = build_photon_map_on_device(c, nullptr, 0, box); return rc < 0 ? rc : 0; }
    const size_t N = (size_t)total;
    DevBuf<PhotonOut> d_p;
    DevBuf<int32_t> d_s, d_t, d_x;
    HIP_TRY(c, d_p.alloc(N)); HIP_TRY(c, d_s.alloc(N)); HIP_TRY(c, d_t.alloc(N)); HIP_TRY(c, d_x.alloc(N));
    hipLaunchKernelGGL(k_emit, GI_GRID(total), 0, c->stream, c->S, count, max_depth, seed, d_p.p, d_s.p, d_t.p);
    // stored photons in (photon index, light) order = the order one reference thread appends them (include/raytracer.h:593-706)
    HIP_TRY(c, hipMemcpyAsync(d_x.p, d_s.p, N * sizeof(int32_t), hipMemcpyDeviceToDevice, c->stream));
    hipLaunchKernelGGL(k_rs_scan, dim3(1), dim3(1024), 0, c->stream, reinterpret_cast<uint32_t*>(d_x.p), (uint32_t)total);   // exclusive prefix sums, in place (gi_sort.inc)
    int32_t last_x = 0, last_s = 0;
    HIP_TRY(c, hipMemcpyAsync(&last_x, d_x.p + (total - 1), 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(&last_s, d_s.p + (total - 1), 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    const int32_t n = last_x + last_s;
    if (tries_out) {      // total emission tries (diagnostic): summed on the host from the per-index counts
        std::vector<int32_t> ht(N);
        HIP_TRY(c, d_t.download(ht.data(), N));
        int64_t tries = 0;
        for (int32_t v : ht) tries += v;
        *tries_out = tries;
    }
    DevBuf<double> d_ph;
    HIP_TRY(c, d_ph.alloc((size_t)std::max(n, 1) * 9));
    hipLaunchKernelGGL(k_pb_compact_emitted, GI_GRID(total), 0, c->stream, d_p.p, d_s.p, d_x.p, (uint32_t)total, d_ph.p);
    HIP_TRY(c, hipGetLastError());
    const int rc = build_photon_map_on_device(c, d_ph.p, n, box);
    return rc < 0 ? rc : n;
}

int gi_debug_photon_tables(gi_ctx* c, int32_t* n_node, int32_t* n_range, int32_t* n_photon, void* nodes128, int32_t* ranges2, double* pos3, double* dircol6)
{
    if (!c) return GI_E_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    const Scene& S = c->S;
    if (n_node) *n_node = S.n_pnode;
    if (n_range) *n_range = S.n_pnode > 0 ? c->photons.n_prange : 0;
    if (n_photon) *n_photon = S.n_photon;
    if (S.n_pnode <= 0) return GI_OK;
    if (nodes128) HIP_TRY(c, hipMemcpy(nodes128, S.pnodes, (size_t)S.n_pnode * sizeof(PNode), hipMemcpyDeviceToHost));
    if (ranges2) HIP_TRY(c, hipMemcpy(ranges2, S.pranges, (size_t)c->photons.n_prange * sizeof(PRange), hipMemcpyDeviceToHost));
    if (pos3 && S.n_photon) HIP_TRY(c, hipMemcpy(pos3, S.ph_pos, (size_t)S.n_photon * 24, hipMemcpyDeviceToHost));
    if (dircol6 && S.n_photon) HIP_TRY(c, hipMemcpy(dircol6, S.ph_dircol, (size_t)S.n_photon * 48, hipMemcpyDeviceToHost));
    return GI_OK;
}

int gi_debug_sort_pairs(gi_ctx* c, int32_t n, const uint32_t* keys, const uint32_t* vals, int32_t begin_bit, int32_t end_bit, uint32_t* keys_out, uint32_t* vals_out)
{
    if (!c || n < 0 || begin_bit < 0 || end_bit > 32 || end_bit <= begin_bit || (n && (!keys || !vals || !keys_out || !vals_out))) return GI_E_INVALID;
    if (n == 0) return GI_OK;
    const size_t N = (size_t)n;
    Entry e(c, "sort_pairs");
    const uint32_t* d_k = e.in(keys, N);
    const uint32_t* d_v = e.in(vals, N);
    uint32_t* d_ko = e.out(keys_out, N);
    uint32_t* d_vo = e.out(vals_out, N);
    uint32_t* d_tk = e.scratch<uint32_t>(N);
    uint32_t* d_tv = e.scratch<uint32_t>(N);
    uint32_t* d_hist = e.scratch<uint32_t>((size_t)GI_RS_MAXBINS * GI_MAX_PRODUCER_BLOCKS);
    return e.run([&] { return rs_sort_pairs(c, d_k, d_ko, d_v, d_vo, d_tk, d_tv, (uint32_t)n, nullptr, begin_bit, end_bit, d_hist); });
}

int gi_debug_find_leaves(gi_ctx* c, int32_t n, const double* pos, int32_t* fast_out, int32_t* full_out)
{
    if (!c || n < 0 || (n && (!pos || !fast_out || !full_out))) return GI_E_INVALID;
    if (c->S.n_pnode <= 0) return fail(c, GI_E_STATE, "find_leaves: no photon map");
    if (n == 0) return GI_OK;
    const size_t N = (size_t)n;
    Entry e(c, "find_leaves");
    const double* d_p = e.in(pos, N * 3);
    int32_t* d_a = e.out(fast_out, N);
    int32_t* d_b = e.out(full_out, N);
    return e.run([&] { hipLaunchKernelGGL(k_find_leaves, GI_GRID(n), 0, c->stream, c->S, n, d_p, d_a, d_b); });
}

int gi_debug_gather_pass(gi_ctx* c, int32_t n, const double* q6, int32_t kernel, int32_t sort, double* res3, uint32_t* keys_out, uint32_t* order_out, int64_t* counters2)
{
    if (!c || n < 0 || kernel < 0 || kernel > 3 || (n && (!q6 || !res3))) return GI_E_INVALID;
    if (c->S.n_pnode <= 0) return fail(c, GI_E_STATE, "gather_pass: no photon map");
    const bool wave = (kernel & 2) != 0, counting = (kernel & 1) != 0;
    if (wave && !c->S.pcand) return fail(c, GI_E_STATE, "gather_pass: k_st_gather_wave needs the written-out candidate lists (off: GI_FLAT_CANDIDATES=0)");
    if (counters2) counters2[0] = counters2[1] = 0;
    if (n == 0) return GI_OK;
    const uint32_t N = (uint32_t)n;
    const size_t pool_bytes = (size_t)N * GI_POOL_BYTES_PER_SLOT;
    StreamCounters h;
    memset(&h, 0, sizeof h);
    Entry e(c, "gather_pass");
    const double* d_q = e.in(q6, (size_t)N * 6);
    double* d_L = e.out(res3, (size_t)N * 3);
    uint32_t *d_k[2], *d_v[2];
    d_k[0] = e.scratch<uint32_t>(N); d_v[0] = e.scratch<uint32_t>(N);
    d_k[1] = e.out(keys_out, N);              // optional
    d_v[1] = e.out(order_out, N);             // optional
    StreamCounters* d_sc = e.out(counting ? &h : nullptr, 1);
    unsigned char* d_pool = e.scratch<unsigned char>(pool_bytes);
    unsigned long long* d_ss = e.scratch<unsigned long long>(N);
    uint32_t* d_tk = e.scratch<uint32_t>(N);
    uint32_t* d_tv = e.scratch<uint32_t>(N);
    uint32_t* d_hist = e.scratch<uint32_t>((size_t)GI_RS_MAXBINS * GI_MAX_PRODUCER_BLOCKS);
    const int rc = e.run([&]() -> int {
        HIP_TRY(c, hipMemsetAsync(d_pool, 0, pool_bytes, c->stream));
        HIP_TRY(c, hipMemsetAsync(d_L, 0, (size_t)N * 3 * sizeof(double), c->stream));
        HIP_TRY(c, hipMemsetAsync(d_sc, 0, sizeof(StreamCounters), c->stream));
        const PathPool pool = make_path_pool(d_pool, N);
        hipLaunchKernelGGL(k_gather_pass_prep, GI_GRID(n), 0, c->stream, c->S, pool, n, d_q, d_ss, d_k[0], d_v[0]);
        HIP_TRY(c, hipGetLastError());
        if (sort) {
            const int rc = rs_sort_pairs(c, d_k[0], d_k[1], d_v[0], d_v[1], d_tk, d_tv, N, nullptr, 0, photon_key_bits(c->S), d_hist);
            if (rc) return rc;
        } else {
            HIP_TRY(c, hipMemcpyAsync(d_k[1], d_k[0], (size_t)N * sizeof(uint32_t), hipMemcpyDeviceToDevice, c->stream));
            HIP_TRY(c, hipMemcpyAsync(d_v[1], d_v[0], (size_t)N * sizeof(uint32_t), hipMemcpyDeviceToDevice, c->stream));
        }
        launch_gather(c, wave, counting, pool, d_k[1], d_v[1], N, d_ss, 0ull, d_L, counting ? d_sc : nullptr);
        return GI_OK;
    });
    if (rc == GI_OK && counters2 && counting) { counters2[0] = (int64_t)h.gather_queries; counters2[1] = (int64_t)h.gather_cand; }
    return rc;
}

int gi_debug_walk(gi_ctx* c, int32_t n, const double* rays, const double* mt, int32_t form, int32_t lds, int32_t* hit_or_vis, int32_t* ent, double* res8)
{
    if (!c || n < 0 || form < 0 || form > 2 || lds < 0 || lds > 1 || (n && (!rays || !hit_or_vis || (!mt && (!ent || !res8))))) return GI_E_INVALID;
    if (!c->scene.have_scene) return fail(c, GI_E_STATE, "debug_walk: no scene uploaded");
    if (!c->S.wnodes) return fail(c, GI_E_STATE, "debug_walk: the scene has no wide records (or gi_set_wide_nodes(0))");
    if (n == 0) return GI_OK;
    // k_debug_walk<FEAT, FORM, ANY>: the level stage_trace picks (textures -> 7, else 3) x the three forms x closest hit, any hit
    typedef decltype(&k_debug_walk<3, 0, false>) WalkK;
    static const WalkK kWalk[2][3][2] = {
        {{k_debug_walk<3, 0, false>, k_debug_walk<3, 0, true>}, {k_debug_walk<3, 1, false>, k_debug_walk<3, 1, true>}, {k_debug_walk<3, 2, false>, k_debug_walk<3, 2, true>}},
        {{k_debug_walk<7, 0, false>, k_debug_walk<7, 0, true>}, {k_debug_walk<7, 1, false>, k_debug_walk<7, 1, true>}, {k_debug_walk<7, 2, false>, k_debug_walk<7, 2, true>}}};
    const WalkK fn = kWalk[c->S.n_tex > 0 ? 1 : 0][form][mt ? 1 : 0];
    const size_t lds_bytes = form == 0 ? (size_t)GI_LDS_WIDE_BOXES_BYTES : (size_t)GI_LDS_BOXES_BYTES(GI_FINISH_COOP_RECORDS);
    const size_t N = (size_t)n, lanes = N * (form == 0 ? 1 : (form == 1 ? 64 : 16));
    const unsigned blocks = (unsigned)std::min<size_t>((lanes + GI_DEBUG_WALK_BLOCK - 1) / GI_DEBUG_WALK_BLOCK, 2048);   // the kernel strides over the rest
    Entry e(c, "debug_walk");
    const double* d_r = e.in(rays, N * 6);
    const double* d_m = mt ? e.in(mt, N) : nullptr;
    int32_t* d_h = e.out(hit_or_vis, N);
    int32_t* d_e = mt ? nullptr : e.out(ent, N);
    double* d_o = mt ? nullptr : e.out(res8, N * 8);
    return e.run([&]() -> int {
        HIP_TRY(c, hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));   // more than 64 KB has to be asked for
        hipLaunchKernelGGL(fn, dim3(blocks), dim3(GI_DEBUG_WALK_BLOCK), lds_bytes, c->stream, c->S, n, d_r, d_m, lds, d_h, d_e, d_o);
        return GI_OK;
    });
}

int gi_debug_leaf_order(gi_ctx* c, int32_t n, const double* rays, int32_t cap, int32_t* leaf_out, int32_t* n_out)
{
    if (!c || n < 0 || cap < 1 || (n && (!rays || !leaf_out || !n_out))) return GI_E_INVALID;
    if (!c->scene.have_scene) return fail(c, GI_E_STATE, "leaf_order: no scene uploaded");
    if (n == 0) return GI_OK;
    const size_t N = (size_t)n;
    Entry e(c, "leaf_order");
    const double* d_r = e.in(rays, N * 6);
    int32_t* d_l = e.out(leaf_out, N * cap);
    int32_t* d_n = e.out(n_out, N);
    return e.run([&]() -> int {
        HIP_TRY(c, hipMemsetAsync(d_l, 0xff, N * cap * sizeof(int32_t), c->stream));
        hipLaunchKernelGGL(k_leaf_order, GI_GRID(n), 0, c->stream, c->S, n, d_r, cap, d_l, d_n);
        return GI_OK;
    });
}

int gi_kat(gi_ctx* c, int32_t what, int32_t n, const double* in, int32_t in_stride, double* out3)
{
    if (!c || n < 0 || in_stride < 1 || in_stride > 9 || (n && (!in || !out3))) return GI_E_INVALID;
    if (n == 0) return GI_OK;
    const size_t N = (size_t)n;
    Entry e(c, "kat");
    const double* d_i = e.in(in, N * in_stride);
    double* d_o = e.out(out3, N * 3);
    return e.run([&] { hipLaunchKernelGGL(k_kat, GI_GRID(n), 0, c->stream, what, n, d_i, in_stride, d_o); });
}

int gi_halton_sample(gi_ctx* c, int32_t n, const uint32_t* dim, const uint32_t* index, float* out)
{
    if (!c || n < 0 || (n && (!dim || !index || !out))) return GI_E_INVALID;
    if (n == 0) return GI_OK;
    for (int i = 0; i < n; i++) if (dim[i] > 255) return fail(c, GI_E_INVALID, "halton_sample: dimension > 255");
    const size_t N = (size_t)n;
    Entry e(c, "halton_sample");
    const uint32_t* d_d = e.in(dim, N);
    const uint32_t* d_i = e.in(index, N);
    float* d_o = e.out(out, N);
    return e.run([&] { hipLaunchKernelGGL(k_halton, GI_GRID(n), 0, c->stream, c->S, n, d_d, d_i, d_o); });
}

int gi_halton_index(gi_ctx* c, int32_t width, int32_t height, int32_t n, const uint32_t* sxy, uint32_t* out)
{
    if (!c || width <= 0 || height <= 0 || n < 0 || (n && (!sxy || !out))) return GI_E_INVALID;
    if (n == 0) return GI_OK;
    const size_t N = (size_t)n;
    Entry e(c, "halton_index");
    const uint32_t* d_i = e.in(sxy, N * 3);
    uint32_t* d_o = e.out(out, N);
    return e.run([&] { hipLaunchKernelGGL(k_halton_index, GI_GRID(n), 0, c->stream, make_halton_enum((unsigned)width, (unsigned)height), n, d_i, d_o); });
}

}  // extern "C"
