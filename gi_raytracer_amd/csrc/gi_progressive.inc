// gi_progressive.inc -- progressive render sessions (gi_progressive_*).  Included by gi_kernels.hip behind gi_api.inc: a step
// runs the bodies of the frame entries (stream_samples, run_rounds, gi_stream.inc).
//
// ---- progressive sessions (an addition: the reference renders a frame in one piece).  The session owns its pixel records (c->prog.pix); a step runs
// the bodies of the one-shot frame on them -- stream_samples over [E, E') for a fixed sample count, run_rounds with the cap E' otherwise -- so a
// frame built in steps has the bits of the frame built in one call.
namespace {
struct ProgBlobHeader {            // little-endian, 192 bytes; the pixel records follow as they lie on the device (include/gi_hip.h)
    char magic[8];
    uint32_t version, header_bytes;
    gi_render_params rp;           // 136 bytes: its fields in declaration order, 4 bytes of padding before noise_thresh
    int32_t schedule, sample_end;
    uint64_t n_records;
    uint32_t record_bytes, reserved0;
    int32_t n_entity, n_node, n_photon;
    uint32_t lens_tag;             // 0: pinhole (gi_layout.h: lens_tag)
};
static_assert(sizeof(gi_render_params) == 136 && sizeof(ProgBlobHeader) == 192 && sizeof(PixRec) == 72, "checkpoint layout (include/gi_hip.h)");
const char kProgMagic[8] = {'G', 'I', 'P', 'R', 'O', 'G', 'R', '\0'};
const uint32_t kProgVersion = 1;

uint32_t prog_records(const Frame& F, int schedule) { return schedule == 0 ? (uint32_t)F.w * (uint32_t)F.local_rows : rounds_records(F); }
// a session on parameters already validated: the records allocated (not yet filled), E = sample_end
int prog_open(gi_ctx* c, const gi_render_params& rp, const Frame& F, int schedule, int32_t sample_end)
{
    gi_ctx::Progressive& g = c->prog;
    g.open = false;
    const uint32_t n_rec = prog_records(F, schedule);
    if (g.pix.n != n_rec || !g.pix.p) HIP_TRY(c, g.pix.alloc(n_rec));
    g.rp = rp; g.F = F; g.schedule = schedule; g.sample_end = sample_end; g.n_rec = n_rec;
    return GI_OK;
}
}  // namespace

extern "C" {

int gi_progressive_begin(gi_ctx* c, const gi_render_params* p)
{
    if (!c) return GI_E_INVALID;
    c->prog.open = false;
    if (!c->scene.have_scene) return fail(c, GI_E_STATE, "progressive_begin: no scene uploaded");
    Frame F;
    std::string ferr;
    if (!make_frame(p, F, ferr)) return fail(c, GI_E_INVALID, ferr);
    if (c->render_mode == 1 || c->count_enabled) return fail(c, GI_E_STATE, "progressive_begin: sessions run on the streaming passes (render mode 0 or 2), not on the megakernel");
    HIP_TRY(c, hipSetDevice(c->device));
    const int schedule = uses_refill_schedule(c, F) ? 0 : 1;
    int rc = prog_open(c, *p, F, schedule, 0);
    if (rc) return rc;
    if (c->prog.n_rec) {
        hipLaunchKernelGGL(k_pix_init, dim3(stream_grids(c).pix), dim3(GI_BLOCK), 0, c->stream, c->prog.pix.p, c->prog.n_rec);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    c->prog.open = true;
    return GI_OK;
}

int gi_progressive_end(gi_ctx* c)
{
    if (!c) return GI_E_INVALID;
    if (c->prog.open || c->prog.pix.p) (void)hipSetDevice(c->device);
    c->prog.open = false;
    c->prog.pix.release();
    return GI_OK;
}

int gi_progressive_step_device(gi_ctx* c, int32_t n_samples, void* d_out, int out_is_f64, int32_t* d_spp, volatile const int* cancel)
{
    if (!c || !d_out || n_samples < 0) return c ? fail(c, GI_E_INVALID, "progressive_step: n_samples < 0 or no output buffer") : GI_E_INVALID;
    gi_ctx::Progressive& g = c->prog;
    if (!g.open) return fail(c, GI_E_STATE, "progressive_step: no session open (gi_progressive_begin; scene and photon uploads end a session)");
    if (cancel && *cancel) return fail(c, GI_E_CANCELLED, "render: cancelled");
    HIP_TRY(c, hipSetDevice(c->device));
    c->t_frame.reset(); c->last_launches = 0;
    // a rank without rows has no pixel and no output: only E moves (no kernel, no timing beyond the reset above), and d_out is never touched --
    // which is why gi_progressive_step_host may hand its host pointer through for such a rank
    if (g.F.local_rows == 0) { g.sample_end = (int32_t)std::min<long long>((long long)g.sample_end + n_samples, g.F.max_samples); return GI_OK; }
    const int32_t e0 = g.sample_end, e1 = (int32_t)std::min<long long>((long long)e0 + n_samples, g.F.max_samples);
    if (e1 == e0) {                 // nothing to take: the frame as the records hold it
        hipStream_t st = c->stream;
        c->clock.restart();
        HIP_TRY(c, c->t_frame.begin(st));
        c->clock.begin(STG_ACCUM, st);
        hipLaunchKernelGGL(k_pix_resolve, dim3(std::min<uint32_t>((g.n_rec + GI_BLOCK - 1) / GI_BLOCK, (uint32_t)stream_grids(c).pix)), dim3(GI_BLOCK), 0, st, g.F, g.pix.p, g.n_rec, g.schedule, d_out, out_is_f64, d_spp);
        c->clock.end(st);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, c->t_frame.end(st));
        c->last_launches = 1;
        return GI_OK;
    }
    if (g.schedule == 0) {
        int done = e0;
        const int rc = stream_samples(c, g.F, g.pix.p, e0, e1, false, d_out, out_is_f64, d_spp, cancel, &done);
        g.sample_end = done;        // a cancelled step keeps the chunks it folded
        return rc;
    }
    if (c->count_stream) return fail(c, GI_E_STATE, "render: the streaming work counters (gi_set_counters 2) belong to fixed-sample-count frames of the wavefront pipeline");
    Frame F = g.F;
    F.max_samples = e1;             // the cap of this step; a pixel the rule has stopped stays stopped
    const int rc = run_rounds(c, F, g.pix.p, false, d_out, out_is_f64, d_spp, cancel);
    // cancelled at the top of a round or between the passes of one (whose radiances are dropped: the records change in k_ad_accum alone, and the n that
    // k_ad_gen left is set again by the next one): every record is at a sample boundary and below the cap; E stays, and the next step offers [.., E')
    // again to those below it
    if (rc == GI_OK) g.sample_end = e1;
    return rc;
}

int gi_progressive_step_host(gi_ctx* c, int32_t n_samples, void* h_out, int out_is_f64, int32_t* h_spp, volatile const int* cancel)
{
    if (!c || !h_out || n_samples < 0) return c ? fail(c, GI_E_INVALID, "progressive_step: n_samples < 0 or no output buffer") : GI_E_INVALID;
    if (!c->prog.open) return fail(c, GI_E_STATE, "progressive_step: no session open (gi_progressive_begin; scene and photon uploads end a session)");
    const size_t npix = (size_t)c->prog.F.local_rows * (size_t)c->prog.F.w;
    if (npix == 0) return gi_progressive_step_device(c, n_samples, h_out, out_is_f64, nullptr, cancel);
    return frame_to_host(c, "progressive_step_host", npix, h_out, out_is_f64, h_spp,
                         [&](void* d_out, int32_t* d_spp) { return gi_progressive_step_device(c, n_samples, d_out, out_is_f64, d_spp, cancel); });
}

int gi_progressive_status(gi_ctx* c, int32_t* sample_end, int64_t* pixels_wanting)
{
    if (!c) return GI_E_INVALID;
    gi_ctx::Progressive& g = c->prog;
    if (!g.open) return fail(c, GI_E_STATE, "progressive_status: no session open");
    if (sample_end) *sample_end = g.sample_end;
    if (pixels_wanting) {
        *pixels_wanting = 0;
        if (g.n_rec) {
            HIP_TRY(c, hipSetDevice(c->device));
            if (!c->st.d_wfcnt.p) HIP_TRY(c, c->st.d_wfcnt.alloc(2));
            HIP_TRY(c, hipMemsetAsync(c->st.d_wfcnt.p, 0, sizeof(unsigned int), c->stream));
            hipLaunchKernelGGL(k_pix_wanting, dim3(std::min<uint32_t>((g.n_rec + GI_BLOCK - 1) / GI_BLOCK, (uint32_t)stream_grids(c).pix)), dim3(GI_BLOCK), 0, c->stream, g.F, g.pix.p, g.n_rec, g.schedule, c->st.d_wfcnt.p);
            HIP_TRY(c, hipGetLastError());
            unsigned int n = 0;
            HIP_TRY(c, hipMemcpyAsync(&n, c->st.d_wfcnt.p, sizeof n, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(c, hipStreamSynchronize(c->stream));
            *pixels_wanting = (int64_t)n;
        }
    }
    return GI_OK;
}

int gi_progressive_state_bytes(gi_ctx* c, int64_t* n_bytes)
{
    if (!c || !n_bytes) return GI_E_INVALID;
    if (!c->prog.open) return fail(c, GI_E_STATE, "progressive_state_bytes: no session open");
    *n_bytes = (int64_t)sizeof(ProgBlobHeader) + (int64_t)c->prog.n_rec * (int64_t)sizeof(PixRec);
    return GI_OK;
}

int gi_progressive_save(gi_ctx* c, void* h_blob, int64_t cap_bytes)
{
    if (!c || !h_blob) return GI_E_INVALID;
    gi_ctx::Progressive& g = c->prog;
    if (!g.open) return fail(c, GI_E_STATE, "progressive_save: no session open");
    const int64_t need = (int64_t)sizeof(ProgBlobHeader) + (int64_t)g.n_rec * (int64_t)sizeof(PixRec);
    if (cap_bytes < need) return fail(c, GI_E_INVALID, "progressive_save: the buffer holds " + std::to_string(cap_bytes) + " bytes, the checkpoint needs " + std::to_string(need));
    ProgBlobHeader h;
    memset(&h, 0, sizeof h);
    memcpy(h.magic, kProgMagic, 8);
    h.version = kProgVersion; h.header_bytes = (uint32_t)sizeof h;
    memcpy(&h.rp, &g.rp, sizeof h.rp);
    memset(reinterpret_cast<char*>(&h.rp) + offsetof(gi_render_params, max_samples) + 4, 0, 4);   // the padding before noise_thresh
    h.schedule = g.schedule; h.sample_end = g.sample_end;
    h.n_records = g.n_rec; h.record_bytes = (uint32_t)sizeof(PixRec);
    h.n_entity = c->S.n_tri; h.n_node = c->S.n_node; h.n_photon = c->S.n_photon;
    h.lens_tag = lens_tag(c->lens.lens);
    memcpy(h_blob, &h, sizeof h);
    if (g.n_rec) {
        HIP_TRY(c, hipSetDevice(c->device));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        HIP_TRY(c, hipMemcpy(static_cast<char*>(h_blob) + sizeof h, g.pix.p, (size_t)g.n_rec * sizeof(PixRec), hipMemcpyDeviceToHost));
    }
    return GI_OK;
}

int gi_progressive_restore(gi_ctx* c, const void* h_blob, int64_t n_bytes)
{
    if (!c) return GI_E_INVALID;
    c->prog.open = false;
    if (!h_blob || n_bytes < (int64_t)sizeof(ProgBlobHeader)) return fail(c, GI_E_INVALID, "progressive_restore: the blob is shorter than a checkpoint header");
    ProgBlobHeader h;
    memcpy(&h, h_blob, sizeof h);
    if (memcmp(h.magic, kProgMagic, 8) != 0) return fail(c, GI_E_INVALID, "progressive_restore: not a checkpoint (magic)");
    if (h.version != kProgVersion) return fail(c, GI_E_INVALID, "progressive_restore: checkpoint format version " + std::to_string(h.version) + ", this library reads " + std::to_string(kProgVersion));
    if (h.header_bytes != sizeof h || h.record_bytes != sizeof(PixRec) || (h.schedule != 0 && h.schedule != 1))
        return fail(c, GI_E_INVALID, "progressive_restore: header or record size, or schedule, not of this format");
    Frame F;
    std::string ferr;
    if (!make_frame(&h.rp, F, ferr)) return fail(c, GI_E_INVALID, "progressive_restore: " + ferr);
    if (h.schedule == 0 && !(F.min_samples == F.max_samples && F.max_samples > 0)) return fail(c, GI_E_INVALID, "progressive_restore: the refill schedule needs a fixed sample count");
    if (h.schedule != 0 && !rounds_fit(F)) return fail(c, GI_E_INVALID, "progressive_restore: frame too large");
    if (h.sample_end < 0 || h.sample_end > F.max_samples) return fail(c, GI_E_INVALID, "progressive_restore: sample counter outside 0 .. max_samples");
    const uint32_t n_rec = prog_records(F, h.schedule);
    if (h.n_records != n_rec || n_bytes != (int64_t)sizeof h + (int64_t)n_rec * (int64_t)sizeof(PixRec))
        return fail(c, GI_E_INVALID, "progressive_restore: " + std::to_string(n_bytes) + " bytes, a checkpoint of this frame has " + std::to_string(sizeof h + (size_t)n_rec * sizeof(PixRec)) + " (truncated?)");
    if (h.lens_tag != lens_tag(c->lens.lens))
        return fail(c, GI_E_INVALID, "progressive_restore: the checkpoint was taken under another lens (tag " + std::to_string(h.lens_tag) + ", the context's lens has " + std::to_string(lens_tag(c->lens.lens)) + "): gi_set_lens first");
    if (!c->scene.have_scene) return fail(c, GI_E_STATE, "progressive_restore: no scene uploaded");
    if (c->count_enabled) return fail(c, GI_E_STATE, "progressive_restore: sessions run on the streaming passes, not with the megakernel's work counters (gi_set_counters 1)");
    if (h.n_entity != c->S.n_tri || h.n_node != c->S.n_node || h.n_photon != c->S.n_photon)
        return fail(c, GI_E_STATE, "progressive_restore: the checkpoint was taken on another scene or photon map (entities, nodes, photons " + std::to_string(h.n_entity) + ", " + std::to_string(h.n_node) + ", " +
                                       std::to_string(h.n_photon) + "; uploaded " + std::to_string(c->S.n_tri) + ", " + std::to_string(c->S.n_node) + ", " + std::to_string(c->S.n_photon) + ")");
    HIP_TRY(c, hipSetDevice(c->device));
    int rc = prog_open(c, h.rp, F, h.schedule, h.sample_end);
    if (rc) return rc;
    if (n_rec) {
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        HIP_TRY(c, hipMemcpy(c->prog.pix.p, static_cast<const char*>(h_blob) + sizeof h, (size_t)n_rec * sizeof(PixRec), hipMemcpyHostToDevice));
    }
    c->prog.open = true;
    return GI_OK;
}

}  // extern "C"
