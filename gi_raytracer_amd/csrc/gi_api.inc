// gi_api.inc -- the context's own entries of include/gi_hip.h: create and destroy, the uploads, the setters, the frame (gi_render_device,
// gi_render_host), its timers and counters.  Host code only; included by gi_kernels.hip behind gi_stream.inc, whose schedules the frame chooses between.
namespace {

// A frame of npix pixels that `render(d_out, d_spp)` leaves in scratch of this call, copied to the caller's arrays (gi_render_host, gi_progressive_step_host)
template <class Render>
int frame_to_host(gi_ctx* c, const char* what, size_t npix, void* h_out, int out_is_f64, int32_t* h_spp, Render render)
{
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t bytes = npix * 3 * (out_is_f64 ? 8 : 4);
    DevBuf<unsigned char> d_out;
    DevBuf<int32_t> d_spp;
    HIP_TRY(c, d_out.alloc(bytes));
    if (h_spp) HIP_TRY(c, d_spp.alloc(npix));
    const int rc = render((void*)d_out.p, d_spp.p);
    return rc != GI_OK ? rc : finish_to_host(c, what, {{h_out, d_out.p, bytes}, to_host(h_spp, d_spp, npix)});
}

}  // namespace

extern "C" {

int gi_create(gi_ctx** out, int device_ordinal)
{
    if (!out) return GI_E_INVALID;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return GI_E_NO_DEVICE;
    if (device_ordinal < 0 || device_ordinal >= n) return GI_E_INVALID;
    if (hipSetDevice(device_ordinal) != hipSuccess) return GI_E_NO_DEVICE;
    gi_ctx* c = new gi_ctx();
    c->device = device_ordinal;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device_ordinal) == hipSuccess) c->n_cu = prop.multiProcessorCount;
    std::vector<HaltonDim> dims;
    std::vector<uint16_t> table;
    build_halton_tables(dims, table);
    if (c->scene.d_hdims.upload(dims) != hipSuccess || c->scene.d_htable.upload(table) != hipSuccess || c->st.d_tile_counter.alloc(1) != hipSuccess ||
        c->st.d_counters.alloc(1) != hipSuccess) {
        delete c;
        return GI_E_HIP;
    }
    c->S.hdims = c->scene.d_hdims.p;
    c->S.htable = c->scene.d_htable.p;
    c->tune = Tuning::from_env(c->sw);
    *out = c;
    return GI_OK;
}

void gi_destroy(gi_ctx* c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    delete c;
}

const char* gi_last_error(const gi_ctx* c) { return c ? c->err.c_str() : "null context"; }

int gi_set_stream(gi_ctx* c, void* s)
{
    if (!c) return GI_E_INVALID;
    c->stream = (hipStream_t)s;
    return GI_OK;
}

int gi_upload_scene(gi_ctx* c, const gi_scene_desc* d)
{
    if (!c) return GI_E_INVALID;
    c->prog.open = false;   // a progressive session belongs to the scene and photon map it began on
    HostScene H;
    std::string err;
    if (!layout_scene(d, H, err)) return fail(c, GI_E_INVALID, err);
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, c->scene.upload(H, c->S));
    apply_switches(c);
    return GI_OK;
}

int gi_clear_photons(gi_ctx* c)
{
    if (!c) return GI_E_INVALID;
    c->prog.open = false;
    clear_photon_map(c);
    return GI_OK;
}

int gi_upload_photons(gi_ctx* c, const gi_photon_map_desc* d)
{
    if (!c || !d) return GI_E_INVALID;
    c->prog.open = false;
    if (!c->scene.have_scene) return fail(c, GI_E_STATE, "upload_photons: no scene");
    HostPhotons H;
    std::string err;
    if (!layout_photons(d, H, err)) return fail(c, GI_E_INVALID, err);
    HIP_TRY(c, hipSetDevice(c->device));
    if (H.n_node == 0) {
        clear_photon_map(c);
        return GI_OK;
    }
    HIP_TRY(c, c->photons.d_pnodes.upload(H.nodes));
    HIP_TRY(c, c->photons.d_pranges.upload(H.ranges));
    HIP_TRY(c, c->photons.d_ph_pos.upload(H.pos));
    HIP_TRY(c, c->photons.d_ph_dircol.upload(H.dircol));
    return install_photon_map(c, H.n_node, H.n_photon, (int32_t)H.ranges.size(), H.planes_ok);
}

int gi_local_rows(const gi_render_params* p) { return local_rows(p); }

int gi_render_device(gi_ctx* c, const gi_render_params* p, void* d_out, int out_is_f64, int32_t* d_spp, volatile const int* cancel)
{
    if (!c || !d_out) return GI_E_INVALID;
    if (!c->scene.have_scene) return fail(c, GI_E_STATE, "render: no scene uploaded");
    Frame F;
    std::string ferr;
    if (!make_frame(p, F, ferr)) return fail(c, GI_E_INVALID, ferr);
    if (cancel && *cancel) return fail(c, GI_E_CANCELLED, "render: cancelled");
    HIP_TRY(c, hipSetDevice(c->device));
    c->t_frame.reset(); c->last_launches = 0;
    if (F.local_rows == 0) return GI_OK;
    if (c->render_mode == 1 || c->count_enabled) return render_megakernel(c, F, d_out, out_is_f64, d_spp);
    if (c->count_stream && !uses_refill_schedule(c, F))
        return fail(c, GI_E_STATE, "render: the streaming work counters (gi_set_counters 2) belong to fixed-sample-count frames of the wavefront pipeline");
    if (uses_refill_schedule(c, F)) return render_streaming(c, F, d_out, out_is_f64, d_spp, cancel);
    return render_adaptive(c, F, d_out, out_is_f64, d_spp, cancel);
}

int gi_render_host(gi_ctx* c, const gi_render_params* p, void* h_out, int out_is_f64, int32_t* h_spp, volatile const int* cancel)
{
    if (!c || !h_out || !p) return GI_E_INVALID;
    const size_t npix = (size_t)gi_local_rows(p) * (size_t)std::max(p->width, 0);
    if (npix == 0) return GI_OK;
    return frame_to_host(c, "render_host", npix, h_out, out_is_f64, h_spp,
                         [&](void* d_out, int32_t* d_spp) { return gi_render_device(c, p, d_out, out_is_f64, d_spp, cancel); });
}

int gi_set_wide_nodes(gi_ctx* c, int enable)
{
    if (!c) return GI_E_INVALID;
    c->sw.wide = enable != 0;
    apply_switches(c);
    return (c->S.wnodes ? 1 : 0) | (c->S.pn_planes ? 2 : 0);
}

int gi_set_content_culling(gi_ctx* c, int enable)
{
    if (!c) return GI_E_INVALID;
    c->sw.cull = enable != 0;
    apply_switches(c);
    return c->S.cboxes ? 1 : 0;
}

int gi_set_entity_boxes(gi_ctx* c, int enable)
{
    if (!c) return GI_E_INVALID;
    c->sw.entity_boxes = enable != 0;
    apply_switches(c);
    return c->S.leaf_boxes ? 1 : 0;
}

int gi_set_render_mode(gi_ctx* c, int mode)
{
    if (!c || mode < 0 || mode > 2) return GI_E_INVALID;
    c->render_mode = mode;
    return GI_OK;
}

int gi_set_pool_slots(gi_ctx* c, int64_t slots)
{
    if (!c || slots < 64) return GI_E_INVALID;
    c->tune.pool_slots_max = (size_t)slots;
    return GI_OK;
}

int gi_last_render_ms(gi_ctx* c, float* ms, int32_t* n_launches)
{
    if (!c) return GI_E_INVALID;
    float frame_ms = 0;
    HIP_TRY(c, c->t_frame.read(&frame_ms));
    c->clock.read(getenv("GI_DEBUG_STAGES") != nullptr);   // read at every call
    if (ms) *ms = frame_ms;
    if (n_launches) *n_launches = c->last_launches;
    return GI_OK;
}

int gi_last_stage_ms(gi_ctx* c, float* out8)
{
    if (!c || !out8) return GI_E_INVALID;
    int rc = gi_last_render_ms(c, nullptr, nullptr);
    if (rc) return rc;
    for (int k = 0; k < 8; k++) out8[k] = c->clock.stage_ms[k];
    out8[STG_SHADE] += c->clock.stage_ms[STG_SHADOW];   // the shade stage of the 8-entry form includes the shadow walks it put off
    return GI_OK;
}

int gi_last_kernel_ms(gi_ctx* c, float* out10)
{
    if (!c || !out10) return GI_E_INVALID;
    int rc = gi_last_render_ms(c, nullptr, nullptr);
    if (rc) return rc;
    for (int k = 0; k < STG_COUNT_MAX; k++) out10[k] = c->clock.stage_ms[k];
    return GI_OK;
}

int gi_set_counters(gi_ctx* c, int enable)
{
    if (!c || enable < 0 || enable > 2) return GI_E_INVALID;
    c->count_enabled = enable == 1;
    c->count_stream = enable == 2;
    return GI_OK;
}
int gi_get_stream_counters(gi_ctx* c, int64_t* out17 /* [19] */)
{
    if (!c || !out17) return GI_E_INVALID;
    if (!c->st.d_stream_cnt.p) return fail(c, GI_E_STATE, "stream counters: no counted frame was rendered (gi_set_counters(ctx, 2), fixed sample count)");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    StreamCounters h;
    HIP_TRY(c, hipMemcpy(&h, c->st.d_stream_cnt.p, sizeof h, hipMemcpyDeviceToHost));
    for (int k = 0; k < 6; k++) { out17[k] = (int64_t)h.trace[k]; out17[7 + k] = (int64_t)h.shadow[k]; }
    out17[6] = (int64_t)h.trace_rays; out17[13] = (int64_t)h.shadow_rays;
    out17[14] = (int64_t)h.gather_queries; out17[15] = (int64_t)h.gather_cand; out17[16] = (int64_t)c->stream_shaded;
    out17[17] = (int64_t)h.trace[6]; out17[18] = (int64_t)h.shadow[6];
    return GI_OK;
}
int gi_get_counters(gi_ctx* c, int64_t* out8)
{
    if (!c || !out8) return GI_E_INVALID;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    Counters h;
    HIP_TRY(c, hipMemcpy(&h, c->st.d_counters.p, sizeof h, hipMemcpyDeviceToHost));
    out8[0] = (int64_t)h.v_trace; out8[1] = (int64_t)h.v_shadow; out8[2] = (int64_t)h.tri; out8[3] = (int64_t)h.shaded;
    out8[4] = (int64_t)h.pcand; out8[5] = (int64_t)h.traces; out8[6] = (int64_t)h.shadows; out8[7] = (int64_t)h.gathers;
    return GI_OK;
}

}  // extern "C"
