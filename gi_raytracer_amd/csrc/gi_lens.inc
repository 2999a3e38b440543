// gi_lens.inc -- the thin-lens camera (gi_set_lens, gi_get_lens, gi_lens_vertices, gi_debug_primary_rays, gi_focus_distance; an addition: the
// reference's camera is a pinhole).  Included by gi_kernels.hip behind gi_entries.inc, whose Entry the two device entries use.
//
// The lens itself is three fields of Scene (gi_path.h: lens_eye, primary_ray_at) that follow gi_ctx::lens; every pass that makes primary rays
// gets them with the Scene it is launched with.  What is here: the setter that keeps those fields and the vertex table, and two small kernels.

// the rays of the samples with the given Halton indices, as every pass builds them
__global__ __launch_bounds__(GI_BLOCK) void k_primary_rays(Scene S, Frame F, int n, const uint32_t* idx, double* rays)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const Ray r = primary_ray_at(S, F, idx[i]);
    double* o = rays + (size_t)i * 6;
    o[0] = r.o.x; o[1] = r.o.y; o[2] = r.o.z; o[3] = r.d.x; o[4] = r.d.y; o[5] = r.d.z;
}

// autofocus: the pinhole ray through (dx, dy) traced as a primary ray of stream 0; out2 = {hit ? 1 : 0, length(hit - eye) dot(dir, fwd)}
__global__ void k_focus(Scene S, Frame F, V3 fwd, double dx, double dy, double* out2)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const V3 eye = F.cam_pos;
    const Ray ray = make_ray(eye, normalize(pixel_pos(F, dx, dy) - eye));
    const Rng rng = rng_make(F.seed, 0u);   // depth 0
    HitRec h;
    const bool ok = trace(S, ray, rng, P_TRACE_ALPHA, h, nullptr);
    out2[0] = ok ? 1.0 : 0.0;
    out2[1] = ok ? length(h.pos - ray.o) * dot(ray.d, fwd) : 0.0;
}

extern "C" {

void gi_lens_default(gi_lens* l)
{
    if (!l) return;
    l->radius = 0.0; l->rotation = 0.0; l->blades = 6; l->reserved = 0;
}

int gi_lens_vertices(const gi_lens* l, double* xy)
{
    if (!lens_valid(l) || !xy) return GI_E_INVALID;
    lens_vertices(*l, xy);
    return GI_OK;
}

int gi_set_lens(gi_ctx* c, const gi_lens* l)
{
    if (!c) return GI_E_INVALID;
    if (!lens_valid(l)) return fail(c, GI_E_INVALID, "set_lens: radius must be finite and >= 0, blades 3 .. 16, rotation finite, reserved 0");
    if (c->prog.open) return fail(c, GI_E_STATE, "set_lens: a progressive session is open (its samples were taken under the lens it began with)");
    if (l->radius > 0) {
        double xy[2 * (GI_LENS_MAX_BLADES + 1)] = {0};
        lens_vertices(*l, xy);
        HIP_TRY(c, hipSetDevice(c->device));
        HIP_TRY(c, hipStreamSynchronize(c->stream));      // no pass in flight still reads the table
        if (!c->lens.d_verts.p) HIP_TRY(c, c->lens.d_verts.alloc(2 * (GI_LENS_MAX_BLADES + 1)));
        HIP_TRY(c, hipMemcpy(c->lens.d_verts.p, xy, sizeof xy, hipMemcpyHostToDevice));
        c->S.lens_verts = c->lens.d_verts.p; c->S.lens_radius = l->radius; c->S.lens_blades = l->blades;
    } else {
        c->S.lens_verts = nullptr; c->S.lens_radius = 0.0; c->S.lens_blades = 0;
    }
    c->lens.lens = *l;
    return GI_OK;
}

int gi_get_lens(gi_ctx* c, gi_lens* l)
{
    if (!c || !l) return GI_E_INVALID;
    *l = c->lens.lens;
    return GI_OK;
}

int gi_debug_primary_rays(gi_ctx* c, const gi_render_params* p, int32_t n, const uint32_t* idx, double* rays)
{
    if (!c || n < 0 || (n && (!idx || !rays))) return GI_E_INVALID;
    Frame F;
    std::string ferr;
    if (!make_frame(p, F, ferr)) return fail(c, GI_E_INVALID, ferr);
    if (n == 0) return GI_OK;
    const size_t N = (size_t)n;
    Entry e(c, "primary_rays");
    const uint32_t* d_i = e.in(idx, N);
    double* d_r = e.out(rays, N * 6);
    return e.run([&] { hipLaunchKernelGGL(k_primary_rays, GI_GRID(n), 0, c->stream, c->S, F, n, d_i, d_r); });
}

int gi_focus_distance(gi_ctx* c, const gi_render_params* p, int32_t x, int32_t y, double* dist)
{
    if (!c || !dist) return GI_E_INVALID;
    if (!c->scene.have_scene) return fail(c, GI_E_STATE, "focus_distance: no scene uploaded");
    Frame F;
    std::string ferr;
    if (!make_frame(p, F, ferr)) return fail(c, GI_E_INVALID, ferr);
    if (x < 0 || y < 0 || x >= F.w || y >= F.h) return fail(c, GI_E_INVALID, "focus_distance: pixel (" + std::to_string(x) + ", " + std::to_string(y) + ") outside the frame");
    double h2[2] = {0, 0};
    Entry e(c, "focus_distance");
    double* d_o = e.out(h2, 2);
    const int rc = e.run([&] { hipLaunchKernelGGL(k_focus, dim3(1), dim3(64), 0, c->stream, c->S, F, ld3(p->cam_forward), x + .5, y + .5, d_o); });
    if (rc) return rc;
    if (h2[0] == 0.0) return 1;
    *dist = h2[1];
    return GI_OK;
}

}  // extern "C"
