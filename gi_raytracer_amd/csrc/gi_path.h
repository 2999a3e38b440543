// gi_path.h -- a path from the camera or a light: ray_type, secondary_ray, shading_normal, PathRec and ShadowQ, the stage_* functions (the
// gather's stage glue among them), coherence_key, radiance_path, then Frame, the primary ray with the thin lens, PixelState and the pixel rule,
// and photon emission.  Needs every part above it, gi_gather.h included.  Included by gi_device.h inside namespace gi, last.
//
// Reference semantics followed (file:line relative to moepforfreedom/GI_Raytracer):
//   secondaryRay     include/raytracer.h:321-379, rayType :481-506
//   radiance         include/raytracer.h:167-276 (recursion turned into a loop carrying the path throughput)
//   primary ray      include/raytracer.h:102-148
//   tracePhotons     include/raytracer.h:582-715

// ------------------------------------------------------------------------------------------------ shading
// RayTracer::rayType, include/raytracer.h:481-506
GI_HD int ray_type(const Mat& m, double tex_a, const Ray& ray, V3 norm, const Rng& rng)
{
    int type = 2;
    if (m.roughness < .001) type = 0;
    double opacity = tex_a * m.opacity;   // diffuse->getAlpha(minUV) * opacity, include/raytracer.h:486
    if (opacity < 1.0) {  // drand() in [0,1) can exceed the opacity only then
        if (rng_draw(rng, P_TYPE_OPACITY) > opacity) {
            double r0 = pow((1 - m.ior) / (1 + m.ior), 2.0);
            double fs = r0 + (1 - r0) * pow(1 - dot(reflect(ray.d, norm), norm), 5.0);
            if (rng_draw(rng, P_TYPE_FRESNEL) < fs) type = 0;
            else type = 1;
        }
    }
    return type;
}
// RayTracer::secondaryRay, include/raytracer.h:321-379
GI_HD void secondary_ray(const Ray& ray, const Mat& m, V3 color, double tex_a, V3& norm, double sx, double sy, V3& refDir, V3& f, double& roughness, V3& contrib, double& offset, const Rng& rng)
{
    // color = diffuse->get(UV), tex_a = diffuse->getAlpha(UV) (1 and the constant colour without GI_FEAT_TEX)
    bool backface = false;
    if (dot(norm, ray.d) > 0) { norm = norm * -1.0; backface = true; }
    roughness = m.roughness;
    int type = ray_type(m, tex_a, ray, norm, rng);
    if (type == 1) {
        refDir = backface ? refr(ray.d, norm, m.ior) : refr(ray.d, norm, 1.0 / m.ior);
        offset *= -1;
        contrib = v3(1, 1, 1);
        f = 1.0 * color;
    } else if (type == 0) {
        refDir = reflect(ray.d, norm);
        contrib = v3(1, 1, 1);
        f = 1.0 * color;
    } else {
        if (m.roughness < .9) {
            refDir = sample_phong(reflect(ray.d, norm), (1.0 / (m.roughness)) + 1, sx, sy);
            if (dot(refDir, norm) < 0) refDir = reflect(refDir, norm);
        } else
            refDir = hemi_cos_n(norm, (float)sx, (float)sy, 2);
        f = 1.0 * color;
        V3 inf = color;
        contrib = contrib * inf;
        contrib = mix(contrib, inf, 0.5);
    }
}
GI_HD V3 shading_normal(const Scene& S, const HitRec& h)  // include/entities.h:478-485
{
    const TriShade& sh = S.shade[h.tri];
    if (h.mf & 4u) return normalize(h.pos - ld3(sh.n0));   // sphere: normalize(intersect - pos), include/entities.h:84
    if (h.mf & 1u) return (1 - h.u - h.v) * ld3(sh.n0) + h.u * ld3(sh.n1) + h.v * ld3(sh.n2);
    return ld3(sh.fnorm);
}

// ---- one path as explicit stages (the recursion of RayTracer::radiance turned into a loop carrying the throughput).
// L = A_0 + f_0 (A_1 + f_1 (A_2 + ...)) is accumulated as sum_k (prod_{j<k} f_j) A_k with A = color*i + emissive (+ color*caustic,
// added by the gather stage) on continue, color*i on a failed roulette, ambient on a miss and 0 past MAX_DEPTH.
// The megakernel and the finisher run the stages back to back per lane on a PathRec in registers; the streaming passes run each
// stage as its own kernel over compacted queues of path slots, on the same fields kept as field arrays (PathPool, gi_pool.h).
struct alignas(16) PathRec {    // 224 B, one path (in registers; the streaming pool stores the same fields as arrays)
    double o[3], d[3];          // current ray (d normalised)
    uint32_t stream;            // Halton sample index = RNG stream
    int32_t depth;              // -1: slot unused
    int32_t htri;
    uint32_t pad;               // matflags of the hit (material << 3 | flags): the shade stage needs no entity record for them
                                // -- the first 64 B are all a new path needs and all the trace stage reads
    double T[3], contrib[3];    // throughput prod f_j ; the reference's `contrib` (roulette weight).  At depth 0 they are 1 and L is 0 by
                                // definition: the stages do not read them there, so a new path does not have to write them (path_begin_lean)
    double gdir[3], gcoef[3];   // pending photon gather: direction (= refDir) and factor T*color -- bytes 0 .. 159 are what the shade stage writes
                                // (five whole 32-byte sectors of a 32-byte aligned record), 112 .. 183 what the gather stage reads
    double hpos[3], hu, hv;     // hit of the current segment
    double L[3];                // radiance so far where the path is advanced in registers (finisher, megakernel); idle in the streaming passes
};
static_assert(sizeof(PathRec) == 224, "PathRec layout");
enum { ST_CONTINUE = 1, ST_GATHER = 2 };

template <class P>
GI_HD void path_begin_lean(P& p, const Ray& ray, uint32_t sample)   // one 64-byte store: what a depth-0 path consists of (P: PathRec, or the streaming pool's PathRef)
{
    p.o[0] = ray.o.x; p.o[1] = ray.o.y; p.o[2] = ray.o.z;
    p.d[0] = ray.d.x; p.d[1] = ray.d.y; p.d[2] = ray.d.z;
    p.stream = sample; p.depth = 0; p.htri = -1; p.pad = 0;
}
GI_HD void path_begin(PathRec& p, const Ray& ray, uint32_t sample)
{
    p.o[0] = ray.o.x; p.o[1] = ray.o.y; p.o[2] = ray.o.z;
    p.d[0] = ray.d.x; p.d[1] = ray.d.y; p.d[2] = ray.d.z;
    for (int k = 0; k < 3; k++) { p.T[k] = 1; p.contrib[k] = 1; p.L[k] = 0; }
    p.stream = sample; p.depth = 0; p.htri = -1; p.pad = 0;
}
// stage 1: RayTracer::trace for the current segment.  Miss: L += T*ambient and the path is finished (returns false).
template <int FEAT, class Nodes>
GI_HD bool stage_trace_nodes(const Scene& S, const Nodes& N, PathRec& p, uint64_t seed, Counters* c)
{
    Rng rng = rng_make(seed, p.stream);
    rng.depth = (uint32_t)p.depth;
    Ray ray = make_ray_exact(ld3(p.o), ld3(p.d));
    HitRec h;
    if (!trace_nodes<FEAT>(S, N, ray, rng, P_TRACE_ALPHA, h, c)) {
        const bool first = p.depth == 0;   // L = 0, T = 1 (PathRec)
        V3 L = (first ? v3(0, 0, 0) : ld3(p.L)) + (first ? v3(1, 1, 1) : ld3(p.T)) * ld3(S.ambient);
        p.L[0] = L.x; p.L[1] = L.y; p.L[2] = L.z;
        return false;
    }
    p.hpos[0] = h.pos.x; p.hpos[1] = h.pos.y; p.hpos[2] = h.pos.z;
    p.hu = h.u; p.hv = h.v; p.htri = h.tri; p.pad = h.mf;
    if (FEAT & GI_FEAT_TEX) { p.gdir[0] = h.tu; p.gdir[1] = h.tv; }   // minUV rides in the (idle between gather and shade) gather fields
    return true;
}
GI_HD bool stage_trace(const Scene& S, PathRec& p, uint64_t seed, Counters* c)
{
    if (S.wnodes && !c) {
        GlobalWide W;
        W.g = S.wnodes; W.cboxes = S.tcboxes; W.cuse = S.tcuse;
        return S.n_tex > 0 ? stage_trace_nodes<7>(S, W, p, seed, nullptr) : stage_trace_nodes<3>(S, W, p, seed, nullptr);
    }
    GlobalNodes N;
    N.g = S.tnodes;
    return S.n_tex > 0 ? stage_trace_nodes<7>(S, N, p, seed, c) : stage_trace_nodes<3>(S, N, p, seed, c);
}
// coherence key of a continuing ray: direction octant (selects the order the children are walked in), Morton code of the origin inside the
// root box, coarse direction -- rays that are neighbours in this order walk the same nodes for about the same number of steps
GI_HD uint32_t coherence_key(const Scene& S, V3 o, V3 d)
{
    uint32_t m = 0;
    uint32_t q[3];
    const double oo[3] = {o.x, o.y, o.z}, dd[3] = {d.x, d.y, d.z};
    for (int k = 0; k < 3; k++) {
        double f = (oo[k] - S.root_bmin[k]) / (S.root_bmax[k] - S.root_bmin[k]);
        f = f < 0.0 ? 0.0 : (f > 0.999 ? 0.999 : f);
        q[k] = (uint32_t)(f * 64.0);
    }
    for (int b = 5; b >= 0; b--) m = (m << 3) | (((q[0] >> b) & 1u) << 2) | (((q[1] >> b) & 1u) << 1) | ((q[2] >> b) & 1u);
    const uint32_t oct = (dd[0] < 0.0 ? 1u : 0u) | (dd[2] < 0.0 ? 2u : 0u) | (dd[1] < 0.0 ? 4u : 0u);
    uint32_t db = 0;
    for (int k = 0; k < 3; k++) { double a = fabs(dd[k]); db = (db << 2) | (uint32_t)(a >= 0.999 ? 3.0 : a * 4.0); }
    return (oct << 24) | (m << 6) | db;
}
struct ShadeOut { uint32_t key; V3 gpos; };   // by-products of the shade stage for the queues: sort key of the next ray, position of the gather query
// A shadow query put off: with one light the vertex adds either A = T * (color * i + emissive) -- light visible -- or A0 = T * (color * 0 +
// emissive) to the path's radiance, so the shade stage can leave the walk to a kernel of its own (k_st_shadow: lanes take a new query as
// soon as theirs is answered) that adds the one or the other to the per-sample buffer.  A0 is zero unless the surface emits; then it waits
// in the record's (otherwise idle) L field.  Same bits as the inline form.
struct alignas(16) ShadowQ { double o[3], dir[3], A[3]; uint32_t idx, stream; int32_t depth; uint32_t live, slot, pad; };   // 96 B; idx = the sample's place in the radiance buffer; live: 0 no query, 1 query, 2 query + A0
// stage 2: shading of the hit: secondaryRay, direct light with shadow rays, Russian roulette, next ray.
// Lext: where the path's radiance accumulates when it does not live in the record (streaming pipeline: the per-sample radiance buffer,
// so that a path that ends -- 96 % of the benchmark's reflected rays leave the scene -- has nothing left to read or write); else p.L.
// DEFER (1: scenes with one light, 2: with several): the shadow walks are put off (sq), this function then contains no walk and touches no radiance at all.
template <int FEAT, class Nodes, int DEFER = 0, class P = PathRec>
GI_HD int stage_shade_nodes(const Scene& S, const Nodes& N, P& p, uint64_t seed, Counters* c, ShadeOut* so = nullptr, double* Lext = nullptr, ShadowQ* sq = nullptr)
{
    double* const Lp = Lext ? Lext : p.L;
    Rng rng = rng_make(seed, p.stream);
    const int depth = p.depth;
    rng.depth = (uint32_t)depth;
    if (c) c->shaded++;
    Ray ray = make_ray_exact(ld3(p.o), ld3(p.d));
    HitRec h;
    h.pos = ld3(p.hpos); h.u = p.hu; h.v = p.hv; h.tri = p.htri; h.mf = p.pad;
    float sx = halton_sample(S, 2 + 2 * depth, p.stream);
    float sy = halton_sample(S, 3 + 2 * depth, p.stream);
    const Mat& m = S.mats[h.mf >> 3];
    V3 norm = shading_normal(S, h);
    V3 color = ld3(m.diffuse), emissive = ld3(m.emissive);
    double tex_a = 1;
    if (FEAT & GI_FEAT_TEX) {   // diffuse->get(minUV), emissive->get(minUV), diffuse->getAlpha(minUV): include/raytracer.h:200,269,486
        const double tu = p.gdir[0], tv = p.gdir[1];
        color = tex_get(S, m.dtex, color, tu, tv);
        emissive = tex_get(S, m.etex, emissive, tu, tv);
        tex_a = tex_alpha(S, m.dtex, tu, tv);
    }
    V3 refDir, f = v3(1, 1, 1), i = v3(0, 0, 0), contrib = depth == 0 ? v3(1, 1, 1) : ld3(p.contrib);
    double roughness, offset = GI_SHADOW_BIAS;
    secondary_ray(ray, m, color, tex_a, norm, sx, sy, refDir, f, roughness, contrib, offset, rng);
    if ((FEAT & GI_FEAT_FOG) && S.n_fog > 0) {   // include/raytracer.h:209-228: the segment may end in the medium instead
        double tmin = 0, tmx = length(h.pos - ray.o);
        if (atmosphere_bounds(S, ray, tmin, tmx)) {
            V3 fh, col;
            if (raymarch(S, ray, fh, col, tmin, tmx, rng, P_FOG_CAMERA)) {
                h.pos = fh;
                p.hpos[0] = fh.x; p.hpos[1] = fh.y; p.hpos[2] = fh.z;   // the gather of this vertex uses the scatter point too
                refDir = random_unit_vec(sx, sy);
                f = 1.0 * col;
                color = col;
                contrib = col;
                roughness = 1;
            }
        }
    }
    constexpr bool defer = DEFER != 0, multi = DEFER == 2;   // DEFER 2: several lights, one query each (sq[li]); k_st_shadow asks them from the last light down
    const bool emits = emissive.x != 0.0 || emissive.y != 0.0 || emissive.z != 0.0;
    const int n_def = multi ? S.n_light : 1;
    if (defer) for (int li = 0; li < n_def; li++) { sq[li].live = (li == 0 && emits) ? 2u : 1u; sq[li].stream = p.stream; sq[li].depth = depth; }
    for (int li = 0; li < (defer ? n_def : S.n_light); li++) {
        const LightD& lt = S.lights[li];
        double ry = rng_draw(rng, P_LIGHT_Y | ((uint32_t)li << 8));
        double rx = rng_draw(rng, P_LIGHT_X | ((uint32_t)li << 8));
        V3 lpos = ld3(lt.pos);
        V3 so = h.pos + GI_SHADOW_BIAS * norm;
        V3 lightDir = (lpos + lt.rad * random_unit_vec(rx, ry)) - so;
        double maxt = len2(lightDir);
        double hfrac = 1 / (GI_PI * len2(lpos - h.pos));
        bool vis = true;
        if constexpr (defer) {   // the walk happens in k_st_shadow, from these two vectors
            sq[li].o[0] = so.x; sq[li].o[1] = so.y; sq[li].o[2] = so.z;
            sq[li].dir[0] = lightDir.x; sq[li].dir[1] = lightDir.y; sq[li].dir[2] = lightDir.z;
        } else {
            Ray sray = make_ray(so, lightDir);
            vis = visible_nodes<FEAT>(S, N, sray, maxt, rng, (uint32_t)li, c);
        }
        if (vis) {
            double d = dot(norm, normalize(lpos - h.pos));
            if (d < 0) d = 0;
            // pow(d, 1/roughness): exact shortcuts for the two exponents every constant-texture scene uses (x^1 = x; x^inf for a
            // mirror: 0 below 1, 1 at 1), the general case through pow()
            const double ex = (1.0 / roughness);
            double l = ex == 1.0 ? d : (ex == INFINITY ? (d < 1.0 ? 0.0 : (d == 1.0 ? 1.0 : INFINITY)) : pow(d, ex));
            i = ld3(lt.col) * l * hfrac;
        }
        if constexpr (multi) { sq[li].A[0] = i.x; sq[li].A[1] = i.y; sq[li].A[2] = i.z; }   // this light's share, until T is known below
    }
    p.contrib[0] = contrib.x; p.contrib[1] = contrib.y; p.contrib[2] = contrib.z;
    V3 T = depth == 0 ? v3(1, 1, 1) : ld3(p.T), L = (defer || depth == 0) ? v3(0, 0, 0) : ld3(Lp);
    double q = comp_max(contrib);
    if (depth <= GI_MIN_DEPTH || rng_draw(rng, P_RR) < q) {
        f = f * (depth <= GI_MIN_DEPTH ? 1.0 : (1.0 / q));
        if constexpr (defer) {
            for (int li = 0; li < n_def; li++) {
                const V3 il = multi ? ld3(sq[li].A) : i;
                const V3 A = T * (color * il + emissive);
                sq[li].A[0] = A.x; sq[li].A[1] = A.y; sq[li].A[2] = A.z;
            }
            if (emits) { const V3 A0 = T * (color * v3(0, 0, 0) + emissive); p.L[0] = A0.x; p.L[1] = A0.y; p.L[2] = A0.z; }
        } else {
            L = L + T * (color * i + emissive);
            Lp[0] = L.x; Lp[1] = L.y; Lp[2] = L.z;
        }
        int flags = 0;
        if (depth <= 10 && S.n_pnode > 0) {   // caustic = depth <= 10 ? samplePhotons(minHit, refDir, 32) : 0, include/raytracer.h:258
            V3 gc = T * color;
            p.gdir[0] = refDir.x; p.gdir[1] = refDir.y; p.gdir[2] = refDir.z;
            p.gcoef[0] = gc.x; p.gcoef[1] = gc.y; p.gcoef[2] = gc.z;
            flags |= ST_GATHER;
        }
        T = T * f;
        p.T[0] = T.x; p.T[1] = T.y; p.T[2] = T.z;
        Ray next = make_ray(h.pos + offset * norm, refDir);
        p.o[0] = next.o.x; p.o[1] = next.o.y; p.o[2] = next.o.z;
        p.d[0] = next.d.x; p.d[1] = next.d.y; p.d[2] = next.d.z;
        p.depth = depth + 1;
        if (so) { so->key = coherence_key(S, next.o, next.d); so->gpos = h.pos; }
        if (p.depth <= GI_MAX_DEPTH) flags |= ST_CONTINUE;   // radiance() returns 0 past MAX_DEPTH
        return flags;
    }
    if constexpr (defer) {
        for (int li = 0; li < n_def; li++) {
            const V3 il = multi ? ld3(sq[li].A) : i;
            const V3 A = T * (color * il);
            sq[li].A[0] = A.x; sq[li].A[1] = A.y; sq[li].A[2] = A.z;
        }
        if (emits) sq[0].live = 1u;   // the path ends without the surface's own light: the hidden case adds T * (color * 0) = 0
    } else {
        L = L + T * (color * i);
        Lp[0] = L.x; Lp[1] = L.y; Lp[2] = L.z;
    }
    return 0;
}
GI_HD int stage_shade(const Scene& S, PathRec& p, uint64_t seed, Counters* c)
{
    if (S.wnodes && !c) {
        GlobalWide W;
        W.g = S.wnodes; W.cboxes = S.cboxes; W.cuse = S.cuse;
        return S.n_tex > 0 ? stage_shade_nodes<7>(S, W, p, seed, nullptr) : stage_shade_nodes<3>(S, W, p, seed, nullptr);
    }
    GlobalNodes N;
    N.g = S.tnodes;
    return S.n_tex > 0 ? stage_shade_nodes<7>(S, N, p, seed, c) : stage_shade_nodes<3>(S, N, p, seed, c);
}
// stage 3: the caustic term of the vertex just shaded: L += (T*color) * samplePhotons(hit, refDir, 32)
template <class P>
GI_HD void stage_gather_in_leaf(const Scene& S, P& p, int32_t leaf, float* heap_mem, int heap_stride, double* Lext = nullptr)
{
    gather_add(Lext ? Lext : p.L, p.gcoef, gather_in_leaf(S, leaf, ld3(p.hpos), ld3(p.gdir), heap_mem, heap_stride, nullptr, nullptr));
}
GI_HD void stage_gather(const Scene& S, PathRec& p, float* heap_mem, int heap_stride, Counters* c)
{
    gather_add(p.L, p.gcoef, gather(S, ld3(p.hpos), ld3(p.gdir), heap_mem, heap_stride, nullptr, c));
}
// the stages back to back for one lane (megakernel, function-level entry points)
GI_HD V3 radiance_path(const Scene& S, Ray ray, uint32_t sample, uint64_t seed, float* heap_mem, int heap_stride, Counters* c)
{
    PathRec p;
    path_begin(p, ray, sample);
    for (;;) {
        if (!stage_trace(S, p, seed, c)) break;
        const int fl = stage_shade(S, p, seed, c);
        if (fl & ST_GATHER) stage_gather(S, p, heap_mem, heap_stride, c);
        if (!(fl & ST_CONTINUE)) break;
    }
    return ld3(p.L);
}

// ------------------------------------------------------------------------------------------------ camera / pixel loop
struct Frame {
    V3 cam_pos, cam_up, screen_center, right;
    double sw, sh;
    int32_t w, h;
    HaltonEnumD he;
    int32_t min_samples, max_samples;
    double noise_thresh;
    uint64_t seed;
    int32_t stripe_h, stripe_rank, stripe_world, local_rows;
};
// primary ray of sample s of pixel (x,y): include/raytracer.h:112-129 (FOCAL_BLUR == 0), and the thin lens that stands in for FOCAL_BLUR (an addition)
template <bool LENS = true> GI_HD Ray primary_ray_at(const Scene& S, const Frame& F, uint32_t idx);
GI_HD Ray primary_ray(const Scene& S, const Frame& F, int s, int x, int y, uint32_t& idx)
{
    idx = halton_index(F.he, (uint32_t)s, (uint32_t)x, (uint32_t)y);
    return primary_ray_at(S, F, idx);
}
// the point of the sensor plane at (dx, dy) pixels from the frame's top left corner: the plane that stays sharp under a lens
GI_HD V3 pixel_pos(const Frame& F, double dx, double dy)
{
    return F.screen_center + (F.sw * (dx / F.w - .5)) * F.right - (F.sh * (dy / F.h - .5)) * F.cam_up;
}
// The eye of the sample with Halton index idx on a lens of S.lens_radius > 0 (gi_hip.h: gi_set_lens states the order of operations): a point drawn
// uniformly by area from the regular polygon S.lens_verts in the plane of F.right and F.cam_up.  u0 picks the blade's triangle (centre, v_k, v_k+1)
// and the distance from the centre, u1 the place between the two vertices.  IEEE operations only -- the vertices were computed on the host.
enum { P_LENS_U = 34, P_LENS_V = 35 };  // RNG purposes of the two numbers (seed, stream idx, depth 0, a = 0)
GI_HD V3 lens_eye(const Scene& S, const Frame& F, uint32_t idx)
{
    const Rng rng = rng_make(F.seed, idx);   // depth 0
    const double u0 = rng_draw(rng, P_LENS_U);
    const double u1 = rng_draw(rng, P_LENS_V);
    const int32_t B = S.lens_blades;
    const double ub = u0 * B;
    int32_t k = (int32_t)ub;
    if (k > B - 1) k = B - 1;
    const double r = sqrt(ub - k);
    const double* v = S.lens_verts + 2 * k;
    const double lx = r * ((1 - u1) * v[0] + u1 * v[2]);
    const double ly = r * ((1 - u1) * v[1] + u1 * v[3]);
    return F.cam_pos + (S.lens_radius * lx) * F.right + (S.lens_radius * ly) * F.cam_up;
}
// LENS = false: an instance that is launched for pinholes only and carries no code for the lens (k_st_trace, where the branch cost registers)
template <bool LENS> GI_HD Ray primary_ray_at(const Scene& S, const Frame& F, uint32_t idx)   // the ray of the sample with Halton index idx (the index names the pixel too: Halton_enum)
{
    double xr = halton_sample(S, 0, idx);
    double yr = halton_sample(S, 1, idx);
    double dx = (float)((float)xr * F.he.scale_x);
    double dy = (float)((float)yr * F.he.scale_y);
    V3 pixelPos = pixel_pos(F, dx, dy);
    V3 eyePos = F.cam_pos;
    if (LENS && S.lens_radius > 0) eyePos = lens_eye(S, F, idx);   // uniform per launch; a pinhole makes no draw
    return make_ray(eyePos, normalize(pixelPos - eyePos));
}
// adaptive per-pixel loop state: include/raytracer.h:102-148
struct PixelState { V3 color, lastCol; double var; int samps, s; };
GI_HD void pixel_begin(PixelState& p) { p.color = v3(0.5, 0.5, 0.5); p.lastCol = v3(0, 0, 0); p.var = 0; p.samps = 0; p.s = 0; }
GI_HD bool pixel_wants_sample(const PixelState& p, const Frame& F) { return p.s < F.max_samples && p.samps < F.min_samples; }
GI_HD void pixel_add_sample(PixelState& p, const Frame& F, V3 L)
{
    p.lastCol = p.color;
    if (p.s == 0) p.color = L;
    else p.color = (1.0 * p.s * p.color + L) * (1.0 / (p.s + 1));
    if (p.s > 0) p.var = (1.0 * 5 * p.var + length(p.color - p.lastCol)) * (1.0 / (5 + 1));
    if (p.s > 0 && p.var > F.noise_thresh) p.samps -= 2;
    p.s++;
    p.samps++;
}
// local row r of this rank -> frame row (interleaved stripes)
GI_HD int global_row(const Frame& F, int r) { return ((r / F.stripe_h) * F.stripe_world + F.stripe_rank) * F.stripe_h + r % F.stripe_h; }

// ------------------------------------------------------------------------------------------------ photon emission (tracePhotons)
struct PhotonOut { double v[9]; };
// one (photon index i, light li): up to 500 emission tries; returns true and fills out when a caustic photon is stored
GI_HD bool emit_photon(const Scene& S, int32_t i, int32_t li, int32_t count, int32_t max_depth, uint64_t seed, PhotonOut& out, int32_t& tries_out)
{
    const LightD& l = S.lights[li];
    Rng rng = rng_make(seed ^ GI_PHOTON_SEED_XOR, (uint32_t)i * (uint32_t)S.n_light + (uint32_t)li);
    int tries = 0;
    bool stored = false;
    V3 lpos = ld3(l.pos);
    while (!stored && tries < 500) {
        rng.depth = (uint32_t)tries * 16u;
        float sx = halton_sample(S, 0, (uint32_t)(i * 500 + tries));
        float sy = halton_sample(S, 1, (uint32_t)(i * 500 + tries));
        // Light::getPointInRange, include/light.h:47-53
        V3 pos = l.angle < 1 ? lpos + l.rad * sphere_cap_cos(ld3(l.dir), sx, sy, 1, l.angle) : lpos + l.rad * random_unit_vec(sx, sy);
        double d13 = rng_draw(rng, P_PH_DIR_V);
        double d5 = rng_draw(rng, P_PH_DIR_U);
        V3 dir = sphere_cap_cos(normalize(pos - lpos), (float)fmod(d5 + 5 * i, 1.0), (float)fmod(d13 + 13 * i, 1.0), 2, l.angle);
        Ray r = make_ray(pos, dir);
        V3 col = (1.0 / count) * .5 * l.angle * ld3(l.col);
        HitRec h;
        int depth = 0;
        bool term = false, isCaustic = false;
        if (!trace(S, r, rng, P_PH_TRACE0_ALPHA, h, nullptr)) { tries++; continue; }
        V3 hit = h.pos;
        while (depth < max_depth && !term) {
            rng.depth = (uint32_t)tries * 16u + (uint32_t)depth + 1u;
            double roughness = S.mats[h.mf >> 3].roughness;
            if (roughness < 0.1) {
                if (!trace(S, r, rng, P_TRACE_ALPHA, h, nullptr)) { term = true; continue; }
                hit = h.pos;
                const Mat& m = S.mats[h.mf >> 3];
                V3 norm = shading_normal(S, h);
                V3 refDir, f, contrib = v3(0, 0, 0);
                double offset = GI_SHADOW_BIAS;
                double e13 = rng_draw(rng, P_PH_SEC_V);
                double e5 = rng_draw(rng, P_PH_SEC_U);
                V3 pcolor = ld3(m.diffuse);
                double tex_a = 1;
                if (S.n_tex > 0) { pcolor = tex_get(S, m.dtex, pcolor, h.tu, h.tv); tex_a = tex_alpha(S, m.dtex, h.tu, h.tv); }
                secondary_ray(r, m, pcolor, tex_a, norm, fmod(e5 + 5 * i, 1.0), fmod(e13 + 13 * i, 1.0), refDir, f, roughness, contrib, offset, rng);
                if (S.n_fog > 0) {   // include/raytracer.h:658-675
                    double tmin = 0, tmx = length(hit - r.o);
                    if (atmosphere_bounds(S, r, tmin, tmx)) {
                        V3 ahit, fcol;
                        if (raymarch(S, r, ahit, fcol, tmin, tmx, rng, P_FOG_PHOTON)) {
                            hit = ahit;
                            double g7 = rng_draw(rng, P_PH_FOG_V);
                            double g13 = rng_draw(rng, P_PH_FOG_U);
                            refDir = random_unit_vec(fmod(g13 + 13 * i, 1.0), fmod(g7 + 7 * i, 1.0));
                            f = 1.0 * fcol;
                            roughness = 1;
                        }
                    }
                }
                col = col * f;
                r = make_ray(hit + offset * norm, refDir);
                isCaustic = true;
            }
            if (depth > 0 && isCaustic && roughness >= 0.1) {
                out.v[0] = hit.x; out.v[1] = hit.y; out.v[2] = hit.z;
                out.v[3] = r.d.x; out.v[4] = r.d.y; out.v[5] = r.d.z;
                out.v[6] = col.x; out.v[7] = col.y; out.v[8] = col.z;
                term = true;
                stored = true;
            }
            depth++;
        }
        tries++;
    }
    tries_out = tries;
    return stored;
}
