// gi_intersect.h -- a ray against one thing: boxes, the height fog (atmosphere_bounds, raymarch), the triangle and the sphere, HitRec, the
// wave-uniform leaf loads, textures, and the entity test with its alpha rule (ent_hit, ent_uv, ent_accepts, ent_blocks).  No tree is walked here.
// Needs gi_scene.h and gi_math.h.  Included by gi_device.h inside namespace gi, behind gi_math.h.
//
// Reference semantics followed (file:line relative to moepforfreedom/GI_Raytracer):
//   box tests        include/bbox.h:47-73,117-138
//   triangle test    include/entities.h:443-490, sphere :60-101
//   fog              include/atmosphere.h:30-83, include/octree.cpp:214-251, include/raytracer.h:509-529
//   textures         include/material.h:10-93

// ------------------------------------------------------------------------------------------------ boxes
// BoundingBox::intersect(ray, 0, inf) reduced to the hit flag (t0 is only used for ordering, which the direction-ordered
// tree provides) -- same slab arithmetic and early-outs as include/bbox.h:47-73 / :117-138.
GI_HD bool box_hit(const double* bmin, const double* bmax, const Ray& r, double tmin, double tmax)
{
    {
        double t0 = (bmin[0] - r.o.x) * r.inv.x, t1 = (bmax[0] - r.o.x) * r.inv.x;
        if (r.inv.x < 0.0) { double t = t0; t0 = t1; t1 = t; }
        tmin = t0 > tmin ? t0 : tmin;
        tmax = t1 < tmax ? t1 : tmax;
        if (tmax <= tmin) return false;
    }
    {
        double t0 = (bmin[1] - r.o.y) * r.inv.y, t1 = (bmax[1] - r.o.y) * r.inv.y;
        if (r.inv.y < 0.0) { double t = t0; t0 = t1; t1 = t; }
        tmin = t0 > tmin ? t0 : tmin;
        tmax = t1 < tmax ? t1 : tmax;
        if (tmax <= tmin) return false;
    }
    {
        double t0 = (bmin[2] - r.o.z) * r.inv.z, t1 = (bmax[2] - r.o.z) * r.inv.z;
        if (r.inv.z < 0.0) { double t = t0; t0 = t1; t1 = t; }
        tmin = t0 > tmin ? t0 : tmin;
        tmax = t1 < tmax ? t1 : tmax;
        if (tmax <= tmin) return false;
    }
    return true;
}
GI_HD bool box_contains(const double* bmin, const double* bmax, V3 p)  // include/bbox.h:41-44 (half open)
{
    return p.x >= bmin[0] && p.y >= bmin[1] && p.z >= bmin[2] && p.x < bmax[0] && p.y < bmax[1] && p.z < bmax[2];
}
// BoundingBox::intersect(ray, tmin, tmax, toutmin, toutmax), include/bbox.h:47-73
GI_HD bool box_range(const double* bmin, const double* bmax, const Ray& r, double tmin, double tmax, double& t0o, double& t1o)
{
    const double o[3] = {r.o.x, r.o.y, r.o.z}, inv[3] = {r.inv.x, r.inv.y, r.inv.z};
    for (int i = 0; i < 3; i++) {
        double t0 = (bmin[i] - o[i]) * inv[i], t1 = (bmax[i] - o[i]) * inv[i];
        if (inv[i] < 0.0) { double t = t0; t0 = t1; t1 = t; }
        tmin = t0 > tmin ? t0 : tmin;
        tmax = t1 < tmax ? t1 : tmax;
        if (tmax <= tmin) return false;
    }
    t0o = tmin; t1o = tmax;
    return true;
}
GI_HD double fast_pow(double a, double b)   // include/util.h:100-111
{
    union { double d; int32_t x[2]; } u;
    u.d = a;
    u.x[1] = (int32_t)(b * (u.x[1] - 1072632447) + 1072632447);
    u.x[0] = 0;
    return u.d;
}
// HeightFog::density, include/atmosphere.h:50-81 (nscale is 1 after construction; indices are computed in double as there)
GI_HD double fog_density(const Scene& S, const FogD& f, V3 p)
{
    const double ymax = f.pos[1] + .5 * f.size[1];
    const V3 rel = v3(p.x - f.bmin[0], p.y - f.bmin[1], p.z - f.bmin[2]);
    const int rx = (int)rel.x, ry = (int)rel.y, rz = (int)rel.z;
    const double dx = (rel.x - rx), dy = (rel.y - ry), dz = (rel.z - rz);
    const double* G = S.fog_grid + f.grid_off;
    const int last = f.grid_n - 1;
#define GI_FOG_G(expr) G[((int)(expr)) < last ? (((int)(expr)) < 0 ? 0 : (int)(expr)) : last]
    const double sx = f.size[0], sz = f.size[2];
    double c00 = (1 - dx) * GI_FOG_G((rx * sx + ry) * sz + rz) + dx * GI_FOG_G(((rx + 1) * sx + ry) * sz + rz);
    double c01 = (1 - dx) * GI_FOG_G((rx * sx + ry) * sz + rz + 1) + dx * GI_FOG_G(((rx + 1) * sx + ry) * sz + rz + 1);
    double c10 = (1 - dx) * GI_FOG_G((rx * sx + (ry + 1)) * sz + rz) + dx * GI_FOG_G(((rx + 1) * sx + (ry + 1)) * sz + rz);
    double c11 = (1 - dx) * GI_FOG_G((rx * sx + (ry + 1)) * sz + rz + 1) + dx * GI_FOG_G(((rx + 1) * sx + (ry + 1)) * sz + rz + 1);
#undef GI_FOG_G
    double c0 = c00 * (1 - dy) + c10 * dy;
    double c1 = c01 * (1 - dy) + c11 * dy;
    double noise = fast_pow((1 - dz) * c0 + dz * c1, 7);
    return f.d * noise * fast_pow((ymax - p.y) / f.size[1], 2);
}
GI_HD double atmosphere_density(const Scene& S, V3 pos, V3& col)   // Octree::atmosphereDensity, include/octree.cpp:214-226
{
    double d = 0;
    for (int i = 0; i < S.n_fog; i++) {
        const FogD& f = S.fogs[i];
        if (box_contains(f.bmin, f.bmax, pos)) { col = ld3(f.col); d += GI_RAYMARCH_STEPSIZE * fog_density(S, f, pos); }
    }
    return d;
}
GI_HD bool atmosphere_bounds(const Scene& S, const Ray& r, double& mint, double& maxt)   // Octree::atmosphereBounds, include/octree.cpp:229-251
{
    double mn = 0, mx = 0;
    bool intersected = false;
    for (int i = 0; i < S.n_fog; i++) {
        double a, b;
        if (box_range(S.fogs[i].bmin, S.fogs[i].bmax, r, mint, maxt, a, b)) { mn = a < mn ? a : mn; mx = b > mx ? b : mx; intersected = true; }
    }
    mint = mint > mn ? mint : mn;
    maxt = maxt < mx ? maxt : mx;
    return intersected;
}
// RayTracer::raymarch, include/raytracer.h:509-529: absorb with probability density*step per 0.04 step
GI_HD bool raymarch(const Scene& S, const Ray& r, V3& hit, V3& col, double mint, double maxt, const Rng& rng, uint32_t which)
{
    double t = mint + GI_SHADOW_BIAS;
    V3 current = r.o + mint * r.d;
    uint32_t step = 0;
    while (t < maxt) {
        if (rng_draw(rng, P_FOG, step, which) < atmosphere_density(S, current, col)) { hit = current; return true; }
        current = current + GI_RAYMARCH_STEPSIZE * r.d;
        t += GI_RAYMARCH_STEPSIZE;
        step++;
    }
    return false;
}
// child visiting order: the reference numbers children x = bit0, z = bit1, y = bit2 (include/octree.cpp:321-328)
GI_HD int dir_octant(const Ray& r) { return (r.d.x < 0.0 ? 1 : 0) | (r.d.z < 0.0 ? 2 : 0) | (r.d.y < 0.0 ? 4 : 0); }

// ------------------------------------------------------------------------------------------------ triangle (include/entities.h:443-490)
template <class Tri>
GI_HD bool tri_hit(const Tri& g, const Ray& ray, double& u, double& v, double& t)
{
    V3 edge1 = ld3(g.e1), edge2 = ld3(g.e2);
    V3 p = cross(ray.d, edge2);
    double det = dot(edge1, p);
    if (det < GI_EPSILON && det > -GI_EPSILON) return false;
    double inv_det = 1.0 / det;
    V3 tvec = ray.o - ld3(g.p0);
    u = dot(tvec, p) * inv_det;
    if (u < 0 || u > 1) return false;
    V3 q = cross(tvec, edge1);
    v = dot(ray.d, q) * inv_det;
    if (v < 0 || u + v > 1) return false;
    t = dot(edge2, q) * inv_det;
    if (t <= 0) return false;
    return true;
}

struct HitRec { V3 pos; double u, v; int32_t tri; uint32_t mf; double tu, tv; };   // mf = LeafTri::matflags of the hit (material << 3 | flags)   // u, v barycentric; tu, tv = the reference's `uv` (GI_FEAT_TEX only)

// Wave-uniform leaves.  When every active lane of a wave stands on the SAME leaf (primary rays of one 8x8 tile, shadow rays towards one
// light) the leaf's records are fetched once per wave through the scalar cache (s_load into SGPRs -- a load from the constant address
// space at a wave-uniform address) instead of once per lane through the vector memory path: the 64 identical copies of an 80-byte
// record were what kept the L1 -> VGPR path as busy as the VALU.  The tests then read the record as SGPR operands; same arithmetic,
// same order, same bits.  Device code only (the CPU build of these functions has no waves).
#if defined(__HIP_DEVICE_COMPILE__)
#define GI_WAVE_UNIFORM_LEAVES 1
GI_HD bool leaf_is_wave_uniform(int32_t first, int32_t cnt, int32_t& first_u, int32_t& cnt_u)
{
    first_u = __builtin_amdgcn_readfirstlane(first);
    cnt_u = __builtin_amdgcn_readfirstlane(cnt);
    return __ballot(first != first_u || cnt != cnt_u) == 0ull;
}
GI_HD LeafTri leaf_tri_scalar(const LeafTri* rec)   // rec is wave-uniform
{
    typedef const __attribute__((address_space(4))) double* KD;
    typedef const __attribute__((address_space(4))) int32_t* KI;
    const KD d = (KD)(reinterpret_cast<const double*>(rec));
    const KI w = (KI)(reinterpret_cast<const int32_t*>(rec));
    LeafTri g;
    g.p0[0] = d[0]; g.p0[1] = d[1]; g.p0[2] = d[2];
    g.e1[0] = d[3]; g.e1[1] = d[4]; g.e1[2] = d[5];
    g.e2[0] = d[6]; g.e2[1] = d[7]; g.e2[2] = d[8];
    g.tri = w[18]; g.matflags = (uint32_t)w[19];
    return g;
}
struct Box6 { double b[6]; };
GI_HD Box6 leaf_box_scalar(const double* rec)   // rec is wave-uniform: the entity's box through the scalar cache
{
    typedef const __attribute__((address_space(4))) double* KD;
    const KD d = (KD)rec;
    Box6 r;
    for (int k = 0; k < 6; k++) r.b[k] = d[k];
    return r;
}
#endif

// ------------------------------------------------------------------------------------------------ textures (include/material.h:10-81)
GI_HD const unsigned char* tex_pixel(const Scene& S, const TexD& x, double tu, double tv)   // image.pixelColor(...), include/material.h:65
{
    const int px = abs((int)(tu * x.w * x.tile_u) % x.w);
    const int py = x.h - abs((int)(tv * x.h * x.tile_v) % x.h) - 1;
    return S.tex_pixels + x.pix + ((size_t)py * x.w + px) * 4;
}
GI_HD V3 tex_get(const Scene& S, int32_t t, V3 constant, double tu, double tv)   // texture::get
{
    if (t < 0) return constant;
    const TexD& x = S.texs[t];
    if (x.kind == 0) return ld3(x.a);
    if (x.kind == 1) {
        const int tiles = (int)x.tiles;
        if (((int)(tu * tiles) % 2 == 0) ^ ((int)(tv * tiles) % 2 == 0)) return ld3(x.a);
        return ld3(x.b);
    }
    const unsigned char* px = tex_pixel(S, x, tu, tv);
    return v3(S.tex_lut[px[0]], S.tex_lut[px[1]], S.tex_lut[px[2]]);
}
GI_HD double tex_alpha(const Scene& S, int32_t t, double tu, double tv)   // texture::getAlpha
{
    if (t < 0) return 1;
    const TexD& x = S.texs[t];
    if (x.kind != 2 || !x.has_alpha) return 1;
    return tex_pixel(S, x, tu, tv)[3] / 255.0;
}
// the reference's `uv` after a successful Entity::intersect: interpolated texCoords of a smooth triangle (include/entities.h:480-482),
// asin / atan2 of a sphere (include/entities.h:93-96); a flat-shaded triangle leaves the caller's variable as it was
template <class Tri>
GI_HD void ent_uv(const Scene& S, const Tri& g, uint32_t flags, int32_t ti, double u, double v, V3 hp, double& tu, double& tv)
{
    if (flags & 4u) {
        const V3 d = (ld3(g.p0) - hp) / g.e1[0];
        tv = .5 + asin(d.y) / GI_PI;
        tu = .5 + atan2(d.z, d.x) / (2 * GI_PI);
    } else if (flags & 1u) {
        const TriUV& sh = S.tri_uv[ti];
        const double w = (1 - u - v);
        tu = w * sh.t0[0] + u * sh.t1[0] + v * sh.t2[0];
        tv = w * sh.t0[1] + u * sh.t1[1] + v * sh.t2[1];
    }
}
// Material::getAlpha = opacity * diffuse->getAlpha(uv), include/material.h:90-93
GI_HD double mat_alpha(const Scene& S, const Mat& m, double tu, double tv) { return m.opacity * tex_alpha(S, m.dtex, tu, tv); }

// Entity::intersect for the two kinds on this path: triangle (include/entities.h:443-490, barycentric u, v) and analytic sphere
// (include/entities.h:60-101).  hp = hit point.
template <int FEAT, class Tri>
GI_HD bool ent_hit(const Tri& g, uint32_t flags, const Ray& ray, double& u, double& v, V3& hp)
{
    if (!(FEAT & GI_FEAT_SPHERES) || !(flags & 4u)) {   // no sphere bit: the scene holds triangles only (checked at upload)
        double t;
        if (!tri_hit(g, ray, u, v, t)) return false;
        hp = ray.o + t * ray.d;
        return true;
    }
    const V3 pos = ld3(g.p0);
    const double rad = g.e1[0];
    const V3 oc = ray.o - pos;
    const double dt = dot(ray.d, oc);
    const double r = (dt * dt - len2(oc) + rad * rad);
    if (r < 0) return false;
    const double sr = sqrt(r);
    const double t_1 = -1 * dt - sr, t_2 = -1 * dt + sr;
    if (t_1 < 0 && t_2 < 0) return false;
    if ((t_1 < t_2 && t_1 > 0) || t_2 < 0) hp = ray.o + ray.d * t_1;
    else hp = ray.o + ray.d * t_2;
    u = 0; v = 0;   // the reference derives texture coordinates here (asin / atan2); constant textures never read them
    return true;
}
// Does the ray hit this leaf reference, and does the hit count?  Entity::intersect, then the alpha test of RayTracer::trace / visible
// (include/raytracer.h:290-305,446-472) for an entity whose material has one (flag 2 clear): the hit counts when a number drawn per
// (purpose, leaf, entity) falls below the material's alpha, or the material refracts.  The draw is per (leaf, entity): an entity that failed
// from one leaf is drawn again from every later leaf that refers to it -- what the closest-hit short cuts have to respect (trace_wide_over).
// leaf_id: where the leaf's canonical id stands (read only when a number is drawn).  uv, under GI_FEAT_TEX, is the walk's texture-coordinate policy:
//  * closest-hit walk: the pair the walk carries across entities -- the reference's `uv` variable of trace(), written by every successful
//    intersect of a smooth triangle or sphere and left as it was by a flat one (ent_uv), so the alpha look-up of a flat entity reads what the
//    entity before it left behind;
//  * any-hit walk: null -- a fresh (0, 0) pair, computed only when an alpha test needs it.
// Called by the one-ray-per-group walks (trace_wide_coop, visible_wide_coop).  The per-lane walks (trace_wide_step, visible_leaf_blocks, trace_nodes,
// visible_nodes) still spell the same rule out themselves: moving them here cost four kernels scratch, so they wait for a form that does not.
template <int FEAT, class Tri>
GI_HD bool ent_accepts(const Scene& S, const Tri& g, const Ray& ray, const Rng& rng, uint32_t purpose, const int32_t* leaf_id, double* uv, double& u, double& v, V3& hp)
{
    if (!ent_hit<FEAT>(g, g.matflags, ray, u, v, hp)) return false;
    if ((FEAT & GI_FEAT_TEX) && uv) ent_uv(S, g, g.matflags, g.tri, u, v, hp, uv[0], uv[1]);
    if (!(g.matflags & 2u)) {
        const Mat& m = S.mats[g.matflags >> 3];
        double alpha = m.opacity * 1.0;
        if (FEAT & GI_FEAT_TEX) {
            double fresh[2] = {0, 0};
            double* const c = uv ? uv : fresh;
            if (!uv) ent_uv(S, g, g.matflags, g.tri, u, v, hp, c[0], c[1]);
            alpha = mat_alpha(S, m, c[0], c[1]);
        }
        if (!(rng_draw(rng, purpose, (uint32_t)*leaf_id, (uint32_t)g.tri) < alpha || m.ior != 1)) return false;
    }
    return true;
}
// the any-hit walk's question (RayTracer::visible): an accepted hit strictly between the origin and the light, 0 < |hit - o|^2 < mt
template <int FEAT, class Tri>
GI_HD bool ent_blocks(const Scene& S, const Tri& g, const Ray& ray, double mt, const Rng& rng, uint32_t light_index, const int32_t* leaf_id)
{
    double u, v;
    V3 hp;
    if (!ent_accepts<FEAT>(S, g, ray, rng, P_SHADOW_ALPHA | (light_index << 8), leaf_id, nullptr, u, v, hp)) return false;
    const double ts = len2(hp - ray.o);
    return (ts < mt) && (ts > 0);
}
