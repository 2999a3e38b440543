// gi_baked.h -- the per-lane functions of the baked-light pass (gi_render_baked_*; include/gi_hip.h states the definition): the probe grid's cell, the
// irradiance factors of an SH9 probe, the trilinear step, the texel of a direction in a reflection probe's cube, the chart coordinate of a hit and the
// two filters of a lightmap atlas (tests/cpp/baked_lightmap_lookup.cpp, tests/baked_lightmap_expect.py), the direct-light loop, and -- host
// only -- the level a material's roughness reads from.  Needs gi_device.h (visible_nodes, the RNG, LightD) and gi_cubemap.h (the texel order).
// Included by gi_baked.inc inside namespace gi; tests/cpp/baked_lookup.cpp compiles it for the host.  Apart from the light loop, which is the shade
// stage's arithmetic, everything is IEEE + - * / and sqrt only, in the header's order, so that with -ffp-contract=off every value equals the
// tests' numpy statement (tests/baked_expect.py) bit for bit.

// the cell of one axis of a grid of n probes between gmin and gmax, probes at the cell centres (probe_grid): the two probes around p and the weight of the upper one
struct GridCell { int32_t i0, i1; double t; };
GI_HD GridCell grid_cell(double p, double gmin, double gmax, int32_t n)
{
    double g = ((p - gmin) / (gmax - gmin)) * (double)n - 0.5;
    const double top = (double)(n - 1);
    g = g > 0.0 ? (g < top ? g : top) : 0.0;      // clamped to [0, n - 1]; a NaN goes to 0
    GridCell c;
    c.i0 = (int32_t)g;                              // floor: g >= 0
    c.i1 = c.i0 + 1 < n ? c.i0 + 1 : n - 1;
    c.t = g - (double)c.i0;
    return c;
}
// F_j = k_j * Y_j(n): the real SH basis of bands 0 to 2 at the unit normal n (the order and literals of GI_BAKE_SH9) times the band's cosine-lobe
// factor over pi (1, 2/3, 1/4), so that sum_j F_j c_j is on the scale of a GI_BAKE_TEXEL result
GI_HD void sh9_factor(V3 n, double* F)
{
    const double x = n.x, y = n.y, z = n.z;
    F[0] = 1.0 * 0.28209479177387814;
    F[1] = 0.6666666666666666 * (0.4886025119029199 * y);
    F[2] = 0.6666666666666666 * (0.4886025119029199 * z);
    F[3] = 0.6666666666666666 * (0.4886025119029199 * x);
    F[4] = 0.25 * (1.0925484305920792 * (x * y));
    F[5] = 0.25 * (1.0925484305920792 * (y * z));
    F[6] = 0.25 * (0.31539156525252005 * (3.0 * (z * z) - 1.0));
    F[7] = 0.25 * (1.0925484305920792 * (x * z));
    F[8] = 0.25 * (0.5462742152960396 * (x * x - y * y));
}
// one probe [9][3] under the factors: D[ch] = the sum over j, ascending from +0.0, of F_j * c_j[ch]
GI_HD V3 sh9_probe(const double* c, const double* F)
{
    double d[3] = {0.0, 0.0, 0.0};
    GI_UNROLL
    for (int j = 0; j < 9; j++) {
        GI_UNROLL
        for (int ch = 0; ch < 3; ch++) d[ch] += F[j] * c[j * 3 + ch];
    }
    return v3(d[0], d[1], d[2]);
}
// the trilinear step
GI_HD V3 lerp3(V3 a, V3 b, double t) { return a + t * (b - a); }
// D at the point P under the normal nf from the grid sh [nz][ny][nx][9][3]: the eight probes around P evaluated first, then interpolated along x,
// then y, then z, then each channel clamped at 0 from below
GI_HD V3 grid_irradiance(const double* sh, const int32_t* n3, const double* gmin, const double* gmax, V3 P, V3 nf)
{
    double F[9];
    sh9_factor(nf, F);
    const GridCell cx = grid_cell(P.x, gmin[0], gmax[0], n3[0]), cy = grid_cell(P.y, gmin[1], gmax[1], n3[1]), cz = grid_cell(P.z, gmin[2], gmax[2], n3[2]);
    const auto line = [&](int32_t iz, int32_t iy) {     // the two probes of a grid line along x, interpolated
        const size_t row = ((size_t)iz * (size_t)n3[1] + (size_t)iy) * (size_t)n3[0];
        return lerp3(sh9_probe(sh + (row + (size_t)cx.i0) * 27, F), sh9_probe(sh + (row + (size_t)cx.i1) * 27, F), cx.t);
    };
    const V3 lo = lerp3(line(cz.i0, cy.i0), line(cz.i0, cy.i1), cy.t);
    const V3 hi = lerp3(line(cz.i1, cy.i0), line(cz.i1, cy.i1), cy.t);
    const V3 d = lerp3(lo, hi, cz.t);
    return v3(d.x < 0.0 ? 0.0 : d.x, d.y < 0.0 ? 0.0 : d.y, d.z < 0.0 ? 0.0 : d.z);
}
// a face coordinate in [-1, 1] to its texel column (or row) of n: min(n - 1, max(0, floor(((a + 1.0) * 0.5) * n))); a NaN goes to 0
GI_HD uint32_t cube_coord_texel(double a, uint32_t n)
{
    const double v = ((a + 1.0) * 0.5) * (double)n;
    return v >= 1.0 ? (v < (double)n ? (uint32_t)v : n - 1u) : 0u;
}
// the texel t = (f n + y) n + x (cm_texel's order) of a cube of face n that the direction R, of any length but 0, falls into: the face of the
// largest |component|, the first of equals; (a, b) = the other two components, as cm_face_dir lays them out, over that component's size
GI_HD uint32_t cube_texel(V3 R, uint32_t n)
{
    const double ax = R.x < 0.0 ? -R.x : R.x, ay = R.y < 0.0 ? -R.y : R.y, az = R.z < 0.0 ? -R.z : R.z;
    int axis = 0;
    double size = ax;
    if (ay > size) { axis = 1; size = ay; }
    if (az > size) { axis = 2; size = az; }
    const double x = R.x / size, y = R.y / size, z = R.z / size;
    uint32_t f;
    double a, b;
    if (axis == 0) { if (R.x < 0.0) { f = 1u; a = z; b = -y; } else { f = 0u; a = -z; b = -y; } }
    else if (axis == 1) { if (R.y < 0.0) { f = 3u; a = x; b = -z; } else { f = 2u; a = x; b = z; } }
    else { if (R.z < 0.0) { f = 5u; a = -x; b = -y; } else { f = 4u; a = x; b = -y; } }
    return (f * n + cube_coord_texel(b, n)) * n + cube_coord_texel(a, n);
}
// ---- the lightmap look-up (gi_render_baked_lightmap_*): from the hit point to the chart, from the chart to the atlas
// (u, v) of the point P of the entity g under the chart row uv [3][2]: the barycentrics of P in the entity's plane from the normal equations of
// P - p0 = b1 e1v + b2 e2v -- the inverse of lm_point (gi_lightmap.inc) -- then the row's three coordinates under them.  A function of the
// entity's record and P alone.  A degenerate triangle has den = 0: NaN (or infinite) coordinates, which both filters send to a border texel.
struct LmCoord { double u, v; };
GI_HD LmCoord lm_coord(const TriGeom& g, V3 P, const double* uv)
{
    const V3 e1 = ld3(g.e1), e2 = ld3(g.e2), d = P - ld3(g.p0);
    const double d00 = dot(e1, e1), d01 = dot(e1, e2), d11 = dot(e2, e2), d20 = dot(d, e1), d21 = dot(d, e2);
    const double den = d00 * d11 - d01 * d01;
    const double b1 = (d11 * d20 - d01 * d21) / den, b2 = (d00 * d21 - d01 * d20) / den;
    const double b0 = 1 - b1 - b2;
    LmCoord c;
    c.u = (b0 * uv[0] + b1 * uv[2]) + b2 * uv[4];
    c.v = (b0 * uv[1] + b1 * uv[3]) + b2 * uv[5];
    return c;
}
// GI_LM_NEAREST: the texel column (or row) of n that the coordinate falls into, min(n - 1, max(0, floor(a * n))); a NaN goes to 0
GI_HD int32_t lm_coord_texel(double a, int32_t n)
{
    const double v = a * (double)n;
    return v >= 1.0 ? (v < (double)n ? (int32_t)v : n - 1) : 0;
}
GI_HD V3 lm_nearest(const double* atlas, int32_t w, int32_t h, LmCoord c)
{
    return ld3(atlas + ((size_t)lm_coord_texel(c.v, h) * (size_t)w + (size_t)lm_coord_texel(c.u, w)) * 3);
}
// GI_LM_BILINEAR: the four texels around (u, v), texel centres at (x + .5) / w as the bake places them (lm_centre), clamped to the border texels
// (grid_cell: a NaN goes to texel 0); interpolated along x on both rows, then along y, then each channel clamped at 0 from below
GI_HD V3 lm_bilinear(const double* atlas, int32_t w, int32_t h, LmCoord c)
{
    const GridCell cx = grid_cell(c.u, 0.0, 1.0, w), cy = grid_cell(c.v, 0.0, 1.0, h);
    const auto row = [&](int32_t iy) {
        const double* r = atlas + (size_t)iy * (size_t)w * 3;
        return lerp3(ld3(r + (size_t)cx.i0 * 3), ld3(r + (size_t)cx.i1 * 3), cx.t);
    };
    const V3 d = lerp3(row(cy.i0), row(cy.i1), cy.t);
    return v3(d.x < 0.0 ? 0.0 : d.x, d.y < 0.0 ? 0.0 : d.y, d.z < 0.0 ? 0.0 : d.z);
}

// The analytic lights at a first hit: what the frame's depth-0 shade adds for them, as the streaming passes compute it (stage_shade_nodes with the
// walks put off, k_st_shadow): the share of the LAST light that is visible, asked from the last light down.  P the hit, norm the shading normal as
// the shade stage holds it (turned to the viewer's side, not renormalised), rng the stream's at depth 0.  VFEAT: the shade stage's level of the
// any-hit walk, the medium included.  Returns i; the term is color * i.
template <int VFEAT, class Nodes>
GI_HD V3 lit_direct(const Scene& S, const Nodes& N, V3 P, V3 norm, double roughness, const Rng& rng)
{
    for (int li = S.n_light - 1; li >= 0; li--) {
        const LightD& lt = S.lights[li];
        const double ry = rng_draw(rng, P_LIGHT_Y | ((uint32_t)li << 8));
        const double rx = rng_draw(rng, P_LIGHT_X | ((uint32_t)li << 8));
        const V3 lpos = ld3(lt.pos);
        const V3 so = P + GI_SHADOW_BIAS * norm;
        const V3 lightDir = (lpos + lt.rad * random_unit_vec(rx, ry)) - so;
        const double maxt = len2(lightDir);
        const Ray sray = make_ray(so, lightDir);
        if (!visible_nodes<VFEAT>(S, N, sray, maxt, rng, (uint32_t)li, nullptr)) continue;
        const double hfrac = 1 / (GI_PI * len2(lpos - P));
        double d = dot(norm, normalize(lpos - P));
        if (d < 0) d = 0;
        const double ex = (1.0 / roughness);   // pow(d, 1 / roughness) with the shade stage's exact short cuts
        const double l = ex == 1.0 ? d : (ex == INFINITY ? (d < 1.0 ? 0.0 : (d == 1.0 ? 1.0 : INFINITY)) : pow(d, ex));
        return ld3(lt.col) * l * hfrac;
    }
    return v3(0, 0, 0);
}

// host: the level of a chain of `levels` that a material of this roughness reads.  A mirror (roughness < .001) and a chain of one level read level 0;
// else the level l of 1 .. levels - 1 whose log2_exponent[l] is nearest to log2(1 / roughness + 1), the Phong exponent of the glossy bounce
// (secondary_ray); ties go to the lower l
inline int32_t baked_level_of(double roughness, int32_t levels, const int32_t* log2_exponent)
{
    if (levels <= 1 || roughness < .001 || !(roughness == roughness)) return 0;
    const double want = log2(1.0 / roughness + 1.0);
    int32_t best = 1;
    double best_d = fabs((double)log2_exponent[1] - want);
    for (int32_t l = 2; l < levels; l++) {
        const double d = fabs((double)log2_exponent[l] - want);
        if (d < best_d) { best = l; best_d = d; }
    }
    return best;
}
