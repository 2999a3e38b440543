// gi_visibility.h -- the per-lane functions of probe visibility (gi_probe_visibility_*, gi_render_baked_visibility_*; include/gi_hip.h states the
// definition): the octahedral map's decode and encode, a capture's ray, the two sums of a texel, the bilinear value of a map, and step 4 of the
// baked-light pass with the eight probes weighted by a back-face term and a Chebyshev test.  Needs gi_math.h (V3, Ray, halton_sample) and, in front
// of it, gi_baked.h (grid_cell, sh9_factor, sh9_probe).  Included by gi_baked.inc inside namespace gi; tests/cpp/visibility_lookup.cpp compiles it
// for the host.  IEEE + - * / and sqrt only (and the sign operations fabs and negation), in the header's order, so that with -ffp-contract=off every
// value equals the tests' numpy statement (tests/visibility_expect.py) bit for bit.

#define GI_PV_MAX_SIZE 64

// sgn of the octahedral fold: +1 for q >= 0 (and for -0.0), else -1 (a NaN: -1)
GI_HD double octa_sgn(double q) { return q >= 0.0 ? 1.0 : -1.0; }
// (a, b) in [0, 1]^2 to the unnormalised direction of the octahedral map: the upper half (vz >= 0) is the square's inner diamond, the lower half
// its four corners folded over the diamond's edges
GI_HD V3 octa_decode(double a, double b)
{
    const double px = 2.0 * a - 1.0, py = 2.0 * b - 1.0;
    const double vz = (1.0 - fabs(px)) - fabs(py);
    if (vz < 0.0) return v3((1.0 - fabs(py)) * octa_sgn(px), (1.0 - fabs(px)) * octa_sgn(py), vz);
    return v3(px, py, vz);
}
// a vector that is not 0 0 0, of any length, to its (a, b)
struct OctaUV { double a, b; };
GI_HD OctaUV octa_encode(V3 v)
{
    const double s = (fabs(v.x) + fabs(v.y)) + fabs(v.z);
    double px = v.x / s, py = v.y / s;
    if (v.z < 0.0) {
        const double fx = (1.0 - fabs(py)) * octa_sgn(px), fy = (1.0 - fabs(px)) * octa_sgn(py);
        px = fx; py = fy;
    }
    OctaUV c;
    c.a = (px + 1.0) * 0.5; c.b = (py + 1.0) * 0.5;
    return c;
}
// a capture's ray: sample `stream` of texel (x, y) of a map of M x M around P.  The jitter is Halton dimensions 0 and 1 at the stream index, as in a
// reflection probe's capture (cm_ray); the ray leaves P itself
GI_HD Ray pv_ray(const Scene& S, V3 P, uint32_t M, uint32_t x, uint32_t y, uint32_t stream)
{
    const double ju = (double)halton_sample(S, 0, stream);
    const double jv = (double)halton_sample(S, 1, stream);
    return make_ray(P, octa_decode(((double)x + ju) / (double)M, ((double)y + jv) / (double)M));
}
// the distance a sample adds: that of the hit H from P, max_dist for a miss, never more than max_dist
GI_HD double pv_hit_distance(V3 H, V3 P)
{
    const double dx = H.x - P.x, dy = H.y - P.y, dz = H.z - P.z;
    return sqrt((dx * dx + dy * dy) + dz * dz);
}
GI_HD double pv_clamp(double r, double max_dist) { return r < max_dist ? r : max_dist; }
// a texel's two sums, in ascending k from +0.0, and the pair (m, m2) they leave
struct PvSums { double s1, s2; };
GI_HD void pv_add(PvSums& a, double r) { a.s1 += r; a.s2 += r * r; }
struct PvMoments { double m, m2; };
GI_HD PvMoments pv_moments(const PvSums& a, double n)
{
    PvMoments q;
    q.m = a.s1 / n; q.m2 = a.s2 / n;
    return q;
}
// the bilinear value of one map [M][M][2] at (a, b): lm_bilinear's rule on two channels -- texel centres at (x + 0.5) / M, clamped at the map's
// border (grid_cell: a NaN goes to texel 0), along x on both rows, then along y.  No octahedral wrap: see DESIGN.md.  The values are the caller's
GI_HD PvMoments pv_bilinear(const double* map, int32_t M, OctaUV c)
{
    const GridCell cx = grid_cell(c.a, 0.0, 1.0, M), cy = grid_cell(c.b, 0.0, 1.0, M);
    const double* r0 = map + (size_t)cy.i0 * (size_t)M * 2;
    const double* r1 = map + (size_t)cy.i1 * (size_t)M * 2;
    const double* p00 = r0 + (size_t)cx.i0 * 2; const double* p01 = r0 + (size_t)cx.i1 * 2;
    const double* p10 = r1 + (size_t)cx.i0 * 2; const double* p11 = r1 + (size_t)cx.i1 * 2;
    PvMoments q;
    const double m_lo = p00[0] + cx.t * (p01[0] - p00[0]), m_hi = p10[0] + cx.t * (p11[0] - p10[0]);
    const double s_lo = p00[1] + cx.t * (p01[1] - p00[1]), s_hi = p10[1] + cx.t * (p11[1] - p10[1]);
    q.m = m_lo + cy.t * (m_hi - m_lo);
    q.m2 = s_lo + cy.t * (s_hi - s_lo);
    return q;
}
// the Chebyshev weight of a point at distance r > 0 from a probe whose map says (m, m2) in its direction: 1 in front of the mean distance, behind it
// the one-sided bound var / (var + (r - m)^2) cubed, never below vis_floor
GI_HD double pv_chebyshev(double r, PvMoments q, double vis_floor)
{
    if (!(r > q.m)) return 1.0;
    const double var = fabs(q.m * q.m - q.m2), dd = r - q.m;
    double ch = var / (var + dd * dd);
    ch = (ch * ch) * ch;
    return ch > vis_floor ? ch : vis_floor;
}
// the weight of one probe at Q for the hit P under the unit normal nf, beside its trilinear weight: the back-face term ((cos + 1) / 2)^2 + 0.2, and
// the visibility of P + nf * normal_bias in the probe's map
GI_HD double pv_backface(V3 P, V3 nf, V3 Q)
{
    const double ex = Q.x - P.x, ey = Q.y - P.y, ez = Q.z - P.z;
    const double le = sqrt((ex * ex + ey * ey) + ez * ez);
    const double cb = le > 0.0 ? ((ex * nf.x + ey * nf.y) + ez * nf.z) / le : 1.0;
    const double h = (cb + 1.0) * 0.5;
    return h * h + 0.2;
}
GI_HD double pv_visibility(const double* map, int32_t M, V3 P, V3 nf, V3 Q, double normal_bias, double vis_floor)
{
    const V3 v = v3((P.x + nf.x * normal_bias) - Q.x, (P.y + nf.y * normal_bias) - Q.y, (P.z + nf.z * normal_bias) - Q.z);
    const double r = sqrt((v.x * v.x + v.y * v.y) + v.z * v.z);
    if (r == 0.0) return 1.0;
    return pv_chebyshev(r, pv_bilinear(map, M, octa_encode(v)), vis_floor);
}
// D at the point P under the normal nf from the grid sh [nz][ny][nx][9][3] and its maps vis [nz][ny][nx][M][M][2]: the eight probes around P in
// ascending corner c = cx + 2 cy + 4 cz, each weighted by (trilinear, at least 0.001) * back-face * visibility; num / den per channel, clamped at 0
// from below.  den > 0: every factor is
GI_HD V3 pv_irradiance(const double* sh, const double* vis, int32_t M, const int32_t* n3, const double* gmin, const double* gmax, V3 P, V3 nf, double normal_bias, double vis_floor)
{
    double F[9];
    sh9_factor(nf, F);
    const GridCell cell[3] = {grid_cell(P.x, gmin[0], gmax[0], n3[0]), grid_cell(P.y, gmin[1], gmax[1], n3[1]), grid_cell(P.z, gmin[2], gmax[2], n3[2])};
    double num[3] = {0.0, 0.0, 0.0}, den = 0.0;
    for (int c = 0; c < 8; c++) {
        int32_t j[3];
        double w[3], Q[3];
        GI_UNROLL
        for (int a = 0; a < 3; a++) {
            const bool up = ((c >> a) & 1) != 0;
            j[a] = up ? cell[a].i1 : cell[a].i0;
            w[a] = up ? cell[a].t : 1.0 - cell[a].t;
            Q[a] = gmin[a] + (((double)j[a] + 0.5) / (double)n3[a]) * (gmax[a] - gmin[a]);
        }
        const size_t q = ((size_t)j[2] * (size_t)n3[1] + (size_t)j[1]) * (size_t)n3[0] + (size_t)j[0];
        double tw = (w[0] * w[1]) * w[2];
        tw = tw > 0.001 ? tw : 0.001;
        const V3 Qv = v3(Q[0], Q[1], Q[2]);
        const double wb = pv_backface(P, nf, Qv);
        const double vs = pv_visibility(vis + q * (size_t)M * (size_t)M * 2, M, P, nf, Qv, normal_bias, vis_floor);
        const double wc = (tw * wb) * vs;
        const V3 D = sh9_probe(sh + q * 27, F);
        num[0] += wc * D.x; num[1] += wc * D.y; num[2] += wc * D.z;
        den += wc;
    }
    const double dx = num[0] / den, dy = num[1] / den, dz = num[2] / den;
    return v3(dx < 0.0 ? 0.0 : dx, dy < 0.0 ? 0.0 : dy, dz < 0.0 ? 0.0 : dz);
}
