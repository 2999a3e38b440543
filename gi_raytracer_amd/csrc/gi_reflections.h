// gi_reflections.h -- the per-lane functions of a reflection probe set (gi_render_baked_reflections_*; include/gi_hip.h states the definition): a
// probe's containment test, the distance to its box's nearest face, the blend weight, the exit distance of the reflection ray from the box, the
// box-projected direction, and step 5 of the baked-light pass with the probes that contain the hit blended.  Needs gi_math.h (V3) and, in front of
// it, gi_baked.h (cube_texel).  Included by gi_baked.inc inside namespace gi; tests/cpp/reflections_lookup.cpp compiles it for the host.  IEEE
// + - * / and comparisons only, in the header's order, so that with -ffp-contract=off every value equals the tests' numpy statement
// (tests/reflections_expect.py) bit for bit.
//
// No table content takes a read out of bounds.  The probe table is indexed by k < K alone.  A chain is indexed by k < K, the level's offset and
// cube_texel(D, n), and cube_texel clamps both face coordinates to 0 .. n - 1 and sends a NaN to texel 0 whatever D is -- zero, infinite or NaN
// (the face index is one of six by construction).  rs_direction hands it a finite D that is not 0 0 0, or else R as it came, which cube_texel
// takes the same way; rs_nearest's index starts at 0 and only moves to a k < K.  tests/cpp/reflections_lookup.cpp reads tables of exactly K rows
// and K chains under the address sanitizer, with NaN and infinities in P, R and the table.

#ifndef GI_REFLECTIONS_MAX_PROBES
#define GI_REFLECTIONS_MAX_PROBES 64        // (include/gi_hip.h's, for the host program that compiles this file without it)
#endif
#define GI_RS_ROW 10        // doubles per probe: pos[3], box_min[3], box_max[3], fade

// box_min <= P <= box_max on all three axes; a NaN on either side fails
GI_HD bool rs_contains(const double* pr, V3 P)
{
    return pr[3] <= P.x && P.x <= pr[6] && pr[4] <= P.y && P.y <= pr[7] && pr[5] <= P.z && P.z <= pr[8];
}
// the least of the six distances from P to the box's faces: x-low, x-high, y-low, y-high, z-low, z-high, a later one taken where it is smaller
GI_HD double rs_edge(const double* pr, V3 P)
{
    double e = P.x - pr[3], v;
    v = pr[6] - P.x; if (v < e) e = v;
    v = P.y - pr[4]; if (v < e) e = v;
    v = pr[7] - P.y; if (v < e) e = v;
    v = P.z - pr[5]; if (v < e) e = v;
    v = pr[8] - P.z; if (v < e) e = v;
    return e;
}
// the blend weight of a probe that contains P: edge / fade up to 1 inside the fade band, 1 beyond it and with no band at all
GI_HD double rs_weight(double edge, double fade) { return fade > 0.0 ? (edge / fade < 1.0 ? edge / fade : 1.0) : 1.0; }
// the distance along R at which the ray from P leaves the box: per axis with R_a != 0 the face R points at, the first such axis's value, then a
// later one where it is smaller (a NaN first stays, a NaN later is never smaller); 0 when R is 0 0 0
GI_HD double rs_exit(const double* pr, V3 P, V3 R)
{
    double t = 0.0;
    bool have = false;
    if (R.x != 0.0) { t = ((R.x > 0.0 ? pr[6] : pr[3]) - P.x) / R.x; have = true; }
    if (R.y != 0.0) { const double v = ((R.y > 0.0 ? pr[7] : pr[4]) - P.y) / R.y; if (!have || v < t) t = v; have = true; }
    if (R.z != 0.0) { const double v = ((R.z > 0.0 ? pr[8] : pr[5]) - P.z) / R.z; if (!have || v < t) t = v; }
    return t;
}
GI_HD bool rs_finite(double x) { return x - x == 0.0; }      // an infinity and a NaN give NaN here
// the direction the probe's cube is read in: from its position to the point where the reflection ray leaves its box; R itself where that
// direction has a component that is not finite, or is 0 0 0
GI_HD V3 rs_direction(const double* pr, V3 P, V3 R)
{
    const double t = rs_exit(pr, P, R);
    const V3 Q = v3(P.x + t * R.x, P.y + t * R.y, P.z + t * R.z);
    const V3 D = v3(Q.x - pr[0], Q.y - pr[1], Q.z - pr[2]);
    if (!(rs_finite(D.x) && rs_finite(D.y) && rs_finite(D.z)) || (D.x == 0.0 && D.y == 0.0 && D.z == 0.0)) return R;
    return D;
}
// the probe nearest to P by ((dx dx + dy dy) + dz dz): the first of equals, a NaN never nearer, probe 0 when none is nearer than infinity
GI_HD int32_t rs_nearest(const double* probes, int32_t K, V3 P)
{
    int32_t best = 0;
    double bd = INFINITY;
    for (int32_t k = 0; k < K; k++) {
        const double* pr = probes + (size_t)k * GI_RS_ROW;
        const double dx = P.x - pr[0], dy = P.y - pr[1], dz = P.z - pr[2];
        const double d = (dx * dx + dy * dy) + dz * dz;
        if (d < bd) { bd = d; best = k; }
    }
    return best;
}
// S at the hit P for the reflection direction R from the set probes [K][10] and its chains [K][texels][3], read at the level of face n whose
// texels start `off` texels into a chain: the probes that contain P in ascending k, each read at its box-projected direction and weighted by
// its distance to the box's faces; with no weight at all, the nearest probe read at R
GI_HD V3 rs_specular(const double* probes, const double* chains, int32_t K, size_t texels, uint32_t off, uint32_t n, V3 P, V3 R)
{
    double acc[3] = {0.0, 0.0, 0.0}, W = 0.0;
    for (int32_t k = 0; k < K; k++) {
        const double* pr = probes + (size_t)k * GI_RS_ROW;
        if (!rs_contains(pr, P)) continue;
        const double w = rs_weight(rs_edge(pr, P), pr[9]);
        const double* v = chains + ((size_t)k * texels + (size_t)off + cube_texel(rs_direction(pr, P, R), n)) * 3;
        acc[0] += w * v[0]; acc[1] += w * v[1]; acc[2] += w * v[2];
        W += w;
    }
    if (W > 0.0) return v3(acc[0] / W, acc[1] / W, acc[2] / W);
    const double* v = chains + ((size_t)rs_nearest(probes, K, P) * texels + (size_t)off + cube_texel(R, n)) * 3;
    return v3(v[0], v[1], v[2]);
}
