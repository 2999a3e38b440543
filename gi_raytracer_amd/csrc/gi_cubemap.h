// gi_cubemap.h -- the per-lane functions of a reflection probe (gi_cubemap_*; include/gi_hip.h states the definition): a cube texel's direction, its
// measure, the lobe weight of the prefilter and the box mean.  Needs gi_math.h (V3, Ray, halton_sample).  Included by gi_cubemap.inc inside namespace
// gi; tests/cpp/cubemap_kat.cpp compiles it for the host.  IEEE + - * / and sqrt only, in the header's order, so that with -ffp-contract=off every
// value equals the tests' numpy statement (tests/cubemap_expect.py) bit for bit.

// the face coordinate of texel column (or row) i of n under the jitter j: -1 at the face's left (top) edge, +1 at its right (bottom) edge
GI_HD double cm_coord(uint32_t i, double j, uint32_t n) { return (2.0 * ((double)i + j)) / (double)n - 1.0; }
// the unnormalised direction of (a, b) on face f: +X, -X, +Y, -Y, +Z, -Z; row b grows downward
GI_HD V3 cm_face_dir(uint32_t f, double a, double b)
{
    switch (f) {
    case 0: return v3(1.0, -b, -a);
    case 1: return v3(-1.0, -b, a);
    case 2: return v3(a, 1.0, b);
    case 3: return v3(a, -1.0, -b);
    case 4: return v3(a, -b, 1.0);
    default: return v3(-a, -b, -1.0);
    }
}
// texel t = (f n + y) n + x of a cube of face n
struct CmTexel { uint32_t f, y, x; };
GI_HD CmTexel cm_texel(uint32_t t, uint32_t n)
{
    CmTexel q;
    q.x = t % n; q.y = (t / n) % n; q.f = t / (n * n);
    return q;
}
GI_HD V3 cm_unit(V3 u) { return u * (1.0 / sqrt((u.x * u.x + u.y * u.y) + u.z * u.z)); }
// the unit direction of the centre of texel t
GI_HD V3 cm_centre_dir(uint32_t t, uint32_t n)
{
    const CmTexel q = cm_texel(t, n);
    return cm_unit(cm_face_dir(q.f, cm_coord(q.x, 0.5, n), cm_coord(q.y, 0.5, n)));
}
// the measure of the texel whose centre is (a, b): the solid angle of a face element over its area, up to the factor common to a level
GI_HD double cm_measure(double a, double b)
{
    const double r = (1.0 + a * a) + b * b;
    return 1.0 / (r * sqrt(r));
}
// the weight of a source texel (unit centre direction d, measure m) for the output direction R: the clamped cosine squared log2_e times, times m
GI_HD double cm_weight(V3 R, V3 d, double m, int log2_e)
{
    const double c = (R.x * d.x + R.y * d.y) + R.z * d.z;
    double w = c > 0.0 ? c : 0.0;
    for (int k = 0; k < log2_e; k++) w = w * w;
    return w * m;
}
// a box level's texel from the 2 x 2 block below it, row-major
GI_HD double cm_box(double p00, double p01, double p10, double p11) { return ((p00 + p01) + (p10 + p11)) * 0.25; }
// a capture's ray: sample `stream` of texel t of a cube of face n around P.  The jitter is Halton dimensions 0 and 1 at the stream index, the two a
// bake's ray takes for its direction; the ray leaves P itself
GI_HD Ray cm_ray(const Scene& S, V3 P, uint32_t n, uint32_t t, uint32_t stream)
{
    const double ju = (double)halton_sample(S, 0, stream);
    const double jv = (double)halton_sample(S, 1, stream);
    const CmTexel q = cm_texel(t, n);
    return make_ray(P, cm_face_dir(q.f, cm_coord(q.x, ju, n), cm_coord(q.y, jv, n)));
}
