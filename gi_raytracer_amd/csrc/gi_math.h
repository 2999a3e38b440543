// gi_math.h -- the arithmetic under everything: V3 in glm's operand order, Ray, the counter RNG and its purposes (DESIGN.md "RNG contract"),
// Halton and HaltonEnumD, the samplers.  Needs gi_scene.h (GI_HD, the constants, Scene's Halton tables) and <math.h>.  Included by gi_device.h
// inside namespace gi, behind gi_scene.h.
//
// Reference semantics followed (file:line relative to moepforfreedom/GI_Raytracer):
//   samplers         include/util.cpp:27-107, include/util.h:100-188
//   Halton           include/halton_enum.h:106-155, include/halton_sampler.h:626-888,1417-3286

// ------------------------------------------------------------------------------------------------ vec3 in glm operand order
struct V3 { double x, y, z; };
GI_HD V3 v3(double x, double y, double z) { V3 r; r.x = x; r.y = y; r.z = z; return r; }
GI_HD V3 ld3(const double* p) { return v3(p[0], p[1], p[2]); }
GI_HD V3 operator+(V3 a, V3 b) { return v3(a.x + b.x, a.y + b.y, a.z + b.z); }
GI_HD V3 operator-(V3 a, V3 b) { return v3(a.x - b.x, a.y - b.y, a.z - b.z); }
GI_HD V3 operator*(V3 a, V3 b) { return v3(a.x * b.x, a.y * b.y, a.z * b.z); }
GI_HD V3 operator*(V3 a, double s) { return v3(a.x * s, a.y * s, a.z * s); }
GI_HD V3 operator*(double s, V3 a) { return v3(s * a.x, s * a.y, s * a.z); }
GI_HD V3 operator/(V3 a, double s) { return v3(a.x / s, a.y / s, a.z / s); }
GI_HD double dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
GI_HD V3 cross(V3 x, V3 y) { return v3(x.y * y.z - y.y * x.z, x.z * y.x - y.z * x.x, x.x * y.y - y.x * x.y); }
GI_HD V3 normalize(V3 v) { return v * (1.0 / sqrt(dot(v, v))); }
GI_HD double length(V3 v) { return sqrt(dot(v, v)); }
GI_HD V3 reflect(V3 I, V3 N) { return I - N * dot(N, I) * 2.0; }
GI_HD V3 mix(V3 x, V3 y, double a) { return x + a * (y - x); }
GI_HD double len2(V3 v) { return v.x * v.x + v.y * v.y + v.z * v.z; }
GI_HD double comp_max(V3 v) { return fmax(fmax(v.x, v.y), v.z); }

struct Ray { V3 o, d, inv; };
GI_HD Ray make_ray(V3 o, V3 d)  // Ray ctor / setDir, include/ray.h:7-17
{
    Ray r;
    r.o = o;
    r.d = normalize(d);
    r.inv = v3(1.0 / r.d.x, 1.0 / r.d.y, 1.0 / r.d.z);
    return r;
}
GI_HD Ray make_ray_exact(V3 o, V3 d)
{
    Ray r;
    r.o = o; r.d = d;
    r.inv = v3(1.0 / d.x, 1.0 / d.y, 1.0 / d.z);
    return r;
}

// ------------------------------------------------------------------------------------------------ counter RNG (DESIGN.md "RNG contract")
GI_HD uint64_t mix64(uint64_t z)
{
    z ^= z >> 30; z *= 0xbf58476d1ce4e5b9ull;
    z ^= z >> 27; z *= 0x94d049bb133111ebull;
    z ^= z >> 31;
    return z;
}
enum {
    P_TRACE_ALPHA = 0, P_SHADOW_ALPHA = 1, P_LIGHT_X = 2, P_LIGHT_Y = 3, P_TYPE_OPACITY = 4, P_TYPE_FRESNEL = 5,
    P_RR = 6, P_FOG = 7, P_TRACE_GUARD = 8,
    P_PH_DIR_U = 16, P_PH_DIR_V = 17, P_PH_SEC_U = 18, P_PH_SEC_V = 19, P_PH_TRACE0_ALPHA = 20, P_PH_FOG_U = 21, P_PH_FOG_V = 22
};
enum { P_FOG_CAMERA = 0, P_FOG_SHADOW = 1, P_FOG_PHOTON = 2 };   // `b` key of P_FOG draws (shadow: + 16 * light index); `a` = step
#define GI_PHOTON_SEED_XOR 0x5048544f4e5eed00ull
struct Rng {
    uint64_t hs;      // hash of (seed, stream)
    uint32_t depth;
};
GI_HD Rng rng_make(uint64_t seed, uint32_t stream)
{
    Rng r;
    r.hs = mix64(seed + 0x9E3779B97F4A7C15ull * ((uint64_t)stream + 1));
    r.depth = 0;
    return r;
}
GI_HD double rng_draw(const Rng& r, uint32_t purpose, uint32_t a = 0, uint32_t b = 0)
{
    uint64_t h = mix64(r.hs ^ (((uint64_t)r.depth << 32) | purpose));
    h = mix64(h ^ (((uint64_t)a << 32) | b));
    return (double)(h >> 11) * (1.0 / 9007199254740992.0);
}

// ------------------------------------------------------------------------------------------------ Halton
GI_HD uint32_t rev_bits32(uint32_t index)
{
    index = (index << 16) | (index >> 16);
    index = ((index & 0x00ff00ffu) << 8) | ((index & 0xff00ff00u) >> 8);
    index = ((index & 0x0f0f0f0fu) << 4) | ((index & 0xf0f0f0f0u) >> 4);
    index = ((index & 0x33333333u) << 2) | ((index & 0xccccccccu) >> 2);
    index = ((index & 0x55555555u) << 1) | ((index & 0xaaaaaaaau) >> 1);
    return index;
}
// Halton_sampler::sample: base 2 by bit reversal into the mantissa, other bases by table digit groups (Horner form of the
// reference's sum_k table[(index / P^k) % P] * P^(n-1-k)), then one float multiply.
GI_HD float halton_sample(const Scene& S, uint32_t dim, uint32_t index)
{
    if (dim == 0) {
        union { uint32_t u; float f; } r;
        r.u = 0x3f800000u | (rev_bits32(index) >> 9);
        return r.f - 1.f;
    }
    const HaltonDim D = S.hdims[dim];
    // digit groups first (division by the table size as a multiplication: exact for every 32-bit index and P <= 1619), then all table
    // reads at once -- they do not depend on each other, and up to 7 dependent L2 round trips per sample were what this cost
    uint32_t dg[7], idx = index;
    GI_UNROLL
    for (int k = 0; k < 7; k++) {
        unsigned long long t = ((unsigned long long)idx * D.mlo) >> 32;
        t += (unsigned long long)idx * D.mhi;
        const uint32_t q = (uint32_t)(t >> 32);
        dg[k] = idx - q * D.P;
        idx = q;
    }
    uint32_t tv[7];
    GI_UNROLL
    for (int k = 0; k < 7; k++) tv[k] = (uint32_t)k < D.n ? (uint32_t)S.htable[D.off + dg[k]] : 0u;
    uint32_t sum = 0;
    GI_UNROLL
    for (int k = 0; k < 7; k++) if ((uint32_t)k < D.n) sum = sum * D.P + tv[k];
    return (float)sum * D.scale;
}
struct HaltonEnumD { uint32_t p2, p3, m_x, m_y, inc; float scale_x, scale_y; };
// Halton_enum::get_index, include/halton_enum.h:106-114,136-155
GI_HD uint32_t halton_index(const HaltonEnumD& e, uint32_t i, uint32_t x, uint32_t y)
{
    const unsigned long long hx = e.p2 ? (rev_bits32(x) >> (32 - e.p2)) : 0u;
    uint32_t r3 = 0, yy = y;
    for (uint32_t d = 0; d < e.p3; ++d) { r3 = r3 * 3 + yy % 3; yy /= 3; }
    const unsigned long long hy = r3;
    const uint32_t offset = (uint32_t)((hx * e.m_x + hy * e.m_y) % e.inc);
    return offset + i * e.inc;
}

// ------------------------------------------------------------------------------------------------ samplers (include/util.h, util.cpp)
GI_HD double fast_precise_pow(double a, double b)  // include/util.h:113-136: bit hack on the high word + exact integer power
{
    int e = (int)b;
    union { double d; int32_t x[2]; } u;
    u.d = a;
    u.x[1] = (int32_t)((b - e) * (u.x[1] - 1072632447) + 1072632447);
    u.x[0] = 0;
    double r = 1.0;
    while (e) {
        if (e & 1) r *= a;
        a *= a;
        e >>= 1;
    }
    return r * u.d;
}
GI_HD V3 frame_mul(V3 n, double z, V3 r)  // the explicit 3x3 of include/util.cpp:37-42 applied to r (glm column-major)
{
    double k = (1.0 / (1 + z));
    V3 c0 = v3(z + k * -n.y * -n.y, k * (n.x * -n.y), -n.x);
    V3 c1 = v3(k * (n.x * -n.y), z + k * -n.x * -n.x, -n.y);
    V3 c2 = v3(n.x, n.y, z);
    return v3(c0.x * r.x + c1.x * r.y + c2.x * r.z, c0.y * r.x + c1.y * r.y + c2.y * r.z, c0.z * r.x + c1.z * r.y + c2.z * r.z);
}
GI_HD V3 lobe_local(float u, float v, double power, double frac, bool cap)
{
    float phi = (float)(v * 2.0f * GI_PI);
    float cosTheta = cap ? (float)(frac * fast_precise_pow(1.0f - u, (1.0f / power)) + (1 - frac)) : (float)fast_precise_pow(1.0f - u, (1.0f / power));
    float sinTheta = (float)sqrt((double)(1.0f - cosTheta * cosTheta));
    return v3(cos((double)phi) * sinTheta, sin((double)phi) * sinTheta, cosTheta);
}
GI_HD V3 hemi_cos_n(V3 n, float u, float v, double power)  // include/util.cpp:35-58
{
    V3 res = frame_mul(n, fabs(n.z), lobe_local(u, v, power, 0, false));
    if (n.z < 0) res.z *= -1.0;
    return res;
}
GI_HD V3 sphere_cap_cos(V3 n, float u, float v, double power, double frac)  // include/util.cpp:60-83
{
    V3 res = frame_mul(n, fabs(n.z), lobe_local(u, v, power, frac, true));
    if (n.z < 0) res.z *= -1.0;
    return res;
}
GI_HD V3 sample_phong(V3 outdir, double power, double sx, double sy)  // include/util.cpp:91-107
{
    V3 out = frame_mul(outdir, fabs(outdir.z), lobe_local((float)sx, (float)sy, power, 0, false));
    if (outdir.z < 0) out.z *= -1.0;
    return out;
}
GI_HD V3 random_unit_vec(double x, double y)  // include/util.h:183-188
{
    double theta = acos(2 * y - 1);
    return v3(sin(theta) * cos(2 * x * GI_PI), sin(theta) * sin(2 * x * GI_PI), cos(theta));
}
GI_HD V3 refr(V3 inc, V3 norm, double eta)  // include/util.h:173-181
{
    double d = dot(norm, inc);
    double k = 1.0 - eta * eta * (1.0 - d * d);
    if (k < GI_EPSILON) return reflect(inc, norm);
    return eta * inc - (eta * d + sqrt(k)) * norm;
}
