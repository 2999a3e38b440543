// gi_host_geom.inc -- double-precision geometry of the host builders: D3, Aabb, the reference's octants, its triangle/box test, the box and
// cell test of the two entity kinds, glm's Euler rotation.  Included by gi_host.cpp (first piece, inside its unnamed namespace).

const double kEps = 0.00001;   // EPSILON, include/util.h:18

struct D3 { double x, y, z; };
inline D3 mk(double x, double y, double z) { D3 r = {x, y, z}; return r; }
inline D3 d3(const double* p) { return mk(p[0], p[1], p[2]); }
inline D3 sub(D3 a, D3 b) { return mk(a.x - b.x, a.y - b.y, a.z - b.z); }
inline D3 add(D3 a, D3 b) { return mk(a.x + b.x, a.y + b.y, a.z + b.z); }
inline D3 scl(D3 a, double s) { return mk(a.x * s, a.y * s, a.z * s); }
inline double dot3(D3 a, D3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
inline D3 cross3(D3 x, D3 y) { return mk(x.y * y.z - y.y * x.z, x.z * y.x - y.z * x.x, x.x * y.y - y.x * x.y); }
inline D3 unit(D3 v) { return scl(v, 1.0 / std::sqrt(dot3(v, v))); }   // glm::normalize = v * inversesqrt(dot)
inline double comp(const D3& v, int i) { return i == 0 ? v.x : (i == 1 ? v.y : v.z); }

struct Aabb { D3 lo, hi; };
inline Aabb load_box(const double* b6) { Aabb b = {d3(b6), d3(b6 + 3)}; return b; }
inline void store_box(const Aabb& b, double* out6) { out6[0] = b.lo.x; out6[1] = b.lo.y; out6[2] = b.lo.z; out6[3] = b.hi.x; out6[4] = b.hi.y; out6[5] = b.hi.z; }
inline double ext_x(const Aabb& b) { return b.hi.x - b.lo.x; }
inline double ext_y(const Aabb& b) { return b.hi.y - b.lo.y; }
inline double ext_z(const Aabb& b) { return b.hi.z - b.lo.z; }
inline D3 centre(const Aabb& b) { return add(b.lo, scl(sub(b.hi, b.lo), 0.5)); }   // min + 0.5*(max-min), include/bbox.h:25
// closed box overlap, include/bbox.h:33-38, and half-open point in box, :41-44
inline bool closed_overlap(const Aabb& a, const Aabb& o) { return (a.lo.x <= o.hi.x && a.hi.x >= o.lo.x) && (a.lo.y <= o.hi.y && a.hi.y >= o.lo.y) && (a.lo.z <= o.hi.z && a.hi.z >= o.lo.z); }
inline bool half_open_contains(const Aabb& b, D3 p) { return p.x >= b.lo.x && p.y >= b.lo.y && p.z >= b.lo.z && p.x < b.hi.x && p.y < b.hi.y && p.z < b.hi.z; }

// the 8 octants in the reference's child numbering and with its exact corner expressions (include/octree.cpp:318-328,
// include/photonMap.cpp:139-149): x is bit 0, z is bit 1, y is bit 2; upper corners are mid + .5*extent, not the parent max
void octants(const Aabb& b, Aabb out[8])
{
    const D3 mid = add(b.lo, scl(sub(b.hi, b.lo), .5));   // glm::mix(min, max, .5) = min + .5*(max - min)
    const double hx = .5 * ext_x(b), hy = .5 * ext_y(b), hz = .5 * ext_z(b);
    for (int i = 0; i < 8; i++) {
        const bool ux = i & 1, uz = i & 2, uy = i & 4;
        out[i].lo = mk(ux ? b.lo.x + hx : b.lo.x, uy ? b.lo.y + hy : b.lo.y, uz ? b.lo.z + hz : b.lo.z);
        out[i].hi = mk(ux ? mid.x + hx : mid.x, uy ? mid.y + hy : mid.y, uz ? mid.z + hz : mid.z);
    }
    out[0].lo = b.lo; out[0].hi = mid;
    out[7].lo = mid; out[7].hi = b.hi;
}

// Akenine-Moeller triangle/box overlap as the reference compiles it (include/util.cpp:186-330): the projections, radii,
// extents and the plane offset are held in *float* variables while the vectors stay double.
struct TriBox {
    D3 v0, v1, v2, h;
    float lo, hi, rad;
    bool sep(double a, double b, float r) { if (a < b) { lo = (float)a; hi = (float)b; } else { lo = (float)b; hi = (float)a; } rad = r; return lo > rad || hi < -rad; }
};
bool tri_overlaps_box(D3 c, D3 half, D3 t0, D3 t1, D3 t2)
{
    TriBox T;
    T.v0 = sub(t0, c); T.v1 = sub(t1, c); T.v2 = sub(t2, c); T.h = half;
    const D3 e0 = sub(T.v1, T.v0), e1 = sub(T.v2, T.v1), e2 = sub(T.v0, T.v2);
    const D3 &v0 = T.v0, &v1 = T.v1, &v2 = T.v2;
    float fx, fy, fz, p, q;
    // edge e0: X01, Y02, Z12
    fx = (float)std::fabs(e0.x); fy = (float)std::fabs(e0.y); fz = (float)std::fabs(e0.z);
    p = (float)(e0.z * v0.y - e0.y * v0.z); q = (float)(e0.z * v2.y - e0.y * v2.z);
    if (T.sep(p, q, (float)(fz * half.y + fy * half.z))) return false;
    p = (float)(-e0.z * v0.x + e0.x * v0.z); q = (float)(-e0.z * v2.x + e0.x * v2.z);
    if (T.sep(p, q, (float)(fz * half.x + fx * half.z))) return false;
    p = (float)(e0.y * v1.x - e0.x * v1.y); q = (float)(e0.y * v2.x - e0.x * v2.y);
    if (T.sep(q, p, (float)(fy * half.x + fx * half.y))) return false;
    // edge e1: X01, Y02, Z0
    fx = (float)std::fabs(e1.x); fy = (float)std::fabs(e1.y); fz = (float)std::fabs(e1.z);
    p = (float)(e1.z * v0.y - e1.y * v0.z); q = (float)(e1.z * v2.y - e1.y * v2.z);
    if (T.sep(p, q, (float)(fz * half.y + fy * half.z))) return false;
    p = (float)(-e1.z * v0.x + e1.x * v0.z); q = (float)(-e1.z * v2.x + e1.x * v2.z);
    if (T.sep(p, q, (float)(fz * half.x + fx * half.z))) return false;
    p = (float)(e1.y * v0.x - e1.x * v0.y); q = (float)(e1.y * v1.x - e1.x * v1.y);
    if (T.sep(p, q, (float)(fy * half.x + fx * half.y))) return false;
    // edge e2: X2, Y1, Z12
    fx = (float)std::fabs(e2.x); fy = (float)std::fabs(e2.y); fz = (float)std::fabs(e2.z);
    p = (float)(e2.z * v0.y - e2.y * v0.z); q = (float)(e2.z * v1.y - e2.y * v1.z);
    if (T.sep(p, q, (float)(fz * half.y + fy * half.z))) return false;
    p = (float)(-e2.z * v0.x + e2.x * v0.z); q = (float)(-e2.z * v1.x + e2.x * v1.z);
    if (T.sep(p, q, (float)(fz * half.x + fx * half.z))) return false;
    p = (float)(e2.y * v1.x - e2.x * v1.y); q = (float)(e2.y * v2.x - e2.x * v2.y);
    if (T.sep(q, p, (float)(fy * half.x + fx * half.y))) return false;
    // the three box axes: min/max of the vertex coordinates kept in float, compared with the double half size
    for (int ax = 0; ax < 3; ax++) {
        const double a = comp(v0, ax), b = comp(v1, ax), cc = comp(v2, ax);
        float mn = (float)a, mx = (float)a;
        if (b < mn) mn = (float)b;
        if (b > mx) mx = (float)b;
        if (cc < mn) mn = (float)cc;
        if (cc > mx) mx = (float)cc;
        if (mn > comp(half, ax) || mx < -comp(half, ax)) return false;
    }
    // triangle plane against the box
    const D3 n = cross3(e0, e1);
    const float d = (float)(-dot3(n, v0));
    D3 vmin, vmax;
    vmin.x = n.x > 0.0f ? -half.x : half.x; vmax.x = n.x > 0.0f ? half.x : -half.x;
    vmin.y = n.y > 0.0f ? -half.y : half.y; vmax.y = n.y > 0.0f ? half.y : -half.y;
    vmin.z = n.z > 0.0f ? -half.z : half.z; vmax.z = n.z > 0.0f ? half.z : -half.z;
    if (dot3(n, vmin) + d > 0.0f) return false;
    if (dot3(n, vmax) + d >= 0.0f) return true;
    return false;
}

// Entity::boundingBox and Entity::intersect(BoundingBox) of the two entity kinds over the 9 position values of one entity
// (0 triangle: three vertices; 1 sphere: centre = p9[0..2], radius = p9[3])
// triangle::boundingBox, include/entities.h:530-557: the upper corner grows by EPSILON after EVERY vertex; sphere::boundingBox, :103-106
Aabb entity_box(int kind, const double* p9)
{
    Aabb b;
    if (kind == 1) {
        const D3 c = d3(p9); const double rad = p9[3];
        b.lo = mk(c.x + rad * -1, c.y + rad * -1, c.z + rad * -1);
        b.hi = mk(c.x + rad * 1, c.y + rad * 1, c.z + rad * 1);
        return b;
    }
    b.lo = mk(INFINITY, INFINITY, INFINITY); b.hi = mk(-INFINITY, -INFINITY, -INFINITY);
    for (int k = 0; k < 3; k++) {
        const D3 p = d3(p9 + k * 3);
        if (p.x < b.lo.x) b.lo.x = p.x;
        if (p.x > b.hi.x) b.hi.x = p.x;
        if (p.y < b.lo.y) b.lo.y = p.y;
        if (p.y > b.hi.y) b.hi.y = p.y;
        if (p.z < b.lo.z) b.lo.z = p.z;
        if (p.z > b.hi.z) b.hi.z = p.z;
        b.hi.x += kEps; b.hi.y += kEps; b.hi.z += kEps;
    }
    return b;
}
// triangle::intersect(BoundingBox), include/entities.h:522-528; sphere::intersect(BoundingBox), :108-141 (squared distance centre-box <= rad^2)
bool entity_in_cell(int kind, const double* p9, const Aabb& cell)
{
    if (kind == 1) {
        const D3 c = d3(p9); const double rad = p9[3];
        double sq = 0.0;
        for (int ax = 0; ax < 3; ax++) {
            const double q = comp(c, ax), lo = comp(cell.lo, ax), hi = comp(cell.hi, ax);
            double out = 0;
            if (q < lo) { const double val = (lo - q); out += val * val; }
            if (q > hi) { const double val = (q - hi); out += val * val; }
            sq += out;
        }
        return sq <= (rad * rad);
    }
    Aabb g;
    g.lo = mk(cell.lo.x - kEps, cell.lo.y - kEps, cell.lo.z - kEps);
    g.hi = mk(cell.hi.x + kEps, cell.hi.y + kEps, cell.hi.z + kEps);
    return tri_overlaps_box(centre(g), mk(ext_x(g) / 2, ext_y(g) / 2, ext_z(g) / 2), d3(p9), d3(p9 + 3), d3(p9 + 6));
}

// glm::eulerAngleXYZ upper 3x3 (3rd_party/glm/gtx/euler_angles.inl:135-167), column-major m[col][row]
struct M3 { double m[3][3]; };
M3 euler_xyz(double t1, double t2, double t3)
{
    const double c1 = std::cos(-t1), c2 = std::cos(-t2), c3 = std::cos(-t3);
    const double s1 = std::sin(-t1), s2 = std::sin(-t2), s3 = std::sin(-t3);
    M3 r;
    r.m[0][0] = c2 * c3;  r.m[0][1] = -c1 * s3 + s1 * s2 * c3;  r.m[0][2] = s1 * s3 + c1 * s2 * c3;
    r.m[1][0] = c2 * s3;  r.m[1][1] = c1 * c3 + s1 * s2 * s3;   r.m[1][2] = -s1 * c3 + c1 * s2 * s3;
    r.m[2][0] = -s2;      r.m[2][1] = s1 * c2;                  r.m[2][2] = c1 * c2;
    return r;
}
inline D3 mul(const M3& r, D3 v)
{
    return mk(r.m[0][0] * v.x + r.m[1][0] * v.y + r.m[2][0] * v.z, r.m[0][1] * v.x + r.m[1][1] * v.y + r.m[2][1] * v.z,
              r.m[0][2] * v.x + r.m[1][2] * v.y + r.m[2][2] * v.z);
}
