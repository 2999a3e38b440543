// gi_layout.h -- host-side construction of the device tables (pure C++, no HIP calls).
//
// Turns the flat C-ABI descriptions (include/gi_hip.h) into the arrays the kernels read (gi_device.h):
//   * layout_scene, one named step per table: the octree's nodes once, breadth first, with hit / skip links per direction octant (TNode); wide
//     records of the inner nodes where the tree is made of exact octants (WNode) and the content boxes of their children; per entity a test,
//     a shading and a uv record, and the test record again per leaf reference (LeafTri); per leaf reference the entity's box (leaf_boxes) and,
//     where the scene allows the closest-hit walk its short cuts (closest_hit_cut_rule, lights_are_clear -> WalkCuts), the box of the part of
//     it inside the leaf (trace_boxes) with content boxes of their own; materials, lights, textures, fog;
//   * layout_photons: the photon octree with the 8 children of a node in consecutive records and the planes their boxes are made of, photons
//     re-ordered leaf by leaf, and every leaf's candidate photon ranges;
//   * apply_scene_switches: which of those tables the walks see under the context's switches;
//   * Halton/Faure digit-group tables, the per-frame Halton enumeration and camera constants, and the pool budget of a fixed-spp call.
// Used by gi_kernels.hip (which uploads the vectors) and by tests/host_emul (which points a gi::Scene at them); tests/test_layout_tables_cpu.py
// pins every table byte for byte and every refusal word for word.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/gi_hip.h"
#include "gi_device.h"

namespace gi {

// What layout_scene found the scene to allow the walks' short cuts.  HostScene and SceneTables are each one of these (a base, so that the three read
// as their own fields) and it is copied whole from the one to the other (through SceneStore): walk_cuts().
struct WalkCuts {
    double cut_margin = -1;           // how far behind its best hit the closest-hit walk still looks (scene_margins: wide); -1 where an entity has an alpha test: it walks on
    bool clipped = false;             // trace_boxes differs from leaf_boxes (never with textures or an alpha-tested entity in the scene)
    bool lights_clear = false;        // nothing can block a shadow segment in its last stretch before a light (lights_are_clear)
};
struct HostScene : WalkCuts {
    const WalkCuts& walk_cuts() const { return *this; }
    std::vector<TNode> tnodes;
    std::vector<WNode> wnodes;        // empty when the tree is not made of exact octants (layout_wide)
    std::vector<int32_t> wleaf_id;
    std::vector<float> cboxes;        // [n_wnode][8][6] content boxes of the children (gi_walk.h: content_cull); one dummy entry without wide records
    std::vector<uint32_t> cuse;       // [n_wnode] children worth testing
    std::vector<int32_t> refs;
    std::vector<LeafTri> leaf_tris;
    std::vector<double> leaf_boxes;   // [n_refs][6] the entity's own box, widened (gi_walk.h: entity_box_missed), parallel to leaf_tris
    std::vector<double> trace_boxes;  // [n_refs][6] for the closest-hit walk: the box of the part of an opaque entity inside its leaf (gi_walk.h: trace_wide_over)
    std::vector<float> tcboxes;       // content boxes made of the trace boxes: what the closest-hit walk culls by (like cboxes; empty when !clipped)
    std::vector<uint32_t> tcuse;
    std::vector<int32_t> worder;      // canonical node of every wide record
    std::vector<TriGeom> tris;
    std::vector<TriShade> shade;
    std::vector<TriUV> tri_uv;
    std::vector<Mat> mats;
    std::vector<LightD> lights;
    std::vector<FogD> fogs;
    std::vector<double> fog_grid;
    std::vector<TexD> texs;           // only when the scene has a non-constant texture (n_tex() > 0)
    std::vector<unsigned char> tex_pixels;
    std::vector<double> tex_lut;
    int32_t n_tex() const { return (int32_t)texs.size(); }
    int32_t n_node = 0, n_tri = 0, n_light = 0;
    double ambient[3] = {0, 0, 0};
    int32_t n_fog() const { return (fogs.size() == 1 && fogs[0].grid_n == 0) ? 0 : (int32_t)fogs.size(); }
};
struct HostPhotons {
    std::vector<PNode> nodes;
    std::vector<PRange> ranges;
    std::vector<double> pos, dircol;
    int32_t n_node = 0, n_photon = 0;
    bool planes_ok = true;            // inner records' planes reproduce every child box (gather_find_leaf's one-record-per-level walk)
};

// The Scene fields that follow the switches.  SceneTables: the tables of the scene and photon map last uploaded, wherever they live (device memory in
// gi_kernels.hip, the HostScene vectors in tests/host_emul) and what layout_scene / layout_photons said about them; S.n_wnode and S.cuse are set.
struct SceneTables : WalkCuts {
    void set_walk_cuts(const WalkCuts& c) { WalkCuts::operator=(c); }      // HostScene's
    const WNode* wnodes = nullptr;
    const float* cboxes = nullptr;  size_t n_cboxes = 0;
    const double* leaf_boxes = nullptr;
    const double* trace_boxes = nullptr;
    const float* tcboxes = nullptr; size_t n_tcboxes = 0;
    const uint32_t* tcuse = nullptr;
    bool pn_planes_ok = false;        // HostPhotons::planes_ok of a map in use
    const PDescent* pdescent = nullptr;   // the fast descent of the gather keys and its jump table, where they were built for the current map
    const int32_t* pjump = nullptr;
};
struct SceneSwitches {
    bool wide = true;                 // gi_set_wide_nodes
    bool cull = true;                 // gi_set_content_culling
    bool entity_boxes = true;         // gi_set_entity_boxes, GI_ENTITY_BOXES=0: every entity of a leaf is tested, as the reference does
    bool clip_boxes = true;           // GI_CLIP_BOXES=0: the closest-hit walk uses the entities' whole boxes
    bool walk_cut = true;             // GI_WALK_CUT=0: the closest-hit walk goes on behind its best hit, as the reference does
};
inline void apply_scene_switches(Scene& S, const SceneTables& T, const SceneSwitches& sw)
{
    S.wnodes = (sw.wide && S.n_wnode > 0) ? T.wnodes : nullptr;
    S.cboxes = (sw.cull && S.wnodes && T.n_cboxes > 1) ? T.cboxes : nullptr;
    // Which of the walks' short cuts are on (all of them leave every result as it is: DESIGN.md section 4): entity boxes; for the closest-hit walk
    // the boxes cut to the leaves, and no look behind the best hit.  Entity boxes off turns all three off: the walks then ask what the reference asks.
    const bool clip = sw.entity_boxes && sw.clip_boxes && T.clipped;
    S.leaf_boxes = sw.entity_boxes ? T.leaf_boxes : nullptr;
    S.trace_boxes = !sw.entity_boxes ? nullptr : (clip ? T.trace_boxes : T.leaf_boxes);
    S.cut_margin = (sw.entity_boxes && sw.walk_cut) ? T.cut_margin : -1.0;
    const bool cut_to_leaves = clip && S.cboxes && T.n_tcboxes == T.n_cboxes;
    S.tcboxes = cut_to_leaves ? T.tcboxes : S.cboxes;
    S.tcuse = cut_to_leaves ? T.tcuse : S.cuse;
    // segments that end at a light (k_st_shadow): the same boxes, as long as nothing can block a segment inside its last GI_SHADOW_BIAS (gi_walk.h: visible_leaf_blocks, shadow_cut)
    const bool sh = T.lights_clear && clip;
    S.shadow_boxes = sh ? S.trace_boxes : S.leaf_boxes;
    S.scboxes = sh ? S.tcboxes : S.cboxes;
    S.scuse = sh ? S.tcuse : S.cuse;
    // the photon octree's counterpart of the wide records (gather_find_leaf), and the fast descent of the gather keys over it
    S.pn_planes = (sw.wide && T.pn_planes_ok) ? 1 : 0;
    S.pdescent = S.pn_planes ? T.pdescent : nullptr;
    S.pjump = S.pdescent ? T.pjump : nullptr;
}

// Faure permutations and per-base digit-group tables of Halton_sampler (include/halton_sampler.h:573-603,890-1414).
inline void build_halton_tables(std::vector<HaltonDim>& dims, std::vector<uint16_t>& table)
{
    const unsigned max_base = 1619u;
    std::vector<std::vector<uint16_t>> perm(max_base + 1);
    for (unsigned k = 1; k <= 3; ++k) { perm[k].resize(k); for (unsigned i = 0; i < k; ++i) perm[k][i] = (uint16_t)i; }
    for (unsigned base = 4; base <= max_base; ++base) {
        std::vector<uint16_t>& pb = perm[base];
        pb.resize(base);
        const unsigned half = base / 2;
        if (base & 1) {
            const std::vector<uint16_t>& prev = perm[base - 1];
            for (unsigned i = 0; i + 1 < base; ++i) pb[i + (i >= half)] = (uint16_t)(prev[i] + (prev[i] >= half));
            pb[half] = (uint16_t)half;
        } else {
            const std::vector<uint16_t>& hp = perm[half];
            for (unsigned i = 0; i < half; ++i) { pb[i] = (uint16_t)(2 * hp[i]); pb[half + i] = (uint16_t)(2 * hp[i] + 1); }
        }
    }
    std::vector<unsigned> primes;
    for (unsigned c = 2; primes.size() < 256; c++) {
        bool is_prime = true;
        for (unsigned p : primes) { if (p * p > c) break; if (c % p == 0) { is_prime = false; break; } }
        if (is_prime) primes.push_back(c);
    }
    dims.resize(256);
    table.clear();
    for (unsigned d = 0; d < 256; d++) {
        const unsigned b = primes[d];
        unsigned digits = 1, P = b;
        while ((unsigned long long)P * b <= 500ull) { P *= b; digits++; }      // table over the largest b^g <= 500
        unsigned groups = 1;
        unsigned long long full = P;
        while (full * P < 4294967296ull) { full *= P; groups++; }               // groups with (b^g)^n < 2^32
        dims[d].P = P; dims[d].n = groups; dims[d].off = (uint32_t)table.size();
        dims[d].scale = float(0.9999998807907104 / (double)full);
        // groups <= 7: the longest chain is base 23 (23^7 < 2^32 <= 23^8); halton_sample unrolls 7 (all 256 dims are checked bit for bit by the tests)
        const unsigned long long magic = 0xffffffffffffffffull / P + 1ull;
        dims[d].mlo = (uint32_t)magic; dims[d].mhi = (uint32_t)(magic >> 32); dims[d].pad[0] = dims[d].pad[1] = 0;
        for (unsigned i = 0; i < P; i++) {
            unsigned rest = i;
            uint16_t inv = 0;
            for (unsigned k = 0; k < digits; ++k) { inv = (uint16_t)(inv * b + perm[b][rest % b]); rest /= b; }
            table.push_back(inv);
        }
    }
}

inline HaltonEnumD make_halton_enum(unsigned width, unsigned height)  // Halton_enum ctor, include/halton_enum.h:69-104
{
    HaltonEnumD e;
    unsigned w = 1, h = 1;
    e.p2 = 0; while (w < width) { ++e.p2; w *= 2; }
    e.p3 = 0; while (h < height) { ++e.p3; h *= 3; }
    e.scale_x = float(w); e.scale_y = float(h);
    e.inc = w * h;
    // extended Euclid on (h, w), iterative: s0*h + t0*w == gcd == 1
    long long a = (long long)h, b = (long long)w, s0 = 1, s1 = 0, t0 = 0, t1 = 1;
    while (b) {
        long long q = a / b, r = a % b;
        a = b; b = r;
        long long s2 = s0 - q * s1; s0 = s1; s1 = s2;
        long long t2 = t0 - q * t1; t0 = t1; t1 = t2;
    }
    unsigned inv2 = (s0 < 0) ? (unsigned)(s0 + (long long)w) : (unsigned)(s0 % (long long)w);
    unsigned inv3 = (t0 < 0) ? (unsigned)(t0 + (long long)h) : (unsigned)(t0 % (long long)h);
    e.m_x = h * inv2;
    e.m_y = w * inv3;
    return e;
}

// ---- vocabulary over the descriptors.  The scene's octree (gi_scene_desc) and the photon octree (gi_photon_map_desc) come as the same tables:
// node_child [n][8] in pre-order (-1: no child) and node_bbox [n][6] = lo[3], hi[3].
inline bool node_is_inner(const int32_t* node_child, int n)
{
    for (int k = 0; k < 8; k++) if (node_child[(size_t)n * 8 + k] >= 0) return true;
    return false;
}
inline const double* node_box(const double* node_bbox, int n) { return node_bbox + (size_t)n * 6; }
struct RefRange { int32_t first, count; };     // the leaf references [first, first + count) of a scene node
inline RefRange node_refs(const gi_scene_desc* d, int n) { return {d->node_ent_off[n], d->node_ent_off[n + 1] - d->node_ent_off[n]}; }
// the bit of a child's slot that says "high side" on axis ax: x = bit 0, z = bit 1, y = bit 2 (include/octree.cpp:321-328)
inline int axis_slot_bit(int ax) { return ax == 0 ? 0 : (ax == 1 ? 2 : 1); }
inline bool entity_is_sphere(const gi_scene_desc* d, int e) { return d->ent_kind && d->ent_kind[e] == 1; }
// The exact box of entity e (sphere: centre P[0..2] -+ radius P[3]; triangle: its vertices), nothing added.  Not gi_host_geom.inc: entity_box, which
// is the reference's box with its EPSILON growth and decides which leaves refer to the entity.
inline void entity_bounds(const gi_scene_desc* d, int e, double* lo, double* hi)
{
    const double* P = d->tri_pos + (size_t)e * 9;
    for (int ax = 0; ax < 3; ax++) {
        if (entity_is_sphere(d, e)) { lo[ax] = P[ax] - P[3]; hi[ax] = P[ax] + P[3]; continue; }
        lo[ax] = std::min(P[ax], std::min(P[3 + ax], P[6 + ax]));
        hi[ax] = std::max(P[ax], std::max(P[3 + ax], P[6 + ax]));
    }
}
// Breadth-first numbering of a pre-order tree from its root: order[r] = the node of record r, rec_of[n] = the record of node n or -1.  The children
// of a node get consecutive records in slot order; follow(ch) says which children get one at all.  False when a node is reached a second time.
template <class Follow>
inline bool number_breadth_first(const int32_t* node_child, int n_node, Follow follow, std::vector<int32_t>& order, std::vector<int32_t>& rec_of)
{
    rec_of.assign((size_t)n_node, -1);
    order.clear();
    order.reserve((size_t)n_node);
    rec_of[0] = 0;
    order.push_back(0);
    for (size_t head = 0; head < order.size(); head++)
        for (int k = 0; k < 8; k++) {
            const int ch = node_child[(size_t)order[head] * 8 + k];
            if (ch < 0 || !follow(ch)) continue;
            if (rec_of[ch] != -1) return false;
            rec_of[ch] = (int32_t)order.size();
            order.push_back(ch);
        }
    return true;
}
// The two margins every box of the scene is widened by.
//   tight, 1e-7 of the scene's extent: a hit point is off its entity by ~1e-16 of its coordinates, so this leaves eight orders of slack; the
//     entities' own boxes (leaf_boxes) and the content boxes made of them carry it.
//   wide, 1e-5 of the extent or of the farthest coordinate: the tree builder decides in float arithmetic which leaves an entity overlaps (relative
//     error 1e-7 of the coordinates), so a leaf is taken this much larger before an entity is cut to it, the box of what is left is widened by as
//     much again, and the closest-hit walk looks this far behind its best hit: a hit point within rounding of a leaf is never refused there.
struct SceneMargins { double tight, wide; };
inline SceneMargins scene_margins(const gi_scene_desc* d)
{
    double extent = 0, reach = 0;
    for (int ax = 0; ax < 3; ax++) {
        extent = std::max(extent, d->node_bbox[3 + ax] - d->node_bbox[ax]);
        reach = std::max(reach, std::max(std::fabs(d->node_bbox[ax]), std::fabs(d->node_bbox[3 + ax])));
    }
    return {1e-7 * std::max(extent, 1e-3), 1e-5 * std::max(std::max(extent, reach), 1e-3)};
}
inline bool scene_is_textured(const gi_scene_desc* d)      // something is not a constant colour: the kernels take the GI_FEAT_TEX instances
{
    for (int t = 0; t < d->n_tex; t++) if (d->tex_kind[t] != 0) return true;
    return false;
}

// ---- layout_scene's refusals, in the order they are met: the flat tables, the tree's shape, the atmosphere
inline bool validate_scene(const gi_scene_desc* d, std::string& err)
{
    if (!d || d->n_tri < 0 || d->n_mat <= 0 || d->n_light < 0 || d->n_node <= 0) { err = "scene: bad counts"; return false; }
    if (d->n_tri && (!d->tri_pos || !d->tri_nrm || !d->tri_mat)) { err = "scene: null triangle tables"; return false; }
    if (!d->mats || !d->node_bbox || !d->node_child || !d->node_ent_off || (d->n_light && !d->lights)) { err = "scene: null tables"; return false; }
    for (int i = 0; i < d->n_tri; i++) {
        if (d->tri_mat[i] < 0 || d->tri_mat[i] >= d->n_mat) { err = "scene: material index out of range"; return false; }
        if (d->ent_kind && d->ent_kind[i] != 0 && d->ent_kind[i] != 1) { err = "scene: unknown entity kind"; return false; }
    }
    if (d->n_mat >= (1 << 28)) { err = "scene: too many materials"; return false; }
    if (d->n_tex < 0 || (d->n_tex > 0 && (!d->tex_kind || !d->tex_param || !d->mat_tex))) { err = "scene: null texture tables"; return false; }
    for (int t = 0; t < d->n_tex; t++) {
        const double* q = d->tex_param + (size_t)t * 8;
        if (d->tex_kind[t] < 0 || d->tex_kind[t] > 2) { err = "scene: unknown texture kind"; return false; }
        if (d->tex_kind[t] == 2) {
            const double w = q[2], h = q[3], off = q[5];
            if (!(w >= 1 && h >= 1 && w <= 32768 && h <= 32768 && off >= 0) || !d->tex_pixels || off + w * h * 4 > (double)d->n_tex_pixel_bytes) { err = "scene: image texture outside the pixel table"; return false; }
        }
    }
    if (d->n_tex > 0)
        for (int m = 0; m < d->n_mat * 2; m++)
            if (d->mat_tex[m] < -1 || d->mat_tex[m] >= d->n_tex) { err = "scene: material texture index out of range"; return false; }
    const int nref = d->node_ent_off[d->n_node];
    if (d->node_ent_off[0] != 0 || nref < 0 || (nref && !d->node_ent_idx)) { err = "scene: bad leaf reference table"; return false; }
    for (int n = 0; n < d->n_node; n++) {
        if (d->node_ent_off[n + 1] < d->node_ent_off[n]) { err = "scene: leaf offsets not monotone"; return false; }
        for (int k = 0; k < 8; k++) {
            int ch = d->node_child[(size_t)n * 8 + k];
            if (ch != -1 && (ch <= n || ch >= d->n_node)) { err = "scene: child index is not a later pre-order node"; return false; }
        }
    }
    for (int r = 0; r < nref; r++)
        if (d->node_ent_idx[r] < 0 || d->node_ent_idx[r] >= d->n_tri) { err = "scene: leaf reference out of range"; return false; }
    return true;
}
// breadth-first record order of the scene's nodes: the ones every ray visits (top levels) come first and are what the kernels keep in LDS
inline bool number_scene_nodes(const gi_scene_desc* d, std::vector<int32_t>& order, std::vector<int32_t>& rec_of, std::string& err)
{
    if (!number_breadth_first(d->node_child, d->n_node, [](int) { return true; }, order, rec_of)) { err = "scene: octree node has two parents"; return false; }
    if ((int)order.size() != d->n_node) { err = "scene: octree is not one connected tree"; return false; }
    return true;
}
inline bool validate_fog(const gi_scene_desc* d, std::string& err)
{
    if (d->n_fog < 0 || (d->n_fog > 0 && (!d->fog || !d->fog_grid_off || !d->fog_grid))) { err = "scene: bad atmosphere tables"; return false; }
    for (int i = 0; i < d->n_fog; i++)
        if (d->fog_grid_off[i + 1] - d->fog_grid_off[i] <= 0 || d->fog_grid_off[i] < 0) { err = "scene: empty fog noise grid"; return false; }
    return true;
}

// ---- the steps of layout_scene, in its order
// per-octant links of the canonical tree: visiting the children of every node in the order k ^ a (k = 0..7) is front to back for
// every ray whose direction signs are `a` (slot bits: axis_slot_bit).
// hit = first child in that order; skip = next sibling in that order, or the parent's skip after the last child.
inline void link_octant(const gi_scene_desc* d, int a, int node, int32_t skip_to, const std::vector<int32_t>& rec_of, std::vector<TNode>& out)
{
    TNode& t = out[(size_t)rec_of[node]];
    int kids[8], nk = 0;
    for (int k = 0; k < 8; k++) { int ch = d->node_child[(size_t)node * 8 + (k ^ a)]; if (ch >= 0) kids[nk++] = ch; }
    t.link[a].skip = skip_to;
    t.link[a].hit = nk ? rec_of[kids[0]] : skip_to;
    for (int i = 0; i < nk; i++) link_octant(d, a, kids[i], i + 1 < nk ? rec_of[kids[i + 1]] : skip_to, rec_of, out);
}
// the per-node records (the walk without wide records, and every leaf's id), in the breadth-first order, and their links
inline void layout_tnodes(const gi_scene_desc* d, const std::vector<int32_t>& rec_of, HostScene& H)
{
    const int N = d->n_node;
    H.tnodes.assign((size_t)N, TNode());
    for (int n = 0; n < N; n++) {
        TNode& t = H.tnodes[(size_t)rec_of[n]];
        memset(&t, 0, sizeof t);
        const double* b = node_box(d->node_bbox, n);
        for (int k = 0; k < 3; k++) { t.bmin[k] = b[k]; t.bmax[k] = b[3 + k]; }
        t.first_ref = node_refs(d, n).first;
        t.n_ref = node_is_inner(d->node_child, n) ? -1 : node_refs(d, n).count;
        t.leaf_id = n;
    }
    for (int a = 0; a < 8; a++) link_octant(d, a, 0, N, rec_of, H.tnodes);
    H.n_node = N;
}
// The planes of node n's octants on axis ax, read off its children's boxes: pl = {min, mid, lo2, hi2, max, mid}, where the low side spans [min, mid],
// the high side [lo2, hi2] and child 7 [mid, max] (include/octree.cpp:318-328).  False unless every existing child's box is made of them bit for bit.
inline bool octant_planes(const gi_scene_desc* d, int n, int ax, double* pl)
{
    const double mn = node_box(d->node_bbox, n)[ax], mx = node_box(d->node_bbox, n)[3 + ax];
    // the values partition() computes; replaced below by what the children's boxes actually hold
    double mid = mn * 0.5 + mx * 0.5, lo2 = mn + .5 * (mx - mn), hi2 = mid + .5 * (mx - mn);
    bool have_mid = false, have_hi = false;
    for (int c = 0; c < 8; c++) {
        const int ch = d->node_child[(size_t)n * 8 + c];
        if (ch < 0) continue;
        const double clo = node_box(d->node_bbox, ch)[ax], chi = node_box(d->node_bbox, ch)[3 + ax];
        if (c == 7) {
            if (chi != mx) return false;
            if (have_mid && clo != mid) return false;
            mid = clo; have_mid = true;
        } else if (((c >> axis_slot_bit(ax)) & 1) == 0) {
            if (clo != mn) return false;
            if (have_mid && chi != mid) return false;
            mid = chi; have_mid = true;
        } else {
            if (have_hi && (clo != lo2 || chi != hi2)) return false;
            lo2 = clo; hi2 = chi; have_hi = true;
        }
    }
    pl[0] = mn; pl[1] = mid; pl[2] = lo2; pl[3] = hi2; pl[4] = mx; pl[5] = mid;
    return true;
}
// Wide records (gi_scene.h: WNode) for the inner nodes, breadth first; H.worder = the node of every record.  Every existing child's box must be
// the octant Octree::Node::partition gives it (octant_planes), and no inner node lies deeper than 15: the walk keeps one mask byte per level in
// 128 bits.  Returns false, with no wide records in H, for any other tree.
inline bool layout_wide(const gi_scene_desc* d, HostScene& H)
{
    H.wnodes.clear(); H.wleaf_id.clear(); H.worder.clear();
    if (!node_is_inner(d->node_child, 0)) return false;
    std::vector<int32_t> order, wrec;
    if (!number_breadth_first(d->node_child, d->n_node, [d](int ch) { return node_is_inner(d->node_child, ch); }, order, wrec)) return false;
    std::vector<WNode> W(order.size());
    std::vector<int32_t> L(order.size() * 8, -1), depth(order.size(), 0);
    for (WNode& w : W) { memset(&w, 0, sizeof w); w.parent = -1; }
    for (size_t r = 0; r < order.size(); r++) {
        const int n = order[r];
        WNode& w = W[r];
        for (int ax = 0; ax < 3; ax++) if (!octant_planes(d, n, ax, w.pl[ax])) return false;
        for (int c = 0; c < 8; c++) {
            const int ch = d->node_child[(size_t)n * 8 + c];
            if (ch < 0) continue;
            if (node_is_inner(d->node_child, ch)) {
                w.ca[c] = wrec[ch]; w.cb[c] = -1; w.exists |= 1u << c;
                W[(size_t)wrec[ch]].parent = (int32_t)r;
                if ((depth[(size_t)wrec[ch]] = depth[r] + 1) > 15) return false;
            } else {
                w.ca[c] = node_refs(d, ch).first; w.cb[c] = node_refs(d, ch).count;
                if (w.cb[c] > 0) w.exists |= 1u << c;
                L[r * 8 + c] = ch;
            }
        }
    }
    H.worder.swap(order);
    H.wnodes.swap(W);
    H.wleaf_id.swap(L);
    return true;
}
// Content boxes: for every child of every wide record the union of the boxes of everything referenced in its sub-tree, widened by `margin` and
// rounded outwards to float, and (cuse) which children's boxes are clearly smaller than their octants.  ref_boxes = null: the entities' exact
// boxes; else one box per leaf reference -- an entry with b[0] = 1e300 stands for "nothing of it near the leaf".  Without wide records: one
// dummy entry each, so that the tables are never null.
inline void layout_cboxes(const gi_scene_desc* d, const HostScene& H, const double* ref_boxes, double margin, std::vector<float>& cboxes, std::vector<uint32_t>& cuse)
{
    if (H.wnodes.empty()) { cboxes.assign(1, 0.f); cuse.assign(1, 0u); return; }
    const int N = d->n_node;
    std::vector<double> cb((size_t)N * 6);
    for (int n = N - 1; n >= 0; n--) {      // children come later in pre-order
        double* b = &cb[(size_t)n * 6];
        b[0] = b[1] = b[2] = INFINITY; b[3] = b[4] = b[5] = -INFINITY;
        auto add = [b](const double* lo, const double* hi) { for (int ax = 0; ax < 3; ax++) { b[ax] = std::min(b[ax], lo[ax]); b[3 + ax] = std::max(b[3 + ax], hi[ax]); } };
        const RefRange refs = node_refs(d, n);
        for (int r = refs.first; r < refs.first + refs.count; r++) {
            double lo[3], hi[3];
            if (ref_boxes) { if (ref_boxes[(size_t)r * 6] != 1e300) add(ref_boxes + (size_t)r * 6, ref_boxes + (size_t)r * 6 + 3); continue; }
            entity_bounds(d, d->node_ent_idx[r], lo, hi);
            add(lo, hi);
        }
        for (int k = 0; k < 8; k++) {
            const int ch = d->node_child[(size_t)n * 8 + k];
            if (ch >= 0) add(&cb[(size_t)ch * 6], &cb[(size_t)ch * 6 + 3]);
        }
    }
    cboxes.assign(H.worder.size() * 48, 0.f);
    cuse.assign(H.worder.size(), 0u);
    for (size_t r = 0; r < H.worder.size(); r++)
        for (int c = 0; c < 8; c++) {
            const int ch = d->node_child[(size_t)H.worder[r] * 8 + c];
            if (ch < 0 || !(H.wnodes[r].exists & (1u << c))) continue;
            const double* b = &cb[(size_t)ch * 6];
            const double* oct = node_box(d->node_bbox, ch);
            float* out = &cboxes[(r * 8 + (size_t)c) * 6];
            double share = 1.0;                                // how much of the octant the content (clipped to it) fills
            for (int ax = 0; ax < 3; ax++) {
                // (a sub-tree none of whose entities comes near its leaves: an empty box, which no ray touches)
                out[ax] = b[ax] > b[3 + ax] ? INFINITY : std::nextafterf((float)(b[ax] - margin), -INFINITY);
                out[3 + ax] = b[ax] > b[3 + ax] ? -INFINITY : std::nextafterf((float)(b[3 + ax] + margin), INFINITY);
                const double len = std::min((double)out[3 + ax], oct[3 + ax]) - std::max((double)out[ax], oct[ax]);
                share *= oct[3 + ax] > oct[ax] ? std::max(0.0, std::min(1.0, len / (oct[3 + ax] - oct[ax]))) : 1.0;
            }
            if (share < 0.6) cuse[r] |= 1u << c;             // the extra test is only made where it can reject something
        }
}
// the per-entity records: what a ray-entity test needs (TriGeom), what shading needs (TriShade, TriUV)
inline void layout_entities(const gi_scene_desc* d, HostScene& H)
{
    H.n_tri = d->n_tri;
    H.tris.resize((size_t)d->n_tri);
    H.shade.resize((size_t)d->n_tri);
    H.tri_uv.resize((size_t)d->n_tri);
    for (int i = 0; i < d->n_tri; i++) {
        const double* P = d->tri_pos + (size_t)i * 9;
        const double* N = d->tri_nrm + (size_t)i * 9;
        V3 p0 = ld3(P), p1 = ld3(P + 3), p2 = ld3(P + 6);
        V3 e1 = p1 - p0, e2 = p2 - p0;
        TriGeom& g = H.tris[i];
        g.p0[0] = p0.x; g.p0[1] = p0.y; g.p0[2] = p0.z;
        g.e1[0] = e1.x; g.e1[1] = e1.y; g.e1[2] = e1.z;
        g.e2[0] = e2.x; g.e2[1] = e2.y; g.e2[2] = e2.z;
        g.mat = d->tri_mat[i];
        const double* m = d->mats + (size_t)g.mat * 9;
        const bool sphere = entity_is_sphere(d, i);
        const bool smooth = !sphere && len2(ld3(N)) > 0 && len2(ld3(N + 3)) > 0 && len2(ld3(N + 6)) > 0;   // include/entities.h:478
        bool tex_has_alpha = false;   // Material::getAlpha = opacity * diffuse->getAlpha(uv): below 1 wherever an image's alpha channel says so
        if (d->n_tex > 0) { const int dt = d->mat_tex[(size_t)g.mat * 2]; tex_has_alpha = dt >= 0 && d->tex_kind[dt] == 2 && d->tex_param[(size_t)dt * 8 + 4] != 0; }
        const bool always = (!tex_has_alpha && m[1] * 1.0 >= 1.0) || (m[2] != 1);                // include/raytracer.h:455
        g.flags = (smooth ? 1u : 0u) | (always ? 2u : 0u) | (sphere ? 4u : 0u);
        if (sphere) { g.e1[0] = P[3]; g.e1[1] = 0; g.e1[2] = 0; g.e2[0] = 0; g.e2[1] = 0; g.e2[2] = 0; }   // centre in p0, radius in e1[0]
        TriShade& s = H.shade[i];
        for (int k = 0; k < 3; k++) { s.n0[k] = N[k]; s.n1[k] = N[3 + k]; s.n2[k] = N[6 + k]; }
        V3 fn = sphere ? v3(0, 0, 0) : normalize(cross((p1 - p0), (p2 - p0)));                   // include/entities.h:339
        s.fnorm[0] = fn.x; s.fnorm[1] = fn.y; s.fnorm[2] = fn.z;
        if (sphere) { s.n0[0] = P[0]; s.n0[1] = P[1]; s.n0[2] = P[2]; }                         // centre, for the shading normal
        TriUV& tu = H.tri_uv[i];
        for (int k = 0; k < 2; k++) { tu.t0[k] = d->tri_uv ? d->tri_uv[(size_t)i * 6 + k] : 0; tu.t1[k] = d->tri_uv ? d->tri_uv[(size_t)i * 6 + 2 + k] : 0; tu.t2[k] = d->tri_uv ? d->tri_uv[(size_t)i * 6 + 4 + k] : 0; }
    }
}
// the leaf references, and the test record once more per reference, so that a leaf's entities are consecutive in memory
inline void layout_leaf_tris(const gi_scene_desc* d, HostScene& H)
{
    H.refs.assign(d->node_ent_idx, d->node_ent_idx + d->node_ent_off[d->n_node]);
    H.leaf_tris.resize(H.refs.size());
    for (size_t r = 0; r < H.refs.size(); r++) {
        const TriGeom& g = H.tris[(size_t)H.refs[r]];
        LeafTri& lt = H.leaf_tris[r];
        for (int k = 0; k < 3; k++) { lt.p0[k] = g.p0[k]; lt.e1[k] = g.e1[k]; lt.e2[k] = g.e2[k]; }
        lt.tri = H.refs[r];
        lt.matflags = ((uint32_t)g.mat << 3) | g.flags;
    }
    if (H.leaf_tris.empty()) H.leaf_tris.resize(1);
}
// the entities' own boxes, leaf-reference order: what a ray has to touch before Entity::intersect can succeed
inline void layout_leaf_boxes(const gi_scene_desc* d, const SceneMargins& m, HostScene& H)
{
    H.leaf_boxes.assign(std::max<size_t>(H.refs.size(), 1) * 6, 0.0);
    for (size_t r = 0; r < H.refs.size(); r++) {
        double lo[3], hi[3];
        entity_bounds(d, H.refs[r], lo, hi);
        for (int ax = 0; ax < 3; ax++) { H.leaf_boxes[r * 6 + ax] = lo[ax] - m.tight; H.leaf_boxes[r * 6 + 3 + ax] = hi[ax] + m.tight; }
    }
}
// Which short cuts the closest-hit walk of this scene may take.  Both -- boxes cut to the leaves, and no look behind the best hit -- take for
// granted that an entity asked from a later leaf cannot yield a strictly nearer hit.  An entity with an alpha test (flag 2 clear) breaks that: the
// test draws per (leaf, entity) (include/raytracer.h:455), so one that failed its draw from an early leaf is drawn again from every later leaf
// that refers to it and may win there, nearer than the best hit so far -- and the reference walks on to the end of the ray unless the best hit
// lies inside the leaf it was found from.  Cutting only the OPAQUE entities of such a scene is wrong too: it moves the point where the walk ends
// in front of that later draw.  So a scene with any alpha-tested entity gets neither: cut_margin = -1, whole boxes, no tcboxes.  Everything in a
// scene with textures keeps its whole box as well (a hit leaves its uv behind for the next entity's alpha look-up).
struct CutRule { bool behind_hit, to_leaves; };
inline CutRule closest_hit_cut_rule(const gi_scene_desc* d, const HostScene& H)
{
    bool alpha_tested = false;
    for (const TriGeom& g : H.tris) if (!(g.flags & 2u)) alpha_tested = true;
    return {!alpha_tested, !alpha_tested && !scene_is_textured(d)};
}
// Sutherland-Hodgman: the triangle P[3][3] against the six planes of the box [lo, hi], in doubles.  The bounds of the polygon that is left, or
// false when nothing is.  (A triangle cut by six planes has at most nine corners.)
inline bool clip_triangle_to_box(const double* P, const double* lo, const double* hi, double* cmin, double* cmax)
{
    double poly[2][10][3];
    int np = 3, cur = 0;
    for (int v = 0; v < 3; v++) for (int ax = 0; ax < 3; ax++) poly[0][v][ax] = P[v * 3 + ax];
    for (int pl = 0; pl < 6 && np > 0; pl++) {
        const int ax = pl >> 1;
        const bool upper = pl & 1;
        const double lim = upper ? hi[ax] : lo[ax];
        int nn = 0;
        for (int v = 0; v < np; v++) {
            const double* A = poly[cur][v];
            const double* B = poly[cur][(v + 1) % np];
            const bool ain = upper ? A[ax] <= lim : A[ax] >= lim, bin = upper ? B[ax] <= lim : B[ax] >= lim;
            if (ain) { for (int k = 0; k < 3; k++) poly[cur ^ 1][nn][k] = A[k]; nn++; }
            if (ain != bin) {
                const double f = (lim - A[ax]) / (B[ax] - A[ax]);
                for (int k = 0; k < 3; k++) poly[cur ^ 1][nn][k] = k == ax ? lim : A[k] + f * (B[k] - A[k]);
                nn++;
            }
        }
        cur ^= 1;
        np = nn;
    }
    double mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int v = 0; v < np; v++) for (int ax = 0; ax < 3; ax++) { mn[ax] = std::min(mn[ax], poly[cur][v][ax]); mx[ax] = std::max(mx[ax], poly[cur][v][ax]); }
    for (int ax = 0; ax < 3; ax++) { cmin[ax] = mn[ax]; cmax[ax] = mx[ax]; }
    return mn[0] <= mx[0] && mn[1] <= mx[1] && mn[2] <= mx[2];
}
// The closest-hit walk's boxes (gi_walk.h: trace_wide_over) and its margin, as closest_hit_cut_rule allows: the box of the part of an entity
// inside the leaf that refers to it -- the leaf taken m.wide larger, the box of what is left widened by as much again (scene_margins) and never
// larger than the entity's own box.  Nothing of the entity near the leaf: a point no ray of the scene reaches (entity_box_missed has no empty box).
inline void layout_trace_boxes(const gi_scene_desc* d, const SceneMargins& m, HostScene& H)
{
    const CutRule cut = closest_hit_cut_rule(d, H);
    H.cut_margin = cut.behind_hit ? m.wide : -1.0;
    H.clipped = false;
    H.trace_boxes = H.leaf_boxes;
    for (int n = 0; n < d->n_node && cut.to_leaves; n++) {
        if (node_is_inner(d->node_child, n)) continue;
        double lo[3], hi[3], cmin[3], cmax[3];
        for (int ax = 0; ax < 3; ax++) { lo[ax] = node_box(d->node_bbox, n)[ax] - m.wide; hi[ax] = node_box(d->node_bbox, n)[3 + ax] + m.wide; }
        const RefRange refs = node_refs(d, n);
        for (int r = refs.first; r < refs.first + refs.count; r++) {
            const int e = H.refs[(size_t)r];
            double* b = &H.trace_boxes[(size_t)r * 6];
            H.clipped = true;
            bool some;
            if (entity_is_sphere(d, e)) {
                entity_bounds(d, e, cmin, cmax);
                for (int ax = 0; ax < 3; ax++) { cmin[ax] = std::max(cmin[ax], lo[ax]); cmax[ax] = std::min(cmax[ax], hi[ax]); }
                some = cmin[0] <= cmax[0] && cmin[1] <= cmax[1] && cmin[2] <= cmax[2];
            } else
                some = clip_triangle_to_box(d->tri_pos + (size_t)e * 9, lo, hi, cmin, cmax);
            for (int ax = 0; ax < 3; ax++) { b[ax] = some ? std::max(b[ax], cmin[ax] - m.wide) : 1e300; b[3 + ax] = some ? std::min(b[3 + ax], cmax[ax] + m.wide) : 1e300; }
        }
    }
}
// the content boxes made of the trace boxes (which carry their margin already): only where something was cut and there are wide records
inline void layout_trace_cboxes(const gi_scene_desc* d, HostScene& H)
{
    H.tcboxes.clear(); H.tcuse.clear();
    if (H.clipped && !H.wnodes.empty()) layout_cboxes(d, H, H.trace_boxes.data(), 0.0, H.tcboxes, H.tcuse);
}
// RayTracer::visible walks a segment up to GI_SHADOW_BIAS before the light but lets anything up to the light itself block it
// (include/raytracer.h:290-305): a hit in that last stretch is only found from leaves the walk meets earlier.  Where no entity's box comes within a
// light's radius + twice the bias + 4 wide margins of the light (every scene of the reference: lights hang in free space) the stretch is empty
// and the leaf-cut boxes serve shadow segments too.
inline bool lights_are_clear(const gi_scene_desc* d, const SceneMargins& m)
{
    for (int li = 0; li < d->n_light; li++) {
        const double* l = d->lights + (size_t)li * 11;
        const double R = l[6] + 2 * GI_SHADOW_BIAS + 4 * m.wide;
        for (int e = 0; e < d->n_tri; e++) {
            double lo[3], hi[3], d2 = 0;
            entity_bounds(d, e, lo, hi);
            for (int ax = 0; ax < 3; ax++) {
                const double g = l[ax] < lo[ax] ? lo[ax] - l[ax] : (l[ax] > hi[ax] ? l[ax] - hi[ax] : 0.0);
                d2 += g * g;
            }
            if (!(d2 > R * R)) return false;
        }
    }
    return d->n_light > 0;
}
inline void layout_materials(const gi_scene_desc* d, HostScene& H)
{
    const bool textured = scene_is_textured(d);      // else every colour is the material's own: no texture records (layout_textures)
    H.mats.resize((size_t)d->n_mat);
    for (int i = 0; i < d->n_mat; i++) {
        const double* m = d->mats + (size_t)i * 9;
        H.mats[i].roughness = m[0]; H.mats[i].opacity = m[1]; H.mats[i].ior = m[2];
        for (int k = 0; k < 3; k++) { H.mats[i].diffuse[k] = m[3 + k]; H.mats[i].emissive[k] = m[6 + k]; }
        H.mats[i].dtex = textured ? d->mat_tex[(size_t)i * 2] : -1;
        H.mats[i].etex = textured ? d->mat_tex[(size_t)i * 2 + 1] : -1;
    }
}
inline void layout_lights(const gi_scene_desc* d, HostScene& H)
{
    H.n_light = d->n_light;
    H.lights.resize((size_t)d->n_light);
    for (int i = 0; i < d->n_light; i++) {
        const double* l = d->lights + (size_t)i * 11;
        for (int k = 0; k < 3; k++) { H.lights[i].pos[k] = l[k]; H.lights[i].col[k] = l[3 + k]; H.lights[i].dir[k] = l[7 + k]; }
        H.lights[i].rad = l[6]; H.lights[i].angle = l[10];
    }
    for (int k = 0; k < 3; k++) H.ambient[k] = d->ambient[k];
}
// textures: device records only when something is not a constant colour (scene_is_textured)
inline void layout_textures(const gi_scene_desc* d, HostScene& H)
{
    H.texs.clear(); H.tex_pixels.clear(); H.tex_lut.clear();
    if (!scene_is_textured(d)) return;
    H.texs.resize((size_t)d->n_tex);
    for (int t = 0; t < d->n_tex; t++) {
        const double* q = d->tex_param + (size_t)t * 8;
        TexD& x = H.texs[t];
        memset(&x, 0, sizeof x);
        x.kind = d->tex_kind[t];
        if (x.kind == 2) { x.tile_u = q[0]; x.tile_v = q[1]; x.w = (int32_t)q[2]; x.h = (int32_t)q[3]; x.has_alpha = q[4] != 0; x.pix = (unsigned long long)q[5]; }
        else { for (int k = 0; k < 3; k++) { x.a[k] = q[k]; x.b[k] = q[3 + k]; } x.tiles = q[6]; }
    }
    if (d->n_tex_pixel_bytes > 0) H.tex_pixels.assign(d->tex_pixels, d->tex_pixels + d->n_tex_pixel_bytes);
    // imageTexture::get: gamma({p/255}, 1.0/GAMMA) = pow(p / 255.0, 1.0 / (1.0 / 2.2)) (include/material.h:67, include/util.h:94-97),
    // evaluated once per 8-bit value with the host's libm -- the library the reference itself calls
    H.tex_lut.resize(256);
    const double g = 1.0 / 2.2;
    for (int k = 0; k < 256; k++) H.tex_lut[k] = std::pow(k / 255.0, 1.0 / g);
}
inline void layout_fog(const gi_scene_desc* d, HostScene& H)      // (validate_fog has passed)
{
    H.fogs.clear(); H.fog_grid.clear();
    for (int i = 0; i < d->n_fog; i++) {
        const double* q = d->fog + (size_t)i * 12;
        FogD f;
        for (int k = 0; k < 3; k++) {
            f.pos[k] = q[k]; f.size[k] = q[3 + k]; f.col[k] = q[6 + k];
            f.bmin[k] = q[k] - .5 * q[3 + k]; f.bmax[k] = q[k] + .5 * q[3 + k];   // AtmosphereEntity ctor, include/atmosphere.h:14
        }
        f.d = q[9]; f.sc = q[10];
        f.grid_off = d->fog_grid_off[i];
        f.grid_n = d->fog_grid_off[i + 1] - d->fog_grid_off[i];
        H.fogs.push_back(f);
    }
    if (d->n_fog > 0) H.fog_grid.assign(d->fog_grid, d->fog_grid + d->fog_grid_off[d->n_fog]);
    if (H.fogs.empty()) { FogD z; memset(&z, 0, sizeof z); H.fogs.push_back(z); H.fog_grid.push_back(0); }   // non-null tables; n_fog stays 0
}

// The scene's tables, step by step.  Every refusal comes before the first table is written; the steps after that cannot fail.
inline bool layout_scene(const gi_scene_desc* d, HostScene& H, std::string& err)
{
    std::vector<int32_t> order, rec_of;
    if (!validate_scene(d, err) || !number_scene_nodes(d, order, rec_of, err) || !validate_fog(d, err)) return false;
    const SceneMargins m = scene_margins(d);
    layout_tnodes(d, rec_of, H);
    layout_wide(d, H);                                                  // no wide records for a tree that is not made of exact octants
    layout_cboxes(d, H, nullptr, m.tight, H.cboxes, H.cuse);           // over the entities' exact boxes
    layout_entities(d, H);
    layout_leaf_tris(d, H);
    layout_leaf_boxes(d, m, H);
    layout_trace_boxes(d, m, H);
    layout_trace_cboxes(d, H);
    H.lights_clear = lights_are_clear(d, m);
    layout_materials(d, H);
    layout_lights(d, H);
    layout_textures(d, H);
    layout_fog(d, H);
    return true;
}

// ---- the photon octree.  Input: the reference's tree in pre-order (first child = n+1, each next child where the previous sub-tree
// ends).  Output: (1) photons re-ordered leaf by leaf in that DFS order; (2) node records where the 8 children of a node are
// consecutive, so the descent of PhotonMap::Node::getBounds indexes the child directly; (3) for every leaf the result of
// PhotonMap::Node::get(leaf box +- EPSILON) (include/photonMap.cpp:50-92) as a list of photon ranges -- the candidate set of a
// gather depends only on the leaf that contains the query point, so it is computed once per leaf here instead of per query.
inline bool validate_photon_tables(const gi_photon_map_desc* d, std::string& err)
{
    if (!d->photons || !d->node_bbox || !d->node_child || !d->node_off) { err = "photons: null tables"; return false; }
    const int nref = d->node_off[d->n_node];
    if (d->node_off[0] != 0 || nref < 0 || (nref && !d->node_idx)) { err = "photons: bad leaf table"; return false; }
    for (int r = 0; r < nref; r++)
        if (d->node_idx[r] < 0 || d->node_idx[r] >= d->n_photon) { err = "photons: leaf reference out of range"; return false; }
    return true;
}
// end[n] = the node after n's sub-tree in pre-order (the skip link of the candidate search): the max over the children, which come later
inline bool photon_subtree_ends(const gi_photon_map_desc* d, std::vector<int32_t>& end, std::string& err)
{
    const int N = d->n_node;
    end.assign((size_t)N, 0);
    for (int n = N - 1; n >= 0; n--) {
        end[n] = n + 1;
        for (int k = 0; k < 8; k++) {
            int ch = d->node_child[(size_t)n * 8 + k];
            if (ch == -1) continue;
            if (ch <= n || ch >= N) { err = "photons: child index is not a later pre-order node"; return false; }
            end[n] = std::max(end[n], end[ch]);
        }
    }
    return true;
}
// a node has eight children or none, each child begins where the one before it ends, and the leaves' photon ranges follow one another
inline bool validate_photon_order(const gi_photon_map_desc* d, const std::vector<int32_t>& end, std::string& err)
{
    for (int n = 0; n < d->n_node; n++) {
        if (d->node_off[n + 1] < d->node_off[n]) { err = "photons: leaf offsets not monotone"; return false; }
        if (!node_is_inner(d->node_child, n)) continue;
        if (d->node_child[(size_t)n * 8] == -1) { err = "photons: node with partial children"; return false; }
        int32_t expect = n + 1;
        for (int k = 0; k < 8; k++) {
            int ch = d->node_child[(size_t)n * 8 + k];
            if (ch != expect) { err = "photons: nodes are not in pre-order"; return false; }
            expect = end[ch];
        }
    }
    return true;
}
inline void layout_photons_by_leaf(const gi_photon_map_desc* d, HostPhotons& H)      // (1) photons in leaf (DFS) order
{
    const int nref = d->node_off[d->n_node];
    H.pos.resize((size_t)nref * 3);
    H.dircol.resize((size_t)nref * 6);
    for (int r = 0; r < nref; r++) {
        const double* p = d->photons + (size_t)d->node_idx[r] * 9;
        for (int k = 0; k < 3; k++) H.pos[(size_t)r * 3 + k] = p[k];
        for (int k = 0; k < 6; k++) H.dircol[(size_t)r * 6 + k] = p[3 + k];
    }
}
// (2) the record of inner node n: its box, child 7's lower corner, and the planes the 8 children's boxes are made of (include/photonMap.cpp:139-149).
// False unless every child's stored box equals, bit for bit, the box gather_find_leaf derives from them.
inline bool layout_inner_pnode(const gi_photon_map_desc* d, int n, const std::vector<int32_t>& rec_of, PNode& t)
{
    const int32_t* child = d->node_child + (size_t)n * 8;
    t.first_child = rec_of[child[0]];
    for (int ax = 0; ax < 3; ax++) {
        const double* high = node_box(d->node_bbox, child[1 << axis_slot_bit(ax)]);      // a child on the high side of this axis only
        t.mid[ax] = node_box(d->node_bbox, child[7])[ax];
        t.u.in.lo2[ax] = high[ax]; t.u.in.hi2[ax] = high[3 + ax];
    }
    bool planes_ok = true;
    for (int c = 0; c < 8; c++)
        for (int ax = 0; ax < 3; ax++) {
            const bool high = (c >> axis_slot_bit(ax)) & 1;
            const double wlo = c == 7 ? t.mid[ax] : (high ? t.u.in.lo2[ax] : t.bmin[ax]);
            const double whi = c == 7 ? t.bmax[ax] : (high ? t.u.in.hi2[ax] : t.mid[ax]);
            if (node_box(d->node_bbox, child[c])[ax] != wlo || node_box(d->node_bbox, child[c])[3 + ax] != whi) planes_ok = false;
        }
    return planes_ok;
}
// (3) the candidate ranges of leaf t: the reference's get() on the canonical tree, sub-trees skipped with `end`; neighbouring ranges are merged
inline void layout_leaf_candidates(const gi_photon_map_desc* d, const std::vector<int32_t>& end, PNode& t, std::vector<PRange>& ranges)
{
    double qlo[3], qhi[3];
    for (int k = 0; k < 3; k++) { qlo[k] = t.bmin[k] - GI_EPSILON; qhi[k] = t.bmax[k] + GI_EPSILON; }
    t.first_child = -1;
    t.nb_off = (int32_t)ranges.size();
    int total = 0;
    const bool any = !(qhi[0] - qlo[0] <= 0);                     // include/photonMap.cpp:73-74
    for (int m = 0; any && m < d->n_node;) {
        const double* b = node_box(d->node_bbox, m);
        // the root itself is not tested (PhotonMap::getInRange calls _root.get directly); include/bbox.h:33-38
        const bool take = m == 0 || ((b[0] <= qhi[0] && b[3] >= qlo[0]) && (b[1] <= qhi[1] && b[4] >= qlo[1]) && (b[2] <= qhi[2] && b[5] >= qlo[2]));
        if (take && node_is_inner(d->node_child, m)) { m = m + 1; continue; }
        const int first = d->node_off[m], count = take ? d->node_off[m + 1] - d->node_off[m] : 0;
        if (count > 0) {
            if ((int32_t)ranges.size() > t.nb_off && ranges.back().first + ranges.back().count == first) ranges.back().count += count;
            else { PRange rg; rg.first = first; rg.count = count; ranges.push_back(rg); }
            total += count;
        }
        m = end[m];
    }
    t.u.lf.nb_cnt = (int32_t)ranges.size() - t.nb_off;
    t.u.lf.nb_photons = total;
}
inline bool layout_photons(const gi_photon_map_desc* d, HostPhotons& H, std::string& err)
{
    H.nodes.clear(); H.ranges.clear(); H.pos.clear(); H.dircol.clear(); H.n_node = 0; H.n_photon = 0; H.planes_ok = true;
    if (d->n_node <= 0 || d->n_photon <= 0) return true;
    std::vector<int32_t> end, order, rec_of;
    if (!validate_photon_tables(d, err) || !photon_subtree_ends(d, end, err) || !validate_photon_order(d, end, err)) return false;
    layout_photons_by_leaf(d, H);
    // records with consecutive children: breadth-first numbering (after validate_photon_order no node is met twice)
    if (!number_breadth_first(d->node_child, d->n_node, [](int) { return true; }, order, rec_of) || (int)order.size() != d->n_node) { err = "photons: tree is not connected"; return false; }
    H.nodes.assign((size_t)d->n_node, PNode());
    for (int n = 0; n < d->n_node; n++) {
        PNode& t = H.nodes[(size_t)rec_of[n]];
        memset(&t, 0, sizeof t);
        for (int k = 0; k < 3; k++) { t.bmin[k] = node_box(d->node_bbox, n)[k]; t.bmax[k] = node_box(d->node_bbox, n)[3 + k]; }
        if (!node_is_inner(d->node_child, n)) layout_leaf_candidates(d, end, t, H.ranges);
        else if (!layout_inner_pnode(d, n, rec_of, t)) H.planes_ok = false;      // (gather_find_leaf then walks two records per level)
    }
    if (H.ranges.empty()) { PRange z; z.first = 0; z.count = 0; H.ranges.push_back(z); }
    H.n_node = d->n_node; H.n_photon = d->node_off[d->n_node];
    return true;
}

// ---- the thin lens (gi_hip.h: gi_set_lens).  What gi_set_lens accepts; the aperture polygon's vertices as the kernels read them; the checkpoint's tag.
#define GI_LENS_MIN_BLADES 3
#define GI_LENS_MAX_BLADES 16
inline bool lens_valid(const gi_lens* l)
{
    return l && std::isfinite(l->radius) && l->radius >= 0 && std::isfinite(l->rotation) && l->blades >= GI_LENS_MIN_BLADES && l->blades <= GI_LENS_MAX_BLADES && l->reserved == 0;
}
// xy [blades + 1][2]: v_k = (cos, sin)(rotation + (2 pi k) / blades) with the host's libm, the last a copy of the first
inline void lens_vertices(const gi_lens& l, double* xy)
{
    for (int k = 0; k < l.blades; k++) {
        const double th = l.rotation + (2.0 * GI_PI * k) / l.blades;
        xy[2 * k] = std::cos(th); xy[2 * k + 1] = std::sin(th);
    }
    xy[2 * l.blades] = xy[0]; xy[2 * l.blades + 1] = xy[1];
}
// 0 for a pinhole, else the low 32 bits of 64-bit FNV-1a over radius, rotation, blades, reserved as they lie in memory (24 bytes, little-endian), 0 -> 1
inline uint32_t lens_tag(const gi_lens& l)
{
    if (!(l.radius > 0)) return 0u;
    unsigned char b[24];
    static_assert(sizeof(gi_lens) == 24, "gi_lens is 24 bytes without padding");
    memcpy(b, &l, 24);
    uint64_t h = 0xcbf29ce484222325ull;
    for (int k = 0; k < 24; k++) { h ^= b[k]; h *= 0x100000001b3ull; }
    const uint32_t t = (uint32_t)h;
    return t ? t : 1u;
}

inline int local_rows(const gi_render_params* p)
{
    if (!p || p->stripe_h <= 0 || p->stripe_world <= 0 || p->height <= 0) return 0;
    int rows = 0;
    const int n_stripes = (p->height + p->stripe_h - 1) / p->stripe_h;
    for (int k = p->stripe_rank; k < n_stripes; k += p->stripe_world) rows += std::min(p->stripe_h, p->height - k * p->stripe_h);
    return rows;
}

// camera basis and frame constants, include/raytracer.h:74-78
inline bool make_frame(const gi_render_params* p, Frame& F, std::string& err)
{
    if (!p || p->width <= 0 || p->height <= 0 || p->stripe_h <= 0 || p->stripe_world <= 0 || p->stripe_rank < 0 || p->stripe_rank >= p->stripe_world ||
        p->min_samples < 0 || p->max_samples < 0) { err = "render: bad parameters"; return false; }
    V3 pos = ld3(p->cam_pos), up = ld3(p->cam_up), fwd = ld3(p->cam_forward);
    const int w = p->width, h = p->height;
    F.sw = (p->sensor_diag * w) / (std::sqrt((double)w * w + h * h));
    F.sh = F.sw * ((double)h / w);
    F.screen_center = pos + p->focal_dist * fwd;
    F.right = normalize(cross(fwd, up));
    F.cam_pos = pos; F.cam_up = up;
    F.w = w; F.h = h;
    F.he = make_halton_enum((unsigned)w, (unsigned)h);
    F.min_samples = p->min_samples; F.max_samples = p->max_samples; F.noise_thresh = p->noise_thresh;
    F.seed = p->seed;
    F.stripe_h = p->stripe_h; F.stripe_rank = p->stripe_rank; F.stripe_world = p->stripe_world;
    F.local_rows = local_rows(p);
    return true;
}

// ---- the pool budget of a fixed-spp call (gi_stream.inc: stream_samples): how many paths are in flight, P, and how many samples per pixel
// the radiance buffer takes at a time, chunk.  As many paths as fit -- the whole frame when HBM allows (1080p x 256 spp = 531 M paths = 123 GB
// of path records on a 288 GB part): more paths per pass are fewer passes and, above all, better-sorted (more coherent) queues.
// What a slot is budgeted, in bytes: the terms beside the record are kBudgetWorkBytes, which gi_stream.inc asserts to cover what its workspace
// table (kStreamWork) really allocates per slot.  The figure is somewhat larger than that table's (124 against 112 bytes), and P of
// the benchmark frame, which is bound by HBM, follows from it: changing a term changes that frame's speed.
constexpr size_t kPoolRecordBytes = 232;         // the field arrays of PathPool (gi_pool.h: GI_POOL_BYTES_PER_SLOT, asserted there)
constexpr size_t kBudgetSampleIdBytes = 8;       // the slot -> sample table
constexpr size_t kBudgetQueueBytes = 13 * 4;     // 13 queue / key words
constexpr size_t kBudgetSortBytes = 24;          // sort scratch
constexpr size_t kBudgetStagingBytes = 40;       // staging queues
constexpr size_t kBudgetWorkBytes = kBudgetSampleIdBytes + kBudgetQueueBytes + kBudgetSortBytes + kBudgetStagingBytes;
static_assert(kBudgetWorkBytes == 124, "the pool of the benchmark frame is sized with this figure");
struct PoolPlan { uint32_t P; int chunk; };
// free_b: free device memory, when mem_known (the query succeeded); held_b: what the context already holds of its workspaces and would re-use;
// n_deferred_lights: shadow queries (ShadowQ) per slot, 0 where the shade stage walks its shadow segments itself.  No HIP call: the CPU suite runs it.
inline PoolPlan plan_pool(bool mem_known, size_t free_b, size_t held_b, uint32_t n_pix, int spp, size_t pool_slots_max, size_t lbuf_bytes_max, int n_deferred_lights)
{
    size_t slots_budget = pool_slots_max;
    if (mem_known) {
        const size_t per_slot = kPoolRecordBytes + kBudgetWorkBytes + sizeof(ShadowQ) * (size_t)n_deferred_lights;
        const size_t lbuf = (size_t)n_pix * (size_t)std::min<size_t>((size_t)spp, lbuf_bytes_max / ((size_t)n_pix * 24)) * 24;
        const size_t avail = (size_t)((double)(free_b + held_b) * 0.90);
        if (avail > lbuf) slots_budget = std::min(slots_budget, (avail - lbuf) / per_slot);
        else slots_budget = std::min<size_t>(slots_budget, 1u << 20);
    }
    PoolPlan plan;
    plan.P = (uint32_t)std::max<size_t>(64, std::min<size_t>(std::min<size_t>(slots_budget, 0xfffffff0u), (size_t)n_pix * (size_t)spp));
    plan.chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)spp, lbuf_bytes_max / ((size_t)n_pix * 24)));
    return plan;
}

}  // namespace gi
