// gi_scene.h -- what every other part reads: the function markers (GI_HD, GI_HDM, GI_TOUCH, GI_UNROLL), the constants and the GI_FEAT_* bits,
// the device tables as they lie in HBM (gi_layout.h fills them), Scene, the jump grid's size and Counters.  No functions but the two
// feature-level selectors.  Needs <stdint.h> only.  Included by gi_device.h inside namespace gi, first.

#ifndef GI_HD
#define GI_HD __host__ __device__ __forceinline__
#endif
// keep a value alive without using it (a load issued early only to pull its cache line in)
#if defined(__HIP_DEVICE_COMPILE__)
#define GI_TOUCH(x) asm volatile("" ::"v"(x))
#else
#define GI_TOUCH(x) (void)(x)
#endif
#ifndef GI_HDM   // member functions
#define GI_HDM __host__ __device__ __forceinline__
#endif

// ------------------------------------------------------------------------------------------------ constants (include/util.h:14-31)
#if defined(__clang__)
#define GI_UNROLL _Pragma("unroll")
#else
#define GI_UNROLL
#endif
#define GI_EPSILON 0.00001
#define GI_SHADOW_BIAS 0.0001
#define GI_MIN_DEPTH 2
#define GI_MAX_DEPTH 64
#define GI_PI 3.14159265358979323846
#define GI_GATHER_K 32
#define GI_RAYMARCH_STEPSIZE 0.04
#define GI_FEAT_SPHERES 1   // template feature bits: code for entity kinds / media a scene does not contain is not compiled in
#define GI_FEAT_FOG 2
#define GI_FEAT_TEX 4       // checkerboard / image textures (include/material.h:32-81): uv carried through the walk, texture alpha in the alpha test
// The feature level a scene runs (scene_feat, after Scene) is one of four bit sets, not any of the eight: textures -> 7, else fog -> 3,
// else spheres -> GI_FEAT_SPHERES, else 0.  k_st_trace has no fog level (the medium is marched in the shade stage), so its level
// (scene_trace_feat) is textures -> 7, else spheres -> GI_FEAT_SPHERES, else 0.

// ------------------------------------------------------------------------------------------------ device tables (HBM layout)
struct NodeLink { int32_t hit, skip; };
struct alignas(128) TNode { // 128 B = one L2 line: a scene-octree node, stored once, nodes in breadth-first order (top levels first,
                            // so that a prefix of the array is what a kernel stages in LDS)
    double bmin[3], bmax[3];
    int32_t first_ref;      // leaves: first entry in leaf_refs
    int32_t n_ref;          // leaves: number of entries; inner nodes: -1
    int32_t leaf_id;        // canonical pre-order index (RNG key, same numbering as the CPU side)
    int32_t pad;
    NodeLink link[8];       // per direction octant: next node when the box is hit (inner nodes) / when the sub-tree is left;
                            // following them visits the children of every node front to back for that octant; END = n_node
};
// Wide node: one record per INNER node holding what the box tests of all its (up to 8) children need.  Octree::Node::partition
// (include/octree.cpp:318-328) builds the children's boxes from five planes per axis: children on the low side span [min, mid],
// children on the high side [min + .5 d, mid + .5 d], except child 7 which spans [mid, max] (mid = mix(min, max, .5); the three
// forms of "the middle" and of "the far side" differ in the last bit).  The record keeps those planes exactly as the children's
// boxes hold them (checked bit for bit when the scene is laid out; a tree of another shape keeps the per-node walk), so one record
// and 36 multiply-subtracts replace eight records and 96.  pl[axis] = {min, mid, lo2, hi2, max, mid}: the pairs (0,1), (2,3),
// (5,4) are the low-side, high-side and child-7 intervals, and a ray that runs backwards along the axis reads every pair in the
// opposite order (entry plane first) by xor-ing 8 into the byte offset -- the swap of include/bbox.h:52-57 costs no instruction.
struct alignas(32) WNode {  // 224 B
    double pl[3][6];        // x, y, z
    int32_t ca[8], cb[8];   // child slot c (x = bit 0, z = bit 1, y = bit 2): cb < 0: inner, wide record ca; cb > 0: leaf, its references
                            // are leaf_tris[ca .. ca + cb); cb == 0: no such child (or an empty leaf)
    int32_t parent;         // wide record of the parent, -1 at the root
    uint32_t exists;        // bit c: child slot c is an inner node or a non-empty leaf
    int32_t pad[2];
};
struct TriGeom {            // 80 B: what a ray-triangle test needs
    double p0[3], e1[3], e2[3];
    int32_t mat;
    uint32_t flags;         // bit0: interpolate vertex normals; bit1: alpha test always passes (opacity >= 1 or IOR != 1);
                            // bit2: analytic sphere (p0 = centre, e1[0] = radius)
};
struct LeafTri {            // 80 B: the test record again, stored once per leaf reference in leaf order, so that a leaf's triangles
    double p0[3], e1[3], e2[3];   // are consecutive in memory and no index has to be chased before the vertex data can be fetched
    int32_t tri;            // triangle index (shading record, RNG key)
    uint32_t matflags;      // material << 3 | flags
};
struct TriShade { double n0[3], n1[3], n2[3], fnorm[3]; };  // 96 B, read once per shaded hit
struct TriUV { double t0[2], t1[2], t2[2]; };                // 48 B: vertex texCoords, read only by textured scenes (GI_FEAT_TEX)
struct Mat { double roughness, opacity, ior, diffuse[3], emissive[3]; int32_t dtex, etex; };   // dtex / etex: texture record or -1 = the constant colour
struct TexD {               // include/material.h:10-81
    int32_t kind;           // 0 texture(col), 1 checkerboard, 2 imageTexture
    int32_t w, h, has_alpha;
    double a[3], b[3];      // colour; checkerboard colours a, b
    double tiles, tile_u, tile_v;
    unsigned long long pix; // first byte of the image in Scene::tex_pixels (RGBA8, rows top to bottom)
};
struct LightD { double pos[3], col[3], rad, dir[3], angle; };
struct alignas(128) PNode { // 128 B: photon octree node; the 8 children of a node are 8 consecutive records
    double bmin[3], bmax[3];// node box: PhotonMap::Node::getBounds checks contains() at every level
    double mid[3];          // inner nodes: lower corner of child 7 = the split point the reference computes
    int32_t first_child;    // record index of child 0, or -1 for a leaf
    int32_t nb_off;         // leaves: candidate photon ranges [nb_off, nb_off + nb_cnt) in Scene::pranges
    union {
        struct { int32_t nb_cnt, nb_photons, pad[10]; } lf;   // leaves: nb_photons = total photons in those ranges (= what getInRange returns here)
        struct { double lo2[3], hi2[3]; } in;                 // inner nodes: the high-side children span [lo2, hi2] (= [min + .5 d, mid + .5 d],
    } u;                                                      // include/photonMap.cpp:139-149), child 7 [mid, max], low-side children [min, mid]
};
struct PDescent { double mid[3]; int32_t first_child, pad; };   // what the descent of getBounds decides by; the boxes it checks stay in PNode
struct PRange { int32_t first, count; };   // photons are stored leaf by leaf in the reference's DFS order
struct HaltonDim { uint32_t P, n, off; float scale; uint32_t mlo, mhi, pad[2]; };   // (mhi:mlo) = floor((2^64 - 1) / P) + 1: x / P = hi64(x * m) for every 32-bit x
struct FogD { double pos[3], size[3], col[3], d, sc, bmin[3], bmax[3]; int32_t grid_off, grid_n; };   // HeightFog, include/atmosphere.h:30-83

struct Scene {
    const TNode* tnodes;      // [n_node]
    const WNode* wnodes;      // [n_wnode] inner nodes, breadth first; null when the tree is not made of exact octants
    const int32_t* wleaf_id;  // [n_wnode][8] canonical node index of a leaf child (RNG key of the alpha test)
    const float* cboxes;      // [n_wnode][8][6] content box of every child's sub-tree (all entities referenced below it), rounded outwards; null = no culling
    const uint32_t* cuse;     // [n_wnode] children (slot bits) whose content box is worth testing (clearly smaller than their octant)
    const double* shadow_boxes;   // boxes for segments that END AT A LIGHT (k_st_shadow): trace_boxes when no entity comes near a light (visible_leaf_blocks), else leaf_boxes
    const float* scboxes;     // and the content boxes that go with them (= tcboxes / tcuse, or cboxes / cuse)
    const uint32_t* scuse;
    const float* tcboxes;     // the same two tables made of trace_boxes, for the streaming closest-hit walk (k_st_trace); = cboxes / cuse where nothing is cut to its leaf
    const uint32_t* tcuse;
    const int32_t* leaf_refs;
    const LeafTri* leaf_tris; // [n_refs], parallel to leaf_refs
    const double* leaf_boxes; // [n_refs][6] every reference's own box (min xyz, max xyz, widened): a ray that misses it cannot hit the entity; null = not used
    const double* trace_boxes;// [n_refs][6] the same for the closest-hit walk: where the rules of trace_wide_over allow it, the part of the entity inside its leaf; null with leaf_boxes
    const TriGeom* tris;
    const TriShade* shade;
    const TriUV* tri_uv;      // [n_tri], only when n_tex > 0
    const Mat* mats;
    const LightD* lights;
    const PNode* pnodes;
    const struct PDescent* pdescent;   // [n_pnode] split point and first child only (32 B: the whole table stays in L2), for gather_find_leaf_fast; null = not used
    const int32_t* pleaf_rank;   // [n_pnode] rank of a leaf among the leaves with candidate photons (the gather queries' sort key), -1 for every other node
    const int32_t* prank_leaf;   // [n_pleaf] its inverse
    int32_t n_pleaf;             // leaves with candidates
    const uint32_t* pcand_off;   // [n_pleaf + 1] where the candidate list of the leaf of that rank begins in pcand; null = not used
    const double* pcand;         // [total][3] the candidates' POSITIONS: the ranges of every such leaf written out back to back, in the order gather_in_leaf visits them (k_st_gather)
    const double* pcand_dc;      // [total][6] and their direction and colour (read by the second pass)
    const PRange* pranges;
    const double* ph_pos;     // [n_photon][3] leaf order
    const double* ph_dircol;  // [n_photon][6] leaf order
    const FogD* fogs;
    const double* fog_grid;
    const TexD* texs;
    const unsigned char* tex_pixels;
    const double* tex_lut;    // [256] pow(k / 255.0, 1.0 / (1.0 / GAMMA)) as the host libm computes it = imageTexture::get's gamma()
    int32_t n_tex;            // > 0: the scene has a non-constant texture (kernels instantiated with GI_FEAT_TEX)
    const HaltonDim* hdims;   // [256]
    const uint16_t* htable;
    int32_t n_node, n_tri, n_light, n_pnode, n_photon;
    int32_t n_wnode;
    int32_t pn_planes;        // photon octree: every inner record carries its children's planes (gather_find_leaf)
    int32_t has_spheres;      // 0: triangles only
    int32_t n_fog;
    double ambient[3];
    double root_bmin[3], root_bmax[3];   // box of octree node 0 (kernel argument: no memory round trip before a walk starts)
    double pmap_bmin[3], pmap_bmax[3];   // box of the photon map's root (gather_find_leaf_fast)
    const int32_t* pjump;     // [N][N][N] (y, z, x; N = GI_PJUMP_N) the node the descent of a position in that cell of the map's box has reached after GI_PJUMP_BITS levels (or its leaf); null = not used
    double pjump_cell[3], pjump_inv[3];   // a cell's size per axis and its inverse
    double cut_margin;        // >= 0: a closest-hit walk looks no further than its best hit plus this (trace_wide_step, cut_behind_hit); < 0: it walks on as the reference does
    // the thin lens (gi_set_lens; an addition).  The context's, not the scene's: uploads leave these three alone.  lens_radius == 0: a pinhole
    const double* lens_verts; // [lens_blades + 1][2] the aperture polygon's unit vertices, the last a copy of the first (gi_lens_vertices, host libm)
    double lens_radius;
    int32_t lens_blades;
};
// the feature levels of the GI_FEAT_* bits
inline int scene_feat(const Scene& S) { return S.n_tex > 0 ? 7 : (S.n_fog > 0 ? 3 : (S.has_spheres ? GI_FEAT_SPHERES : 0)); }
inline int scene_trace_feat(const Scene& S) { return S.n_tex > 0 ? 7 : (S.has_spheres ? GI_FEAT_SPHERES : 0); }

#ifndef GI_PJUMP_BITS
#define GI_PJUMP_BITS 7          // levels of the photon octree the jump table of gather_find_leaf_fast covers: a grid of 128^3 cells, 8 MB (5: 22.3 ms of queue compaction + gather keys on the benchmark, 6: 21.1, 7: 19.9)
#endif
#define GI_PJUMP_N (1 << GI_PJUMP_BITS)
struct Counters { unsigned long long v_trace, v_shadow, tri, shaded, pcand, traces, shadows, gathers; };
