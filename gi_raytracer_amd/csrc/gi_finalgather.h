// gi_finalgather.h -- the per-lane functions of the final-gather pass (gi_render_final_gather_*; include/gi_hip.h states the definition) that need
// no walk: what a gather ray brings back given its hit's values and the direct light there (fg_secondary), the fold over a sample's rays (fg_add,
// fg_mean) and the codes of the ids tap.  Needs gi_baked.h (grid_irradiance, cube_texel) behind gi_math.h.  Included by gi_finalgather.inc inside
// namespace gi; tests/cpp/finalgather_lookup.cpp compiles it for the host.  Everything is IEEE + - * / and compares only (the grid's look-up and the
// cube's texel are gi_baked.h's), in the header's order, so that with -ffp-contract=off every value equals the tests' numpy statement
// (tests/finalgather_expect.py) bit for bit.

#define GI_FG_MAX_DIRS 64
#define GI_FG_ID_MISS (-1)      // ids: the gather ray left the scene
#define GI_FG_ID_NONE (-2)      // ids: no gather for this sample (the first hit missed or is not on the diffuse lobe, or GI_BAKED_DIFFUSE is clear)

// the baked data a secondary hit reads: the plain grid and one chain (no atlas, no visibility maps, no probe set)
struct FgLook {
    const double* sh;               // [nz][ny][nx][9][3], never null (the gather needs GI_BAKED_DIFFUSE, which needs the grid)
    const int32_t* n3;              // nx, ny, nz
    const double *gmin, *gmax;
    const double* chain;            // the whole chain [texels][3], or null: a specular secondary hit then reads nothing
    const int32_t* level_of_mat;    // [n_mat], with a chain
    uint32_t face;
    const uint32_t* level_off;      // texels before level l
};
// a secondary hit's values: Q, the unit shading normal turned against the gather ray, the material's colours (textures applied), its roughness and index
struct FgHit { V3 Q, nf, color, emissive; double roughness; int32_t mat; };

// the entry of the ids tap for a gather ray
GI_HD int32_t fg_id(bool hit, int32_t ent) { return hit ? ent : GI_FG_ID_MISS; }

// L_j of a gather ray of direction d that hit q, with i = lit_direct at the hit: base = emissive + color * i; a diffuse-lobe hit (roughness >= .9)
// returns base + color * grid_irradiance(Q, Nf); a mirror or glossy one with a chain base + color * chain[level][cube_texel(reflect(d, Nf))],
// level 0 for a mirror (roughness < .001), else the material's; without a chain base itself
GI_HD V3 fg_secondary(const FgLook& A, const FgHit& q, V3 d, V3 i)
{
    const V3 base = q.emissive + q.color * i;
    if (!(q.roughness < .9)) return base + q.color * grid_irradiance(A.sh, A.n3, A.gmin, A.gmax, q.Q, q.nf);
    if (!A.chain) return base;
    const uint32_t l = q.roughness < .001 ? 0u : (uint32_t)A.level_of_mat[q.mat];
    const size_t t = (size_t)A.level_off[l] + cube_texel(reflect(d, q.nf), A.face >> l);
    return base + q.color * ld3(A.chain + t * 3);
}
// the fold over j: acc starts at +0.0 and takes L_0, L_1, ... in ascending j; E = acc / (double) n_dirs; the sample's diffuse term is color * E
GI_HD V3 fg_add(V3 acc, V3 L) { return acc + L; }
GI_HD V3 fg_mean(V3 acc, int32_t n_dirs) { return acc / (double)n_dirs; }
GI_HD V3 fg_diffuse(V3 color, V3 acc, int32_t n_dirs) { return color * fg_mean(acc, n_dirs); }
