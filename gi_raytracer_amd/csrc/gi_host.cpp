// gi_host.cpp -- host-side feeders of the hot path: the gih_* C ABI of gi_host.h over .scn/.obj/PNG ingestion, the scene and photon octree builders
// and their flattening into the tables of include/gi_hip.h.  One translation unit of plain C++17, pieces included in order: gi_host_geom.inc (geometry),
// gi_host_png.inc (PNG decoder), gi_host_tree.inc (octree tables, the one partition, its two rules), gi_host_scene.inc (the parts of a gih_scene,
// Octree::rebuild, loaders).  Host code as in the reference; its trees node for node (tests/test_host_builders.py compares them with the reference's dumps).
#include "gi_host.h"

#include <zlib.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace {
#include "gi_host_geom.inc"
#include "gi_host_png.inc"
#include "gi_host_tree.inc"
#include "gi_host_scene.inc"
}  // namespace

struct gih_scene : Scene {};   // the handle of gi_host.h: the aggregate of gi_host_scene.inc under its global name

extern "C" {

gih_scene* gih_scene_create(void) { return new gih_scene(); }
void gih_scene_destroy(gih_scene* s) { delete s; }
const char* gih_last_error(const gih_scene* s) { return s ? s->err.c_str() : "null scene"; }

int gih_load_scn(gih_scene* s, const char* path) { return s && path ? load_scn(*s, path) : -1; }

int gih_load_obj(gih_scene* s, const char* path, const double* pos3, const double* rot3, int32_t mat_idx)
{
    if (!s || !path || !pos3 || !rot3) return -1;
    if (!mat_in_range(*s, mat_idx, "load_obj")) return -2;
    return load_obj(s->ent, path, d3(pos3), d3(rot3), mat_idx);
}

int gih_add_material(gih_scene* s, const double* m) { return s && m ? s->mat.add_material(m) : -1; }
int gih_add_texture(gih_scene* s, int32_t kind, const double* params8, const uint8_t* rgba, int64_t n_bytes) { return s ? s->mat.add_texture(kind, params8, rgba, n_bytes) : -1; }
int gih_add_material_tex(gih_scene* s, int32_t dif, int32_t em, double roughness, double opacity, double ior) { return s ? s->mat.add_material_tex(dif, em, roughness, opacity, ior) : -1; }

int gih_load_png(const char* path, int32_t* width, int32_t* height, int32_t* has_alpha, uint8_t** rgba_out, char* errbuf, int32_t err_len)
{
    if (!path || !width || !height || !has_alpha || !rgba_out) return -1;
    int w = 0, h = 0; bool a = false;
    std::vector<uint8_t> px;
    std::string err;
    if (!decode_png(path, w, h, a, px, err)) {
        if (errbuf && err_len > 0) { strncpy(errbuf, err.c_str(), (size_t)err_len - 1); errbuf[err_len - 1] = 0; }
        return -2;
    }
    *width = w; *height = h; *has_alpha = a ? 1 : 0;
    *rgba_out = (uint8_t*)malloc(px.size());
    if (!*rgba_out) return -3;
    memcpy(*rgba_out, px.data(), px.size());
    return 0;
}
void gih_free(void* p) { free(p); }

int gih_add_triangles(gih_scene* s, int32_t n, const double* pos, const double* nrm, const double* uv, const int32_t* mat_idx)
{
    if (!s || n < 0 || (n && (!pos || !mat_idx))) return -1;
    for (int i = 0; i < n; i++) {
        if (!mat_in_range(*s, mat_idx[i], "add_triangles")) return -2;
        D3 p[3], nn[3];
        double t[6] = {0, 0, 0, 0, 0, 0};
        for (int k = 0; k < 3; k++) {
            p[k] = d3(pos + (size_t)i * 9 + k * 3);
            nn[k] = nrm ? d3(nrm + (size_t)i * 9 + k * 3) : mk(0, 0, 0);
        }
        if (uv) for (int k = 0; k < 6; k++) t[k] = uv[(size_t)i * 6 + k];
        s->ent.push_triangle(p, nn, t, mat_idx[i]);
    }
    return 0;
}

int gih_add_sphere(gih_scene* s, const double* centre3, double radius, int32_t mat_idx)
{
    if (!s || !centre3) return -1;
    if (!mat_in_range(*s, mat_idx, "add_sphere")) return -2;
    s->ent.push_sphere(d3(centre3), radius, mat_idx);
    return 0;
}

int gih_add_height_fog(gih_scene* s, const double* params12, const double* grid, int32_t n_grid, uint64_t seed) { return s && params12 ? s->env.add_height_fog(params12, grid, n_grid, seed) : -1; }
int gih_add_height_fog_grid(gih_scene* s, const double* params12, const double* grid, int32_t n_grid) { return s && params12 && grid && n_grid > 0 ? s->env.add_height_fog(params12, grid, n_grid, 0, true) : -1; }

int gih_add_light(gih_scene* s, const double* pos3, const double* col3, double rad)
{
    if (!s || !pos3 || !col3) return -1;
    s->env.add_light(pos3, col3, rad);
    return 0;
}
int gih_set_ambient(gih_scene* s, const double* rgb)
{
    if (!s || !rgb) return -1;
    for (int k = 0; k < 3; k++) s->env.st.ambient[k] = rgb[k];
    return 0;
}
int gih_get_settings(const gih_scene* s, gih_settings* out)
{
    if (!s || !out) return -1;
    *out = s->env.st;
    return 0;
}
int gih_set_camera(gih_scene* s, const double* pos3, const double* look_at3)
{
    if (!s || !pos3 || !look_at3) return -1;
    s->env.set_camera(pos3, look_at3);
    return 0;
}

int gih_build_octree(gih_scene* s)
{
    if (!s) return -1;
    if (s->mat.mats.empty()) { s->err = "build_octree: no materials"; return -2; }
    build_octree(*s);
    return 0;
}

int gih_get_scene_desc(const gih_scene* s, gi_scene_desc* d)   // gi_scene_desc keeps its tri_* field names: they are ABI
{
    if (!s || !d) return -1;
    if (!s->tree_valid) return -4;
    const Entities& e = s->ent; const Materials& m = s->mat; const Environment& v = s->env; const OctreeTables& t = s->tree.t;
    memset(d, 0, sizeof *d);
    d->n_tri = e.n_ent();
    d->tri_pos = e.pos.data(); d->tri_nrm = e.nrm.data(); d->tri_uv = e.uv.data(); d->tri_mat = e.mat.data();
    d->n_mat = m.n_mat(); d->mats = m.mats.data();
    d->n_light = (int32_t)(v.lights.size() / 11); d->lights = v.lights.data();
    for (int k = 0; k < 3; k++) d->ambient[k] = v.st.ambient[k];
    d->n_node = t.n_nodes();
    d->node_bbox = t.bbox.data(); d->node_child = t.child.data(); d->node_ent_off = t.off.data(); d->node_ent_idx = t.idx.data();
    d->ent_kind = e.kind.data();
    d->n_fog = (int32_t)(v.fog.size() / 12);
    d->fog = v.fog.data(); d->fog_grid_off = v.fog_grid_off.data(); d->fog_grid = v.fog_grid.data();
    if (m.textured()) {   // constant-colour scenes stay in the plain form (n_tex = 0)
        if (m.mat_tex.size() != (size_t)d->n_mat * 2) return -4;   // a material added as plain colours next to textured ones
        d->n_tex = (int32_t)m.tex_kind.size();
        d->tex_kind = m.tex_kind.data(); d->tex_param = m.tex_param.data(); d->mat_tex = m.mat_tex.data();
        d->tex_pixels = m.tex_pixels.data(); d->n_tex_pixel_bytes = (int64_t)m.tex_pixels.size();
    }
    return 0;
}

int gih_counts(const gih_scene* s, int32_t* n_tri, int32_t* n_mat, int32_t* n_light, int32_t* n_node, int32_t* n_ref)
{
    if (!s) return -1;
    if (n_tri) *n_tri = s->ent.n_ent();
    if (n_mat) *n_mat = s->mat.n_mat();
    if (n_light) *n_light = (int32_t)(s->env.lights.size() / 11);
    if (n_node) *n_node = s->tree.t.n_nodes();
    if (n_ref) *n_ref = (int32_t)s->tree.t.idx.size();
    return 0;
}

int gih_build_photon_map(gih_scene* s, int32_t n, const double* photons)
{
    if (!s || n < 0 || (n && !photons)) return -1;
    if (!s->tree_valid) { s->err = "build_photon_map: build the scene octree first (the map lives in the scene's root box)"; return -4; }
    s->pm.build(s->tree.root_box, n, photons);
    return 0;
}
int gih_build_photon_map_in_box(gih_scene* s, const double* box6, int32_t n, const double* photons)   // leaves the scene tree's part alone
{
    if (!s || !box6 || n < 0 || (n && !photons)) return -1;
    s->pm.build(load_box(box6), n, photons);
    return 0;
}
int gih_get_photon_desc(const gih_scene* s, gi_photon_map_desc* d)
{
    if (!s || !d) return -1;
    const OctreeTables& t = s->pm.t;
    memset(d, 0, sizeof *d);
    d->n_photon = (int32_t)(s->pm.photons.size() / 9);
    d->photons = s->pm.photons.data();
    d->n_node = t.n_nodes();
    d->node_bbox = t.bbox.data(); d->node_child = t.child.data(); d->node_off = t.off.data(); d->node_idx = t.idx.data();
    return 0;
}

// ---- single-object forms of what the tree builder and the loader do, for the C++ entity classes (include/gi/entities.h, atmosphere.h)
int gih_entity_bbox(int32_t kind, const double* pos9, double* out6)
{
    if (!pos9 || !out6 || (kind != 0 && kind != 1)) return -1;
    store_box(entity_box(kind, pos9), out6);
    return 0;
}
int gih_entity_overlaps_box(int32_t kind, const double* pos9, const double* box6)
{
    if (!pos9 || !box6 || (kind != 0 && kind != 1)) return -1;
    return entity_in_cell(kind, pos9, load_box(box6)) ? 1 : 0;
}
int gih_box_mesh(const double* pos3, const double* size3, const double* rot3, double* out108)
{
    if (!pos3 || !size3 || !rot3 || !out108) return -1;
    box_mesh(d3(pos3), d3(size3), d3(rot3), out108);
    return 12;
}
int gih_fog_grid(const double* params12, uint64_t seed, double* grid, int32_t n_grid)
{
    if (!params12) return -1;
    const int n = fog_grid_size(params12);
    if (n <= 0 || (grid && n_grid != n)) return -2;
    if (grid) fog_noise(seed, 0, n, grid);
    return n;
}

// gamma(color, 2.2), glm::clamp(color, 0, 1), Image::setPixel's (int)(255 c) (include/raytracer.h:150-157, include/util.h:94-97, include/image.h:14-16).
// pow of a negative channel is NaN, which the reference's clamp lets through and its cast turns into 0 (known answers: tests/golden/kat.npz kat_pixel).
int gih_to_rgb8(const void* lin, int32_t is_f64, int64_t n_values, uint8_t* out)
{
    if (n_values < 0 || (n_values && (!lin || !out))) return -1;
    for (int64_t i = 0; i < n_values; i++) {
        const double c = is_f64 ? static_cast<const double*>(lin)[i] : (double)static_cast<const float*>(lin)[i];
        const double g = std::pow(c, 1.0 / 2.2);
        out[i] = g != g ? (uint8_t)0 : (uint8_t)(int)(255 * std::min(std::max(g, 0.0), 1.0));
    }
    return 0;
}

}  // extern "C"
