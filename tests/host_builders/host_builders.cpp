// host_builders.cpp -- the host builders (gi_raytracer_amd/csrc/gi_host.cpp, compiled into this program) driven through the gih_* C API under
// the address and undefined-behaviour sanitizers (tests/test_host_builders.py builds and runs it): every scene file, both tree builders, both
// descriptors read to their last element, the single-object entries, and the loaders' refusals.
// usage: host_builders <repository root> <scratch directory> <scene.scn relative to the root>...
#include "../../gi_raytracer_amd/csrc/gi_host.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); exit(1); } } while (0)

static double g_sink = 0;   // every table value is added here, so that every element is read
template <class T> static void read_all(const T* p, long long n) { for (long long i = 0; i < n; i++) g_sink += (double)p[i]; }

static uint64_t g_rng = 0x2545F4914F6CDD1Dull;
static double rnd() { g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull; return (double)(g_rng >> 11) * (1.0 / 9007199254740992.0); }

static std::vector<double> photons_in(const double* box6, int n)
{
    std::vector<double> ph((size_t)n * 9);
    for (int i = 0; i < n; i++)
        for (int k = 0; k < 9; k++) ph[(size_t)i * 9 + k] = k < 3 ? box6[k] + rnd() * (box6[k + 3] - box6[k]) : rnd();
    return ph;
}

static void read_photon_desc(const gih_scene* s, int n, const double* box6)
{
    gi_photon_map_desc p;
    CHECK(gih_get_photon_desc(s, &p) == 0 && p.n_photon == n && p.n_node >= 1);
    CHECK(memcmp(p.node_bbox, box6, 6 * sizeof(double)) == 0);
    read_all(p.photons, (long long)n * 9); read_all(p.node_bbox, (long long)p.n_node * 6); read_all(p.node_child, (long long)p.n_node * 8);
    read_all(p.node_off, p.n_node + 1); read_all(p.node_idx, p.node_off[p.n_node]);
}

static void whole_scene(const std::string& path)
{
    gih_scene* s = gih_scene_create();
    CHECK(s && gih_load_scn(s, path.c_str()) == 0);
    gi_scene_desc d;
    CHECK(gih_get_scene_desc(s, &d) == -4 && gih_build_photon_map(s, 0, nullptr) == -4);   // no tree yet
    CHECK(gih_build_octree(s) == 0 && gih_get_scene_desc(s, &d) == 0 && d.n_tri > 0 && d.n_node >= 1);
    int32_t n_tri, n_mat, n_light, n_node, n_ref;
    CHECK(gih_counts(s, &n_tri, &n_mat, &n_light, &n_node, &n_ref) == 0 && n_tri == d.n_tri && n_mat == d.n_mat && n_light == d.n_light && n_node == d.n_node);
    CHECK(n_ref == d.node_ent_off[d.n_node]);
    read_all(d.tri_pos, (long long)d.n_tri * 9); read_all(d.tri_nrm, (long long)d.n_tri * 9); read_all(d.tri_uv, (long long)d.n_tri * 6);
    read_all(d.tri_mat, d.n_tri); read_all(d.ent_kind, d.n_tri); read_all(d.mats, (long long)d.n_mat * 9); read_all(d.lights, (long long)d.n_light * 11);
    read_all(d.node_bbox, (long long)d.n_node * 6); read_all(d.node_child, (long long)d.n_node * 8); read_all(d.node_ent_off, d.n_node + 1); read_all(d.node_ent_idx, n_ref);
    read_all(d.fog, (long long)d.n_fog * 12); read_all(d.fog_grid_off, d.n_fog + 1); read_all(d.fog_grid, d.fog_grid_off[d.n_fog]);
    read_all(d.tex_kind, d.n_tex); read_all(d.tex_param, (long long)d.n_tex * 8); read_all(d.tex_pixels, d.n_tex_pixel_bytes);
    if (d.n_tex) read_all(d.mat_tex, (long long)d.n_mat * 2);
    gih_settings st;
    CHECK(gih_get_settings(s, &st) == 0 && st.max_samples >= st.min_samples);
    double root[6];
    memcpy(root, d.node_bbox, sizeof root);
    const std::vector<double> ph = photons_in(root, 3000);
    CHECK(gih_build_photon_map(s, 3000, ph.data()) == 0);
    read_photon_desc(s, 3000, root);
    const double other[6] = {root[0] - 1, root[1] - .5, root[2] - 2, root[3] + .25, root[4] + 3, root[5] + 1};
    CHECK(gih_build_photon_map_in_box(s, other, 1500, ph.data()) == 0);
    read_photon_desc(s, 1500, other);
    CHECK(gih_build_photon_map(s, 0, nullptr) == 0);   // back in the scene's own root box, and empty
    read_photon_desc(s, 0, root);
    CHECK(gih_get_scene_desc(s, &d) == 0 && memcmp(d.node_bbox, root, sizeof root) == 0);
    gih_scene_destroy(s);
    printf("%s: %d entities, %d nodes, %d references\n", path.c_str(), n_tri, n_node, n_ref);
}

static void single_objects()
{
    for (int i = 0; i < 200; i++) {
        double pos[9], box[6], out[6], mesh[108];
        for (double& v : pos) v = 4 * rnd() - 2;
        pos[3] = rnd();
        for (int k = 0; k < 3; k++) { box[k] = 4 * rnd() - 2; box[k + 3] = box[k] + 2 * rnd(); }
        for (int kind = 0; kind < 2; kind++) {
            CHECK(gih_entity_bbox(kind, pos, out) == 0 && out[0] <= out[3] && out[1] <= out[4] && out[2] <= out[5]);
            const int hit = gih_entity_overlaps_box(kind, pos, box);
            CHECK(hit == 0 || hit == 1);
        }
        CHECK(gih_box_mesh(pos, pos + 3, pos + 6, mesh) == 12);
        read_all(mesh, 108);
    }
    double out[6];
    const double pos[9] = {0, 0, 0, 1, 0, 0, 0, 1, 0};
    CHECK(gih_entity_bbox(2, pos, out) == -1 && gih_entity_overlaps_box(0, pos, nullptr) == -1 && gih_box_mesh(pos, pos, pos, nullptr) == -1);
    const double fog[12] = {0, 0, 0, 1, 2, 1, 1, 1, 1, .5, .25, 2};
    const int n = gih_fog_grid(fog, 7, nullptr, 0);
    CHECK(n == 2 * 3 * 2 * 8);
    std::vector<double> grid((size_t)n);
    CHECK(gih_fog_grid(fog, 7, grid.data(), n) == n && gih_fog_grid(fog, 7, grid.data(), n - 1) == -2 && gih_fog_grid(nullptr, 7, nullptr, 0) == -1);
    read_all(grid.data(), n);
    const double flat[12] = {0, 0, 0, 1, 2, 1, 1, 1, 1, .5, .25, 0};   // noise scale 0: no grid
    CHECK(gih_fog_grid(flat, 7, nullptr, 0) == -2);
}

static std::string write_file(const std::string& dir, const char* name, const char* text)
{
    const std::string path = dir + "/" + name;
    FILE* f = fopen(path.c_str(), "w");
    CHECK(f);
    fputs(text, f);
    fclose(f);
    return path;
}

// loads `text` as a scene file into a fresh scene, expects return code rc and, where `what` is given, that text in the error
static void scn_gives(const std::string& dir, const char* text, int rc, const char* what, int n_tri_after = -1)
{
    const std::string path = write_file(dir, "case.scn", text);
    gih_scene* s = gih_scene_create();
    const int got = gih_load_scn(s, path.c_str());
    if (got != rc || (what && !strstr(gih_last_error(s), what))) { fprintf(stderr, "scene\n%sgave %d \"%s\", expected %d \"%s\"\n", text, got, gih_last_error(s), rc, what ? what : ""); exit(1); }
    int32_t n_tri = 0;
    CHECK(gih_counts(s, &n_tri, nullptr, nullptr, nullptr, nullptr) == 0 && (n_tri_after < 0 || n_tri == n_tri_after));
    gih_scene_destroy(s);
}

static void error_paths(const std::string& dir)
{
    CHECK(gih_last_error(nullptr) && gih_load_scn(nullptr, "x") == -1);
    gih_scene* s = gih_scene_create();
    CHECK(gih_load_scn(s, (dir + "/missing.scn").c_str()) == -1 && strstr(gih_last_error(s), "cannot open scene file"));
    CHECK(gih_build_octree(s) == -2 && strstr(gih_last_error(s), "no materials"));
    const double zero[3] = {0, 0, 0}, mat[9] = {1, 1, 1, 1, 1, 1, 0, 0, 0};
    CHECK(gih_load_obj(s, (dir + "/missing.obj").c_str(), zero, zero, 0) == -2 && strstr(gih_last_error(s), "load_obj: material index out of range"));
    CHECK(gih_add_material(s, mat) == 0);
    CHECK(gih_load_obj(s, (dir + "/missing.obj").c_str(), zero, zero, 0) == 1);   // a missing mesh file is skipped
    const char* head = "v 0 0 0\nv 1 0 0\nv 0 0 1\nvt 0 0\nvn 0 1 0\nf 1/1/1 2/1/1 3/1/1\n";
    const std::string few = write_file(dir, "few.obj", (std::string(head) + "f 1/1/1 2/1/1\n").c_str());
    const std::string far = write_file(dir, "far.obj", (std::string(head) + "f 1/1/1 2/1/1 9/1/1\n").c_str());
    const std::string zer = write_file(dir, "zero.obj", (std::string(head) + "f 1/1/1 2/1/1 0/1/1\n").c_str());
    int32_t n_tri = 0;
    CHECK(gih_load_obj(s, few.c_str(), zero, zero, 0) == 2 && gih_load_obj(s, far.c_str(), zero, zero, 0) == 2 && gih_load_obj(s, zer.c_str(), zero, zero, 0) == 2);
    CHECK(gih_counts(s, &n_tri, nullptr, nullptr, nullptr, nullptr) == 0 && n_tri == 3);   // the good face of each file stays
    const int32_t bad_mat = 1;
    const double tri[9] = {0, 0, 0, 1, 0, 0, 0, 0, 1};
    CHECK(gih_add_triangles(s, 1, tri, nullptr, nullptr, &bad_mat) == -2 && strstr(gih_last_error(s), "add_triangles: material index out of range"));
    CHECK(gih_add_sphere(s, zero, 1, -1) == -2 && strstr(gih_last_error(s), "add_sphere: material index out of range"));
    const double fog[12] = {0, 0, 0, 1, 1, 1, 1, 1, 1, .5, .25, 2}, grid[5] = {0, 0, 0, 0, 0};
    CHECK(gih_add_height_fog(s, fog, grid, 5, 0) == -2 && strstr(gih_last_error(s), "noise grid size does not match"));
    const double flat[12] = {0, 0, 0, 1, 1, 1, 1, 1, 1, .5, .25, 0};
    CHECK(gih_add_height_fog(s, flat, nullptr, 0, 1) == -2 && strstr(gih_last_error(s), "empty noise grid"));
    CHECK(gih_add_height_fog_grid(s, fog, grid, 0) == -1 && gih_add_height_fog_grid(s, fog, grid, 5) == 0);
    CHECK(gih_add_material_tex(s, 0, 0, 1, 1, 1) == -2 && strstr(gih_last_error(s), "mat: texture index out of range"));
    const double tex[8] = {1, 1, 2, 2, 0, 0, 0, 0};
    const uint8_t px[16] = {0};
    CHECK(gih_add_texture(s, 3, tex, nullptr, 0) == -2 && gih_add_texture(s, 2, tex, px, 12) == -2 && gih_add_texture(s, 2, tex, px, 16) == 0);
    CHECK(gih_add_material_tex(s, 0, 1, 1, 1, 1) == -2 && gih_add_material_tex(s, 0, 0, 1, 1, 1) == 1);
    gih_scene_destroy(s);
    int32_t w, h, a;
    uint8_t* rgba = nullptr;
    char err[64];
    CHECK(gih_load_png((dir + "/missing.png").c_str(), &w, &h, &a, &rgba, err, sizeof err) == -2 && strstr(err, "cannot open image"));
    CHECK(gih_load_png(few.c_str(), &w, &h, &a, &rgba, err, 8) == -2 && strlen(err) == 7);   // not a PNG; the text is cut to the buffer

    const std::string mats = "colorTex 0 0 0\ncolorTex 1 1 1\nmat 1 0 1 1 1\n";
    scn_gives(dir, (mats + "mesh missing.obj 0 0 0 0 0 0 0\nbox 0 0 0 1 1 1 0 0 0 0\n").c_str(), 0, nullptr, 12);   // the missing mesh is skipped
    scn_gives(dir, (mats + "mesh few.obj 0 0 0 0 0 0 0\nmesh far.obj 0 0 0 0 0 0 0\n").c_str(), 0, nullptr, 2);
    scn_gives(dir, (mats + "mesh few.obj 0 0 0 0 0 0 1\n").c_str(), -2, "mesh: material index out of range", 0);
    scn_gives(dir, (mats + "box 0 0 0 1 1 1 0 0 0 -1\n").c_str(), -2, "box: material index out of range", 0);
    scn_gives(dir, (mats + "sphere 0 0 0 1 7\n").c_str(), -2, "sphere: material index out of range", 0);
    scn_gives(dir, (mats + "heightFog 0 0 0 1 1 1 1 1 1 .5 .25 0\n").c_str(), -2, "heightFog: empty noise grid");
    scn_gives(dir, "imTex missing.png 1 1\n", -2, "cannot open image");
    scn_gives(dir, "imTex few.obj 1 1\n", -2, "not a PNG file");
    scn_gives(dir, "colorTex 1 1 1\nmat 0 1 1 1 1\n", -2, "mat: texture index out of range");
    scn_gives(dir, "colorTex 1 1 1\nmat -1 0 1 1 1\n", -2, "mat: texture index out of range");
}

int main(int argc, char** argv)
{
    if (argc < 4) { fprintf(stderr, "usage: host_builders <repository root> <scratch directory> <scene.scn>...\n"); return 2; }
    for (int i = 3; i < argc; i++) whole_scene(std::string(argv[1]) + "/" + argv[i]);
    single_objects();
    error_paths(argv[2]);
    printf("checksum %.17g\nhost_builders ok\n", g_sink);
    return 0;
}
