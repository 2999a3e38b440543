// gi_host_scene.inc -- the parts a gih_scene owns (entities, materials and textures, lights / fog / settings, scene tree, photon map),
// Octree::rebuild over them and the .scn / .obj loaders.  Included by gi_host.cpp (fourth piece, after gi_host_tree.inc).

// Every part that the scene tree depends on carries the owner's tree_valid (and err, where it can refuse) and clears it when it changes.
// entities in insertion order = Octree::_root._entities order; kind 0 triangle, 1 sphere (centre = vertex 0, radius = vertex 1 x)
struct Entities {
    bool& tree_valid;
    std::vector<double> pos, nrm, uv;   // 9, 9, 6 values per entity
    std::vector<int32_t> mat, kind;
    std::vector<Aabb> box;              // cached box_of(e), filled by build_octree
    int n_ent() const { return (int)mat.size(); }
    Aabb box_of(int e) const { return entity_box(kind[e], &pos[(size_t)e * 9]); }
    bool in_cell(int e, const Aabb& cell) const { return entity_in_cell(kind[e], &pos[(size_t)e * 9], cell); }
    void push_triangle(const D3 p[3], const D3 n[3], const double t[6], int m)
    {
        for (int k = 0; k < 3; k++) { pos.push_back(p[k].x); pos.push_back(p[k].y); pos.push_back(p[k].z); }
        for (int k = 0; k < 3; k++) { nrm.push_back(n[k].x); nrm.push_back(n[k].y); nrm.push_back(n[k].z); }
        uv.insert(uv.end(), t, t + 6);
        mat.push_back(m);
        kind.push_back(0);
        tree_valid = false;
    }
    void push_sphere(D3 c, double rad, int m)   // new sphere(pos, rad, mat), include/entities.h:55-58
    {
        const D3 p[3] = {c, mk(rad, 0, 0), mk(0, 0, 0)}, z[3] = {mk(0, 0, 0), mk(0, 0, 0), mk(0, 0, 0)};
        const double t[6] = {0, 0, 0, 0, 0, 0};
        push_triangle(p, z, t, m);
        kind.back() = 1;
    }
};

// materials (9 values each) and textures (include/material.h): kind, 8 parameters, RGBA8 pixel pool; mat_tex = (diffuse, emissive) texture
// per material, -1 for a material given as plain colours
struct Materials {
    std::string& err;
    bool& tree_valid;
    std::vector<double> mats, tex_param;
    std::vector<int32_t> tex_kind, mat_tex;
    std::vector<uint8_t> tex_pixels;
    int n_mat() const { return (int)(mats.size() / 9); }
    bool textured() const { for (int32_t k : tex_kind) if (k != 0) return true; return false; }
    int add_material(const double* m9, int dif = -1, int em = -1)   // plain colours: no texture record
    {
        mats.insert(mats.end(), m9, m9 + 9);
        mat_tex.push_back(dif); mat_tex.push_back(em);
        tree_valid = false;
        return n_mat() - 1;
    }
    int add_texture(int kind, const double* p8, const uint8_t* rgba, long long n_bytes)
    {
        double q[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (kind < 0 || kind > 2 || !p8) { err = "texture: unknown kind"; return -2; }
        for (int k = 0; k < 8; k++) q[k] = p8[k];
        if (kind == 2) {
            const long long w = (long long)q[2], h = (long long)q[3];
            if (w <= 0 || h <= 0 || !rgba || n_bytes != w * h * 4) { err = "image texture: width x height x 4 bytes of RGBA expected"; return -2; }
            q[5] = (double)tex_pixels.size();
            tex_pixels.insert(tex_pixels.end(), rgba, rgba + n_bytes);
        }
        tex_kind.push_back(kind);
        tex_param.insert(tex_param.end(), q, q + 8);
        tree_valid = false;
        return (int)tex_kind.size() - 1;
    }
    int add_material_tex(int dif, int em, double r, double o, double ior)
    {
        const int nt = (int)tex_kind.size();
        if (dif < 0 || em < 0 || dif >= nt || em >= nt) { err = "mat: texture index out of range"; return -2; }
        // the colour fields hold texture::color: the colour of a colorTex, (0, 0, 0) for the others (include/material.h:34,57)
        const double* pd = &tex_param[(size_t)dif * 8];
        const double* pe = &tex_param[(size_t)em * 8];
        const bool cd = tex_kind[dif] == 0, ce = tex_kind[em] == 0;
        const double m[9] = {r, o, ior, cd ? pd[0] : 0, cd ? pd[1] : 0, cd ? pd[2] : 0, ce ? pe[0] : 0, ce ? pe[1] : 0, ce ? pe[2] : 0};
        return add_material(m, dif, em);
    }
};

// new HeightFog(pos, size, col, density, scatter, noiseScale), include/atmosphere.h:37-47: the noise grid has (sx+1)(sy+1)(sz+1) noiseScale^3
// values, counted as the constructor's loop counts them: for (int i = 0; i < (double)N; i++)
int fog_grid_size(const double* q)
{
    const double want = (q[3] + 1) * (q[4] + 1) * (q[5] + 1) * std::pow((double)(int)q[11], 3);
    int n = 0; for (int i = 0; i < want; i++) n++;
    return n;
}
// The reference draws the grid from time-seeded drand(); here value i of a scene's concatenated grids is splitmix64 of seed and i + 1.
void fog_noise(unsigned long long seed, size_t first, int n, double* out)
{
    for (int i = 0; i < n; i++) {
        unsigned long long z = seed + 0x9E3779B97F4A7C15ull * ((unsigned long long)(first + i) + 1);
        z ^= z >> 30; z *= 0xbf58476d1ce4e5b9ull; z ^= z >> 27; z *= 0x94d049bb133111ebull; z ^= z >> 31;
        out[i] = (double)(z >> 11) * (1.0 / 9007199254740992.0);
    }
}

struct Environment {
    std::string& err;
    bool& tree_valid;
    std::vector<double> lights;          // 11 per light
    std::vector<double> fog, fog_grid;   // 12 per HeightFog; concatenated noise grids
    std::vector<int32_t> fog_grid_off = std::vector<int32_t>(1, 0);
    gih_settings st;
    void set_defaults()
    {
        memset(&st, 0, sizeof st);
        st.photons = 75000; st.photon_depth = 5; st.min_samples = 8; st.max_samples = 32; st.noise_thresh = 0.0015;   // include/util.h:24-29
        const double pos[3] = {10, 5, 0}, look[3] = {0, 0, 0};                                                          // main.cpp:28
        st.sensor_diag = 0.035 * 240 * 2; st.focal_dist = 0.04 * 240;                                                   // include/camera.h:4,29-30
        set_camera(pos, look);
    }
    void set_camera(const double* pos, const double* look)   // Camera ctor, include/camera.h:9-15
    {
        const D3 p = d3(pos), f = unit(sub(d3(look), p));
        const D3 right = unit(cross3(mk(0, 1.0, 0), f)), up = cross3(f, right);
        st.cam_pos[0] = p.x; st.cam_pos[1] = p.y; st.cam_pos[2] = p.z;
        st.cam_forward[0] = f.x; st.cam_forward[1] = f.y; st.cam_forward[2] = f.z;
        st.cam_up[0] = up.x; st.cam_up[1] = up.y; st.cam_up[2] = up.z;
    }
    void add_light(const double* p, const double* c, double rad)
    {
        // Light(pos, target = 0, col, rad): dir = normalize(target - pos), angle = .125 until Octree::rebuild (include/light.h:16,26-31)
        const D3 d = unit(sub(mk(0, 0, 0), d3(p)));
        const double L[11] = {p[0], p[1], p[2], c[0], c[1], c[2], rad, d.x, d.y, d.z, .125};
        lights.insert(lights.end(), L, L + 11);
        tree_valid = false;
    }
    // the grid is given (any_size: an entity that carries its own, the C++ HeightFog, taken as it is) or comes from fog_noise
    int add_height_fog(const double* q, const double* grid, int n_grid, unsigned long long seed, bool any_size = false)
    {
        const int n = grid && any_size ? n_grid : fog_grid_size(q);
        if (n <= 0) { err = "heightFog: empty noise grid"; return -2; }
        if (grid && n_grid != n) { err = "heightFog: noise grid size does not match (sx+1)(sy+1)(sz+1) scale^3"; return -2; }
        fog.insert(fog.end(), q, q + 12);
        const size_t first = fog_grid.size();
        fog_grid.resize(first + (size_t)n);
        if (grid) std::copy(grid, grid + n, &fog_grid[first]);
        else fog_noise(seed, first, n, &fog_grid[first]);
        fog_grid_off.push_back((int32_t)fog_grid.size());
        tree_valid = false;
        return 0;
    }
};

struct SceneTree { OctreeTables t; Aabb root_box = {{0, 0, 0}, {0, 0, 0}}; };

// PhotonMap::push_back + rebuild, include/photonMap.cpp:24-47,137-192, in a box of the caller's choice
struct PhotonMap {
    std::vector<double> photons;   // 9 per photon, copied
    OctreeTables t;
    Aabb box = {{0, 0, 0}, {0, 0, 0}};
    void build(const Aabb& in, int n, const double* ph)
    {
        box = in;
        photons.assign(ph, ph + (size_t)n * 9);
        build_tree(t, box, n, PhotonRule{photons.data()});
    }
};

// what a gih_scene handle is (gi_host.cpp derives it, so that the type with a global name stands in the main file)
struct Scene {
    std::string err;
    bool tree_valid = false;
    Entities ent{tree_valid};
    Materials mat{err, tree_valid};
    Environment env{err, tree_valid};
    SceneTree tree;
    PhotonMap pm;
    Scene() { env.set_defaults(); }
    Scene(const Scene&) = delete;   // the parts point back at err and tree_valid
};

// idx counts from `first` (a .scn numbers its own materials from 0); the refusal reads "<what>: material index out of range"
bool mat_in_range(Scene& s, int idx, const char* what, int first = 0)
{
    if (idx < 0 || idx >= s.mat.n_mat() - first) s.err = std::string(what) + ": material index out of range";
    return idx >= 0 && idx < s.mat.n_mat() - first;
}

// light cones, include/octree.cpp:60-102, over the cached entity boxes: every light aims at the mean centre of the emitters (roughness
// below 0.1) and opens to the widest of them.  The running avg / cnt keep growing inside the light loop, as in the reference.
void light_cones(const Entities& ent, const std::vector<double>& mats, std::vector<double>& lights)
{
    const double kPi = 3.14159265358979323846;
    const int T = ent.n_ent();
    D3 avg = mk(0, 0, 0); double cnt = 0;
    for (int t = 0; t < T; t++)
        if (mats[(size_t)ent.mat[t] * 9] < 0.1) { avg = add(avg, centre(ent.box[t])); cnt++; }
    if (cnt > 0) avg = mk(avg.x / cnt, avg.y / cnt, avg.z / cnt);
    for (size_t l = 0; l < lights.size() / 11; l++) {
        double* L = &lights[l * 11];
        const D3 lp = d3(L), dir = unit(sub(avg, lp));
        double widest = 0;
        for (int t = 0; t < T; t++)
            if (mats[(size_t)ent.mat[t] * 9] < 0.1) {
                avg = add(avg, centre(ent.box[t]));
                const double ang = 1.0 - std::acos(dot3(dir, unit(sub(lp, ent.box[t].lo)))) / kPi;
                widest = std::fmax(widest, ang);
                cnt++;
            }
        L[7] = dir.x; L[8] = dir.y; L[9] = dir.z; L[10] = widest;
    }
}

// Octree::rebuild, include/octree.cpp:53-119
void build_octree(Scene& s)
{
    Entities& ent = s.ent;
    const int T = ent.n_ent();
    ent.box.resize((size_t)T);
    for (int t = 0; t < T; t++) ent.box[t] = ent.box_of(t);
    // Octree::push_back, include/octree.cpp:25-38: root box = union of entity boxes (root starts at (0,0,0)-(0,0,0))
    Aabb& root = s.tree.root_box;
    root.lo = mk(0, 0, 0); root.hi = mk(0, 0, 0);
    for (int t = 0; t < T; t++) {
        const Aabb& b = ent.box[t];
        if (t == 0) root = b;
        root.hi = mk(std::fmax(root.hi.x, b.hi.x), std::fmax(root.hi.y, b.hi.y), std::fmax(root.hi.z, b.hi.z));
        root.lo = mk(std::fmin(root.lo.x, b.lo.x), std::fmin(root.lo.y, b.lo.y), std::fmin(root.lo.z, b.lo.z));
    }
    light_cones(ent, s.mat.mats, s.env.lights);
    build_tree(s.tree.t, root, T, EntityRule<Entities>{ent});
    s.tree_valid = true;
}

int load_obj(Entities& ent, const std::string& path, D3 pos, D3 rot_angles, int mat)   // include/meshLoader.cpp:18-99
{
    std::vector<float> v, vt, vn;   // the reference keeps these as glm::vec3 / vec2 (float)
    const M3 R = euler_xyz(rot_angles.x, rot_angles.y, rot_angles.z);
    FILE* f = fopen(path.c_str(), "r");
    if (!f) return 1;   // missing mesh: skipped, as in the reference
    char word[128];
    for (;;) {
        if (fscanf(f, "%127s", word) == EOF) break;
        if (strcmp(word, "v") == 0) {
            D3 p;
            fscanf(f, "%lf %lf %lf\n", &p.x, &p.y, &p.z);
            const D3 w = add(mul(R, p), pos);
            v.push_back((float)w.x); v.push_back((float)w.y); v.push_back((float)w.z);
        } else if (strcmp(word, "vt") == 0) {
            double a, b;
            fscanf(f, "%lf %lf\n", &a, &b);
            vt.push_back((float)a); vt.push_back((float)b);
        } else if (strcmp(word, "vn") == 0) {
            D3 p;
            fscanf(f, "%lf %lf %lf\n", &p.x, &p.y, &p.z);
            const D3 w = mul(R, p);
            vn.push_back((float)w.x); vn.push_back((float)w.y); vn.push_back((float)w.z);
        } else if (strcmp(word, "f") == 0) {
            unsigned vi[3], ti[3], ni[3];
            const int got = fscanf(f, "%u%*[/]%u%*[/]%u %u%*[/]%u%*[/]%u %u%*[/]%u%*[/]%u\n", &vi[0], &ti[0], &ni[0], &vi[1], &ti[1], &ni[1], &vi[2], &ti[2], &ni[2]);
            if (got != 9) { fclose(f); return 2; }   // "error while reading faces": the reference stops reading this mesh
            D3 p[3], n[3]; double uv[6];
            for (int k = 0; k < 3; k++) {
                if (vi[k] == 0 || (size_t)vi[k] * 3 > v.size() || ni[k] == 0 || (size_t)ni[k] * 3 > vn.size() || ti[k] == 0 || (size_t)ti[k] * 2 > vt.size()) { fclose(f); return 2; }
                p[k] = mk(v[(vi[k] - 1) * 3], v[(vi[k] - 1) * 3 + 1], v[(vi[k] - 1) * 3 + 2]);
                n[k] = unit(mk(vn[(ni[k] - 1) * 3], vn[(ni[k] - 1) * 3 + 1], vn[(ni[k] - 1) * 3 + 2]));   // vertex ctor normalises, include/entities.h:311-316
                uv[k * 2] = vt[(ti[k] - 1) * 2]; uv[k * 2 + 1] = vt[(ti[k] - 1) * 2 + 1];
            }
            ent.push_triangle(p, n, uv, mat);
        }
    }
    fclose(f);
    return 0;
}

void box_mesh(D3 pos, D3 size, D3 rot_angles, double out108[108])   // boxMesh, include/entities.h:740-785: 12 triangles [12][3][3]
{
    static const double c[12][3][3] = {
        {{-1, -1, -1}, {-1, 1, -1}, {1, -1, -1}}, {{-1, 1, -1}, {1, 1, -1}, {1, -1, -1}},
        {{-1, -1, -1}, {-1, -1, 1}, {-1, 1, -1}}, {{-1, -1, 1}, {-1, 1, 1}, {-1, 1, -1}},
        {{-1, -1, -1}, {1, -1, -1}, {-1, -1, 1}}, {{-1, -1, 1}, {1, -1, -1}, {1, -1, 1}},
        {{-1, -1, 1}, {1, -1, 1}, {-1, 1, 1}},    {{1, -1, 1}, {1, 1, 1}, {-1, 1, 1}},
        {{-1, 1, 1}, {1, 1, 1}, {1, 1, -1}},      {{-1, 1, 1}, {1, 1, -1}, {-1, 1, -1}},
        {{1, -1, -1}, {1, 1, -1}, {1, -1, 1}},    {{1, -1, 1}, {1, 1, -1}, {1, 1, 1}}};
    const M3 R = euler_xyz(rot_angles.x, rot_angles.y, rot_angles.z);
    for (int t = 0; t < 12; t++)
        for (int k = 0; k < 3; k++) {
            const D3 u = unit(d3(c[t][k]));
            const D3 p = add(mul(R, mk(u.x * size.x, u.y * size.y, u.z * size.z)), pos);
            double* o = out108 + t * 9 + k * 3;
            o[0] = p.x; o[1] = p.y; o[2] = p.z;
        }
}
void add_box(Entities& ent, D3 pos, D3 size, D3 rot_angles, int mat)
{
    double v[108];
    box_mesh(pos, size, rot_angles, v);
    const double uv[6] = {0, 0, 0, 0, 0, 0};
    const D3 zero[3] = {mk(0, 0, 0), mk(0, 0, 0), mk(0, 0, 0)};
    for (int t = 0; t < 12; t++) {
        const D3 p[3] = {d3(v + t * 9), d3(v + t * 9 + 3), d3(v + t * 9 + 6)};
        ent.push_triangle(p, zero, uv, mat);
    }
}

int load_scn(Scene& s, const char* path)   // include/sceneLoader.cpp:12-185
{
    const std::string full = path, dir = full.substr(0, full.find_last_of("/"));
    FILE* f = fopen(path, "r");
    if (!f) { s.err = std::string("cannot open scene file: ") + path; return -1; }
    std::vector<int> tex;   // the scene file's texture list -> indices of this scene's texture table
    const int mat_base = s.mat.n_mat();
    gih_settings& st = s.env.st;
    char word[128];
    int rc = 0;
    for (;;) {
        if (fscanf(f, "%127s", word) == EOF) break;
        if (strcmp(word, "colorTex") == 0) {
            double q[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            fscanf(f, "%lf %lf %lf\n", &q[0], &q[1], &q[2]);
            tex.push_back(s.mat.add_texture(0, q, nullptr, 0));
        } else if (strcmp(word, "checkerboardTex") == 0) {   // include/sceneLoader.cpp:57-64
            double q[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            int tiles = 0;
            fscanf(f, "%lf %lf %lf %lf %lf %lf %d\n", &q[0], &q[1], &q[2], &q[3], &q[4], &q[5], &tiles);
            q[6] = tiles;
            tex.push_back(s.mat.add_texture(1, q, nullptr, 0));
        } else if (strcmp(word, "imTex") == 0) {             // include/sceneLoader.cpp:47-56
            char fn[100];
            int utile = 0, vtile = 0;
            fscanf(f, "%99s %d %d\n", fn, &utile, &vtile);
            int w = 0, h = 0;
            bool alpha = false;
            std::vector<uint8_t> px;
            if (!decode_png(dir + "/" + fn, w, h, alpha, px, s.err)) { rc = -2; break; }
            const double q[8] = {(double)utile, (double)vtile, (double)w, (double)h, alpha ? 1.0 : 0.0, 0, 0, 0};
            tex.push_back(s.mat.add_texture(2, q, px.data(), (long long)px.size()));
        } else if (strcmp(word, "mat") == 0) {
            int dif = 0, em = 0;
            double r = 0, o = 0, ior = 1.0;   // reference: IOR uninitialised when the 5th number is missing
            fscanf(f, "%d %d %lf %lf %lf\n", &dif, &em, &r, &o, &ior);
            if (dif < 0 || em < 0 || dif >= (int)tex.size() || em >= (int)tex.size()) { s.err = "mat: texture index out of range"; rc = -2; break; }
            if (s.mat.add_material_tex(tex[dif], tex[em], r, o, ior) < 0) { rc = -2; break; }
        } else if (strcmp(word, "multiMat") == 0) {
            char m[128];
            int length = 0;
            fscanf(f, "%127[0123456789 ]%n\n", m, &length);   // parsed and ignored: meshes take their single `mat` index
        } else if (strcmp(word, "mesh") == 0) {
            char fn[100];
            D3 pos, rot;
            int mat = 0;
            fscanf(f, "%99s %lf %lf %lf %lf %lf %lf %d\n", fn, &pos.x, &pos.y, &pos.z, &rot.x, &rot.y, &rot.z, &mat);
            if (!mat_in_range(s, mat, "mesh", mat_base)) { rc = -2; break; }
            load_obj(s.ent, dir + "/" + fn, pos, rot, mat_base + mat);
        } else if (strcmp(word, "box") == 0) {
            D3 pos, size, rot;
            int mat = 0;
            fscanf(f, "%lf %lf %lf %lf %lf %lf %lf %lf %lf %d\n", &pos.x, &pos.y, &pos.z, &size.x, &size.y, &size.z, &rot.x, &rot.y, &rot.z, &mat);
            if (!mat_in_range(s, mat, "box", mat_base)) { rc = -2; break; }
            add_box(s.ent, pos, size, rot, mat_base + mat);
        } else if (strcmp(word, "sphere") == 0) {
            D3 pos;
            double rad = 0;
            int mat = 0;
            fscanf(f, "%lf %lf %lf %lf %d\n", &pos.x, &pos.y, &pos.z, &rad, &mat);
            if (!mat_in_range(s, mat, "sphere", mat_base)) { rc = -2; break; }
            s.ent.push_sphere(pos, rad, mat_base + mat);
        } else if (strcmp(word, "heightFog") == 0) {
            double q[12] = {0};
            fscanf(f, "%lf %lf %lf %lf %lf %lf %lf %lf %lf %lf %lf %lf\n", &q[0], &q[1], &q[2], &q[3], &q[4], &q[5], &q[6], &q[7], &q[8], &q[9], &q[10], &q[11]);
            if (s.env.add_height_fog(q, nullptr, 0, 0x9E3779B97F4A7C15ull) != 0) { rc = -2; break; }
        } else if (strcmp(word, "light") == 0) {
            double p[3], c[3], rad = 0;
            fscanf(f, "%lf %lf %lf %lf %lf %lf %lf\n", &p[0], &p[1], &p[2], &c[0], &c[1], &c[2], &rad);
            s.env.add_light(p, c, rad);
        } else if (strcmp(word, "photons") == 0) {
            fscanf(f, "%d %d\n", &st.photons, &st.photon_depth);
        } else if (strcmp(word, "samples") == 0) {
            fscanf(f, "%d %d %lf\n", &st.min_samples, &st.max_samples, &st.noise_thresh);
        } else if (strcmp(word, "ambient") == 0) {
            fscanf(f, "%lf %lf %lf\n", &st.ambient[0], &st.ambient[1], &st.ambient[2]);
        } else if (strcmp(word, "camera") == 0) {
            double p[3], l[3];
            fscanf(f, "%lf %lf %lf %lf %lf %lf\n", &p[0], &p[1], &p[2], &l[0], &l[1], &l[2]);
            s.env.set_camera(p, l);   // Camera::setDir(lookAt - pos): same basis as the constructor
        }
    }
    fclose(f);
    return rc;
}
