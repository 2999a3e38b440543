"""Host-side feeders of the product (gi_raytracer_amd/csrc/gi_host.cpp) against dumps of the reference's own loader,
Octree::rebuild and PhotonMap::rebuild (tests/golden/scene_*.npz).  Everything is exact."""
import ctypes as C
import glob
import os
import re
import subprocess

import numpy as np
import pytest

import gi_raytracer_amd as gi
import parity_checks as pc


@pytest.mark.parametrize("name", ["test_scene", "cornell", "caustics", "spheres_opaque", "caustics_02"])
def test_loader_octree_photon_map_identical_to_reference(golden, name):
    fx = golden("scene_" + name.replace("_opaque", ""))
    s = pc.load_scene(name)
    t = s.tables()
    assert np.array_equal(t["ent_kind"], fx["ent_kind"])
    assert np.array_equal(t["tri_pos"], fx["tri_pos"]) and np.array_equal(t["tri_nrm"], fx["tri_nrm"]) and np.array_equal(t["tri_uv"], fx["tri_uv"])
    rows, ref = t["mats"][t["tri_mat"]], fx["tri_mat"].copy()
    # a `mat` line without IOR: the reference reads an uninitialised double (observed 0.575 in caustics); we define 1.0
    if name == "caustics":
        assert (ref[:, 2] == 0.575).all()
        ref[:, 2] = 1.0
    assert np.array_equal(rows, ref)
    if len(fx["lights"]):
        assert np.array_equal(t["lights"], fx["lights"])      # incl. dir / angle from Octree::rebuild
    assert np.array_equal(t["node_bbox"], fx["oct_bbox"]) and np.array_equal(t["node_child"], fx["oct_child"])
    assert np.array_equal(t["node_ent_off"], fx["oct_ent_off"]) and np.array_equal(t["node_ent_idx"], fx["oct_ent_idx"])
    if "photons" in fx:
        s.build_photon_map(fx["photons"])
        p = s.photon_tables()
        assert np.array_equal(p["node_bbox"], fx["pm_bbox"])
        assert np.array_equal(np.where(p["node_child"][:, 0] >= 0, p["node_child"][:, 0], -1), fx["pm_firstchild"])
        assert np.array_equal(p["node_off"], fx["pm_off"]) and np.array_equal(p["node_idx"], fx["pm_idx"])


CSRC = os.path.join(pc.ROOT, "gi_raytracer_amd", "csrc")
_dp = C.POINTER(C.c_double)


def _p(a):
    return a.ctypes.data_as(_dp)


def _max_photons_per_leaf():
    """kMaxPhotonsPerLeaf as the host builder's source states it (gi_host.cpp and the pieces it includes)."""
    for path in sorted(glob.glob(os.path.join(CSRC, "gi_host*"))):
        m = re.search(r"\bkMaxPhotonsPerLeaf\s*=\s*(\d+)\s*;", open(path).read())
        if m:
            return int(m.group(1))
    raise AssertionError("kMaxPhotonsPerLeaf not found in the host builder's source")


PM_BOX = np.array([-1.0, -2.0, -3.0, 2.0, 1.5, 4.0])
K = _max_photons_per_leaf()


def _cloud(shape, n):
    lo, hi = PM_BOX[:3], PM_BOX[3:]
    ph = np.random.RandomState(n * 7 + len(shape)).rand(n, 9)
    ph[:, :3] = lo + ph[:, :3] * (hi - lo)
    if shape == "point":
        ph[:, :3] = [0.3, 0.4, 0.5]
    elif shape == "mid_face":
        ph[::2, 0] = lo[0] + .5 * (hi[0] - lo[0])          # the root's mid plane, as the builder computes it: these belong to the upper octants
    return ph


def _photon_map_in_box(scene, box, ph):
    box, ph = np.ascontiguousarray(box, np.float64), np.ascontiguousarray(ph, np.float64).reshape(-1, 9)
    assert scene.L.gih_build_photon_map_in_box(scene.h, _p(box), len(ph), _p(ph) if len(ph) else None) == 0
    return scene.photon_tables()


def _subtree_sizes(child):
    size = np.ones(len(child), np.int64)
    for i in range(len(child) - 1, -1, -1):                 # pre-order: every child has a larger number than its parent
        size[i] += size[child[i][child[i] >= 0]].sum()
    return size


@pytest.mark.parametrize("n", [0, 1, K, K + 1, 5000])
@pytest.mark.parametrize("shape", ["uniform", "point", "mid_face"])
def test_photon_tree_invariants(shape, n):
    """The photon octree over a cloud in PM_BOX, checked by numpy alone: every photon is listed exactly once, by a leaf whose half-open box
    holds it; an inner node lists nothing and has all eight children, numbered in pre-order (the first is the node's number + 1, each next
    one follows the subtree of the one before: consecutive numbers wherever the children are leaves); node 0 is the box given; the
    offsets do not decrease and end at n.

    shape "point" with more than K photons: the reference's PhotonMap::Node::partition, which the builder follows node for node, splits
    such a cloud until its cell is a few rounding steps wide, where the octants hold the photons no more, and lists them in no leaf
    (0 references, 457 nodes, for 17 and for 5000 photons; the parent commit gives the same).  "Exactly once" and "ends at n" cannot hold
    there; what holds is asserted: no photon is listed twice, and the offsets end at the number of references."""
    ph = _cloud(shape, n)
    t = _photon_map_in_box(gi.Scene(), PM_BOX, ph)
    child, off, idx, box = t["node_child"], t["node_off"], t["node_idx"], t["node_bbox"]
    print(f"{shape} n={n}: {len(box)} nodes, {len(idx)} references")
    assert np.array_equal(t["photons"], ph) and np.array_equal(box[0], PM_BOX)
    assert off[0] == 0 and (np.diff(off) >= 0).all() and len(off) == len(box) + 1
    inner = (child >= 0).any(axis=1)
    assert (child[inner] >= 0).all() and (np.diff(off)[inner] == 0).all()
    size = _subtree_sizes(child)
    ids = np.nonzero(inner)[0]
    assert np.array_equal(child[inner][:, 0], ids + 1)
    assert np.array_equal(child[inner][:, 1:], child[inner][:, :-1] + size[child[inner][:, :-1]])
    assert np.array_equal(child[inner][:, 7] + size[child[inner][:, 7]], ids + size[ids]) and size[0] == len(box)
    leaf_of_ref = np.repeat(np.arange(len(box)), np.diff(off))
    o, b = ph[idx, :3], box[leaf_of_ref]
    assert ((o >= b[:, :3]) & (o < b[:, 3:])).all()
    assert off[-1] == len(idx) and len(np.unique(idx)) == len(idx) and (len(idx) == 0 or (0 <= idx.min() and idx.max() < n))
    if not (shape == "point" and n > K):
        assert np.array_equal(np.sort(idx), np.arange(n)) and off[-1] == n


@pytest.mark.parametrize("name", ["test_scene", "spheres"])
def test_scene_tree_leaves_list_exactly_the_entities_that_touch_them(name):
    """For every leaf and every entity: the leaf lists the entity if and only if the closed overlap of the two boxes holds and the
    entity's own cell test (gih_entity_overlaps_box) says 1.  Children of a frozen node (a node that kept more than 3/4 of its entities
    per child on average) are leaves, and no child pointer refers to an empty node."""
    s = pc.load_scene(name)
    L, t = s.L, s.tables()
    child, off, idx, box = t["node_child"], t["node_ent_off"], t["node_ent_idx"], t["node_bbox"]
    kind, pos = t["ent_kind"], np.ascontiguousarray(t["tri_pos"].reshape(-1, 9))
    assert 0 in kind and (1 in kind or name != "spheres")        # triangles in both scenes, spheres in the second
    ebox = np.zeros((len(kind), 6))
    for e in range(len(kind)):
        assert L.gih_entity_bbox(kind[e], _p(pos[e]), _p(ebox[e])) == 0
    inner = (child >= 0).any(axis=1)
    listed = np.zeros((len(box), len(kind)), bool)
    listed[np.repeat(np.arange(len(box)), np.diff(off)), idx] = True
    assert not listed[inner].any()
    # touch[i][e]: entity e passes both tests against the box of node i; the cell test runs only where the boxes overlap
    touch = ((box[:, None, :3] <= ebox[None, :, 3:]) & (box[:, None, 3:] >= ebox[None, :, :3])).all(axis=2)
    pairs = np.argwhere(touch)
    for i, e in pairs:
        touch[i, e] = L.gih_entity_overlaps_box(kind[e], _p(pos[e]), _p(box[i])) == 1
    print(f"{name}: {len(box)} nodes, {int((~inner).sum())} leaves, {len(kind)} entities, {len(pairs)} cell tests")
    assert np.array_equal(listed[~inner], touch[~inner])
    kids = child[child >= 0]
    assert (inner[kids] | (np.diff(off)[kids] > 0)).all()
    # what a node was handed: everything for the root, below it what the parent was handed and what passes the child's tests; a node
    # that hands its eight children more than 3/4 of that on average is frozen
    have = np.zeros_like(touch)
    have[0] = True
    for i in np.nonzero(inner)[0]:
        c = child[i][child[i] >= 0]
        have[c] = have[i] & touch[c]
        if have[c].sum() / 8 > 0.75 * have[i].sum():
            assert not inner[c].any(), i


def test_photon_map_in_box_leaves_the_scene_tree_alone(golden):
    s = pc.load_scene("caustics")
    before = s.tables()
    ph = golden("scene_caustics")["photons"][:3000]
    box = np.r_[ph[:, :3].min(axis=0) - .5, ph[:, :3].max(axis=0) + .25]
    assert not np.array_equal(box, before["node_bbox"][0])
    p = _photon_map_in_box(s, box, ph)
    after = s.tables()
    assert all(np.array_equal(before[k], after[k]) for k in before)
    assert np.array_equal(p["node_bbox"][0], box)
    s.build_photon_map(ph)                                    # over the scene's root box again, not over the box left behind
    assert np.array_equal(s.photon_tables()["node_bbox"][0], before["node_bbox"][0])


def test_box_mesh_and_fog_grid_match_the_scn_keywords(tmp_path):
    """gih_box_mesh and gih_fog_grid, which need no scene, give what the `box` and `heightFog` lines of a scene file give."""
    L = gi.lib()
    boxes = [((0.5, 1, -2), (1, 2, 3), (0.1, -0.7, 2.5)), ((-3, 0, 0), (.25, .5, 4), (0, 0, 0))]
    fogs = [((0, 0, 0), (1, 2, 1), (1, 1, 1), .5, .25, 2), ((1, -1, 2), (2, 0, 3), (.5, .6, .7), 1.5, .75, 3)]
    meshes, grids = [], []
    for b in boxes:
        out = np.zeros(108)
        assert L.gih_box_mesh(*[_p(np.array(v, float)) for v in b], _p(out)) == 12
        meshes.append(out.reshape(12, 3, 3))
    for f in fogs:
        par = np.array([*f[0], *f[1], *f[2], *f[3:]], float)
        n = L.gih_fog_grid(_p(par), gi.DEFAULT_SEED, None, 0)
        g = np.zeros(n)
        assert n == (f[1][0] + 1) * (f[1][1] + 1) * (f[1][2] + 1) * f[5] ** 3 and L.gih_fog_grid(_p(par), gi.DEFAULT_SEED, _p(g), n) == n
        grids.append(g)
    scn = tmp_path / "parts.scn"
    lines = ["colorTex 0 0 0", "colorTex 1 1 1", "mat 1 0 1 1 1"]
    lines += ["box " + " ".join(repr(float(x)) for v in b for x in v) + " 0" for b in boxes]
    lines += ["heightFog " + " ".join(repr(float(x)) for x in [*f[0], *f[1], *f[2], *f[3:]]) for f in fogs[:1]]
    scn.write_text("\n".join(lines) + "\n")
    t = gi.Scene.load(str(scn)).rebuild().tables()
    assert np.array_equal(t["tri_pos"], np.concatenate(meshes))
    assert np.array_equal(t["fog_grid"], grids[0])
    # a second fog of a scene continues the scene's counter, so only a scene's first grid equals the stand-alone one
    scn.write_text("\n".join(lines[:3] + ["heightFog " + " ".join(repr(float(x)) for x in [*f[0], *f[1], *f[2], *f[3:]]) for f in fogs[1:]]) + "\n")
    assert np.array_equal(gi.Scene.load(str(scn)).rebuild().tables()["fog_grid"], grids[1])


def test_host_builders_under_sanitizers(tmp_path):
    """tests/host_builders/host_builders.cpp, a program of its own over gi_host.cpp built with the address and undefined-behaviour
    sanitizers: every scene file, both tree builders, the descriptors, the single-object entries and the loaders' error paths."""
    exe = str(tmp_path / "host_builders")
    # the loaders leave fscanf's result unchecked, as the reference's do: -Wno-unused-result
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-g", "-Wall", "-Werror", "-Wno-unused-result", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                    "-fno-omit-frame-pointer", os.path.join(pc.ROOT, "tests", "host_builders", "host_builders.cpp"), os.path.join(CSRC, "gi_host.cpp"), "-lz", "-o", exe], check=True)
    work = tmp_path / "work"
    work.mkdir()
    r = subprocess.run([exe, pc.ROOT, str(work)] + [pc.SCN[k] for k in sorted(pc.SCN)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("host_builders ok"), r.stdout + r.stderr
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr


def test_settings_defaults_and_scene_overrides():
    st = gi.Scene().settings
    assert (st.photons, st.photon_depth, st.min_samples, st.max_samples, st.noise_thresh) == (75000, 5, 8, 32, 0.0015)
    st = pc.load_scene("cornell").settings
    assert (st.photons, st.min_samples, st.max_samples) == (750000, 8, 32)


def test_programmatic_scene_and_box_keyword(tmp_path):
    s = gi.Scene()
    m = s.add_material(1.0, 1.0, 1.0, (1, 1, 1))
    tri = np.array([[[0, 0, 0], [1, 0, 0], [0, 0, 1]], [[1, 0, 0], [1, 0, 1], [0, 0, 1]]], float)
    s.add_triangles(tri, mat_idx=[m, m])
    s.add_light((0, 5, 0), (4, 4, 4), .05)
    s.rebuild()
    t = s.tables()
    assert t["node_bbox"].shape == (1, 6) and list(t["node_ent_idx"]) == [0, 1]      # 2 entities: the root stays a leaf
    scn = tmp_path / "b.scn"
    scn.write_text("colorTex 0 0 0\ncolorTex 1 1 1\nmat 1 0 1 1 1\nbox 0 1 0 1 2 3 0 0 0 0\n")
    b = gi.Scene.load(str(scn)).rebuild().tables()
    assert b["tri_pos"].shape == (12, 3, 3)
    c = 1.0 / np.sqrt(3.0)
    assert np.allclose(np.abs(b["tri_pos"][..., 0]), c * 1) and np.allclose(np.abs(b["tri_pos"][..., 2]), c * 3)


def test_bad_inputs_fail_loudly(tmp_path):
    with pytest.raises(gi.GiError):
        gi.Scene.load(str(tmp_path / "missing.scn"))
    s = gi.Scene()
    with pytest.raises(gi.GiError):
        s.desc()                                   # octree not built
    with pytest.raises(gi.GiError):
        s.add_triangles(np.zeros((1, 3, 3)), mat_idx=[3])   # no such material
    with pytest.raises(gi.GiError):
        s.add_height_fog((0, 0, 0), (1, 1, 1), (1, 1, 1), 1, .5, 2, grid=np.zeros(5))   # grid must have (sx+1)(sy+1)(sz+1) scale^3 values
    scn = tmp_path / "t.scn"
    scn.write_text("imTex a.png 1 1\n")
    with pytest.raises(gi.GiError):
        gi.Scene.load(str(scn))                    # the image file does not exist: refuse instead of guessing a colour


def test_pfm_and_ppm_writers(tmp_path):
    """Headless output: PFM of the linear frame, PPM of the reference's display transform (gamma 2.2, clamp, truncate)."""
    import gi_raytracer_amd as gi
    lin = np.random.RandomState(0).rand(5, 7, 3).astype(np.float32) * 1.5
    gi.save_pfm(str(tmp_path / "a.pfm"), lin)
    raw = open(tmp_path / "a.pfm", "rb").read()
    assert raw.startswith(b"PF\n7 5\n-1.0\n")
    back = np.frombuffer(raw[len(b"PF\n7 5\n-1.0\n"):], "<f4").reshape(5, 7, 3)[::-1]
    assert np.array_equal(back, lin)
    gi.save_ppm(str(tmp_path / "a.ppm"), lin)
    raw = open(tmp_path / "a.ppm", "rb").read()
    px = np.frombuffer(raw[len(b"P6\n7 5\n255\n"):], np.uint8).reshape(5, 7, 3)
    want = (255 * np.clip(lin.astype(np.float64) ** (1 / 2.2), 0, 1)).astype(np.int32)
    assert np.array_equal(px, want) and px.max() == 255


def test_png_decoder_matches_pil_on_every_supported_colour_type(tmp_path):
    """gih_load_png (the `imTex` loader): grey, RGB, palette (+tRNS), grey+alpha, RGBA, every scanline filter, against PIL's decode;
    16-bit and interlaced files are refused by name."""
    import ctypes as C
    from PIL import Image
    import gi_raytracer_amd as gi
    L = gi.lib()
    rs = np.random.RandomState(7)

    def load(path):
        w, h, a = C.c_int32(), C.c_int32(), C.c_int32()
        px = C.POINTER(C.c_uint8)()
        err = C.create_string_buffer(256)
        rc = L.gih_load_png(str(path).encode(), C.byref(w), C.byref(h), C.byref(a), C.byref(px), err, 256)
        if rc != 0:
            return rc, err.value.decode(), None, None
        arr = np.ctypeslib.as_array(px, (h.value, w.value, 4)).copy()
        L.gih_free(px)
        return 0, "", arr, a.value

    smooth = (np.add.outer(np.arange(37), np.arange(53)) * 3 % 256).astype(np.uint8)      # gradients make the encoder pick several filters
    cases = {
        "L": Image.fromarray(smooth, "L"),
        "RGB": Image.fromarray(np.stack([smooth, 255 - smooth, rs.randint(0, 256, smooth.shape).astype(np.uint8)], -1), "RGB"),
        "LA": Image.fromarray(np.stack([smooth, 255 - smooth], -1), "LA"),
        "RGBA": Image.fromarray(rs.randint(0, 256, (37, 53, 4)).astype(np.uint8), "RGBA"),
        "P": Image.fromarray(rs.randint(0, 256, (37, 53, 3)).astype(np.uint8), "RGB").convert("P", palette=Image.ADAPTIVE, colors=64),
    }
    for name, im in cases.items():
        path = tmp_path / (name + ".png")
        im.save(path)
        rc, err, arr, alpha = load(path)
        assert rc == 0, (name, err)
        assert np.array_equal(arr, np.array(im.convert("RGBA"))), name
        assert alpha == (1 if name in ("LA", "RGBA") else 0), name
    pal = cases["P"].copy()
    pal.info["transparency"] = 3
    pal.save(tmp_path / "ptrns.png", transparency=3)
    rc, err, arr, alpha = load(tmp_path / "ptrns.png")
    assert rc == 0 and alpha == 1 and np.array_equal(arr, np.array(Image.open(tmp_path / "ptrns.png").convert("RGBA")))
    Image.fromarray((rs.rand(8, 8) * 65535).astype(np.uint16)).save(tmp_path / "deep.png")
    rc, err, _, _ = load(tmp_path / "deep.png")
    assert rc != 0 and "8 bits" in err
    rc, err, _, _ = load(tmp_path / "missing.png")
    assert rc != 0 and "cannot open" in err


def test_texture_tables_are_validated(golden):
    """gi_upload_scene's checks of the texture tables (run here through the CPU build of the same layout code)."""
    import ctypes as C
    import gi_raytracer_amd as gi
    import emul_lib as el
    import parity_checks as pc
    scene = pc.load_scene("textures")
    rt = el.EmulRayTracer()
    d = scene.desc()
    assert rt.E.emul_upload_scene(rt.h, C.byref(d)) == 0
    mt = np.ctypeslib.as_array(d.mat_tex, (d.n_mat * 2,)).copy()
    bad = mt.copy(); bad[1] = d.n_tex
    d2 = scene.desc(); d2.mat_tex = bad.ctypes.data_as(gi._ip)
    assert rt.E.emul_upload_scene(rt.h, C.byref(d2)) != 0 and b"texture index" in rt.E.emul_error(rt.h)
    d3 = scene.desc(); d3.n_tex_pixel_bytes = 16
    assert rt.E.emul_upload_scene(rt.h, C.byref(d3)) != 0 and b"pixel table" in rt.E.emul_error(rt.h)
    kinds = np.ctypeslib.as_array(d.tex_kind, (d.n_tex,)).copy(); kinds[0] = 9
    d4 = scene.desc(); d4.tex_kind = kinds.ctypes.data_as(gi._ip)
    assert rt.E.emul_upload_scene(rt.h, C.byref(d4)) != 0 and b"texture kind" in rt.E.emul_error(rt.h)
