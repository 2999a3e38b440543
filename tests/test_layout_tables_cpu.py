"""Every table gi_layout.h builds (layout_scene, layout_photons), byte for byte, and every refusal's text, against tests/golden/layout_tables.json:
per scene the SHA-256 and length of the raw storage of each HostScene / HostPhotons vector and the scalars beside them, read through the CPU build
of the device code (tests/host_emul: emul_layout_table, emul_layout_scalars).  Frames and hit tables show a layout error only indirectly; this
shows which table moved.  Every record type is free of padding or zeroed before it is filled, so the bytes are a function of the descriptor.

The golden file was recorded once, from the layout code as it stood before it was split into named steps; record it again (python
tests/test_layout_tables_cpu.py > tests/golden/layout_tables.json) only from a gi_layout.h whose tables are known to be right."""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))     # (for the recorder; conftest.py does it for pytest)

import gi_raytracer_amd as gi
import emul_lib
import parity_checks as pc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "layout_tables.json")
SCENE_TABLES = ("tnodes", "wnodes", "wleaf_id", "cboxes", "cuse", "refs", "leaf_tris", "leaf_boxes", "trace_boxes", "tcboxes", "tcuse", "worder",
                "tris", "shade", "tri_uv", "mats", "lights", "fogs", "fog_grid", "texs", "tex_pixels", "tex_lut")
PHOTON_TABLES = ("nodes", "ranges", "pos", "dircol")
TABLES = SCENE_TABLES + PHOTON_TABLES                   # emul_layout_table's order
SCENE_SCALARS = ("n_node", "n_tri", "n_light", "n_tex", "n_fog", "ambient0", "ambient1", "ambient2", "cut_margin", "clipped", "lights_clear")
PHOTON_SCALARS = ("planes_ok", "n_photon", "n_pnode")
SCALARS = SCENE_SCALARS + PHOTON_SCALARS                # emul_layout_scalars' order
EMPTY = "0 " + hashlib.sha256(b"").hexdigest()


def _lib():
    E = emul_lib.lib()
    E.emul_layout_table.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
    E.emul_layout_scalars.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
    E.emul_layout_scalars.restype = None
    return E


def tables_of(rt, names, scalars):
    """{table: "bytes sha256"} of the named tables of the emulator rt, and {"scalars": {name: value}}"""
    E = _lib()
    out = {}
    for name in names:
        p, n = C.c_void_p(), C.c_uint64()
        assert E.emul_layout_table(rt.h, TABLES.index(name), C.byref(p), C.byref(n)) == 0
        out[name] = f"{n.value} {hashlib.sha256(C.string_at(p, n.value) if n.value else b'').hexdigest()}"
    v = (C.c_double * len(SCALARS))()
    E.emul_layout_scalars(rt.h, v)
    out["scalars"] = {k: v[SCALARS.index(k)] for k in scalars}
    return out


def desc_of(t):
    """A gi.SceneDesc over the arrays of t (Scene.tables(), edited): a key set to None is a null table, "n_*" keys replace the counts.
    The descriptor keeps the arrays alive."""
    d = gi.SceneDesc()
    d._keep = []

    def ptr(key, dtype, ty):
        if t.get(key) is None:
            return None
        a = np.ascontiguousarray(t[key], dtype)
        d._keep.append(a)
        return a.ctypes.data_as(ty)
    u8 = C.POINTER(C.c_uint8)
    d.tri_pos, d.tri_nrm, d.tri_uv, d.tri_mat = ptr("tri_pos", np.float64, gi._dp), ptr("tri_nrm", np.float64, gi._dp), ptr("tri_uv", np.float64, gi._dp), ptr("tri_mat", np.int32, gi._ip)
    d.mats, d.lights, d.ent_kind = ptr("mats", np.float64, gi._dp), ptr("lights", np.float64, gi._dp), ptr("ent_kind", np.int32, gi._ip)
    d.node_bbox, d.node_child = ptr("node_bbox", np.float64, gi._dp), ptr("node_child", np.int32, gi._ip)
    d.node_ent_off, d.node_ent_idx = ptr("node_ent_off", np.int32, gi._ip), ptr("node_ent_idx", np.int32, gi._ip)
    d.fog, d.fog_grid_off, d.fog_grid = ptr("fog", np.float64, gi._dp), ptr("fog_grid_off", np.int32, gi._ip), ptr("fog_grid", np.float64, gi._dp)
    d.tex_kind, d.tex_param, d.mat_tex, d.tex_pixels = ptr("tex_kind", np.int32, gi._ip), ptr("tex_param", np.float64, gi._dp), ptr("mat_tex", np.int32, gi._ip), ptr("tex_pixels", np.uint8, u8)
    d.ambient[:] = list(t["ambient"])
    for count, table in (("n_tri", "tri_mat"), ("n_mat", "mats"), ("n_light", "lights"), ("n_node", "node_child"), ("n_fog", "fog"), ("n_tex", "tex_kind"), ("n_tex_pixel_bytes", "tex_pixels")):
        setattr(d, count, t[count] if count in t else (0 if t[table] is None else len(t[table])))
    return d


def photon_desc_of(t):
    """A gi.PhotonMapDesc over the arrays of t (Scene.photon_tables(), edited), as desc_of."""
    d = gi.PhotonMapDesc()
    d._keep = []

    def ptr(key, dtype, ty):
        if t.get(key) is None:
            return None
        a = np.ascontiguousarray(t[key], dtype)
        d._keep.append(a)
        return a.ctypes.data_as(ty)
    d.photons, d.node_bbox, d.node_child = ptr("photons", np.float64, gi._dp), ptr("node_bbox", np.float64, gi._dp), ptr("node_child", np.int32, gi._ip)
    d.node_off, d.node_idx = ptr("node_off", np.int32, gi._ip), ptr("node_idx", np.int32, gi._ip)
    d.n_photon, d.n_node = (1 if t["photons"] is None else len(t["photons"])), len(t["node_child"])
    return d


class _Made:
    """What EmulRayTracer.setScene takes: a thing with desc() and the reference's default settings."""
    def __init__(self, d):
        self.d, self.settings = d, gi.Scene().settings

    def desc(self):
        return self.d


_CACHE = {}


def _cornell():
    """Scene.tables() of the cornell scene file, loaded once; callers edit a copy (fresh())."""
    if "cornell" not in _CACHE:
        _CACHE["cornell"] = pc.load_scene("cornell").tables()
    return _CACHE["cornell"]


def fresh(t):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in t.items()}


def first_children(child, n=0):
    """The slots of node n that hold a child, in slot order."""
    return [k for k in range(8) if child[n, k] >= 0]


def not_octants_desc():
    """cornell with the upper x plane of the root's first child moved by one ulp: no longer the octant partition() gives, so layout_wide declines."""
    t = fresh(_cornell())
    ch = t["node_child"][0, first_children(t["node_child"])[0]]
    t["node_bbox"][ch, 3] = np.nextafter(t["node_bbox"][ch, 3], np.inf)
    return desc_of(t)


def light_on_entity_desc():
    """cornell with its light moved onto a vertex of entity 0: an entity within the light's radius, so the shadow walk keeps the whole boxes."""
    t = fresh(_cornell())
    t["lights"][0, :3] = t["tri_pos"][0, 0]
    return desc_of(t)


def single_leaf_desc():
    """cornell's entities under one node: the root is a leaf that refers to all of them."""
    t = fresh(_cornell())
    t["node_bbox"], t["node_child"] = t["node_bbox"][:1], np.full((1, 8), -1, np.int32)
    t["node_ent_off"], t["node_ent_idx"] = np.array([0, len(t["tri_mat"])], np.int32), np.arange(len(t["tri_mat"]), dtype=np.int32)
    return desc_of(t)


SCENES = {name: (lambda name=name: pc.load_scene(name)) for name in pc.SCN}          # the eleven scene files, the benchmark's three among them
SCENES.update({
    "two_lights_glass": lambda: pc.two_light_scene(True), "two_lights": lambda: pc.two_light_scene(False),
    "three_lights": lambda: pc.many_lights_scene(3), "four_lights_emitter": lambda: pc.many_lights_scene(4, emitter=True),
    "five_lights_fog": lambda: pc.many_lights_scene(5, fog=True), "coplanar": pc.coplanar_scene,
    "large_alpha": lambda: pc.large_alpha_scene(), "large_opaque": lambda: pc.large_alpha_scene(opacity=1.0), "large_alpha_tex": lambda: pc.large_alpha_scene(textured=True),
    "made_not_octants": lambda: _Made(not_octants_desc()), "made_single_leaf": lambda: _Made(single_leaf_desc()),
    "made_light_on_entity": lambda: _Made(light_on_entity_desc()),
})
PHOTON_SCENES = ("cornell", "caustics", "teapot", "made_planes_off")


def scene_record(name):
    rt = emul_lib.EmulRayTracer().setScene(SCENES[name]())
    return tables_of(rt, SCENE_TABLES, SCENE_SCALARS)


def photon_set(scene, n=20000):
    """n photons at numpy.random.RandomState(7) positions inside the scene's root box, every other one drawn towards the box's lower corner (u^3, in
    products: no libm), so that the map's leaves lie at different depths and some are empty; directions and colours uniform: the layout copies them."""
    box = scene.tables()["node_bbox"][0]
    rs = np.random.RandomState(7)
    u = rs.rand(n, 3)
    u[::2] = u[::2] * u[::2] * u[::2]
    return np.concatenate([box[:3] + (box[3:] - box[:3]) * u, rs.rand(n, 6)], 1)


def planes_off_desc(scene):
    """The photon map of `scene` with the lower x plane of the root's second child moved by one ulp: the children's boxes no longer follow from the planes."""
    t = scene.photon_tables()
    assert t["node_child"][0, 1] > 0
    ch = t["node_child"][0, 1]
    t["node_bbox"][ch, 0] = np.nextafter(t["node_bbox"][ch, 0], -np.inf)
    return photon_desc_of(t)


def photon_record(name):
    scene = pc.load_scene("cornell" if name == "made_planes_off" else name)
    rt = emul_lib.EmulRayTracer().setScene(scene)
    scene.build_photon_map(photon_set(scene))
    d = planes_off_desc(scene) if name == "made_planes_off" else scene.photon_desc()
    assert rt.E.emul_upload_photons(rt.h, C.byref(d)) == 0, rt.E.emul_error(rt.h)
    return tables_of(rt, PHOTON_TABLES, PHOTON_SCALARS)


# ---- refusals: cornell's tables (and a photon map over them) with one field damaged per message of validate_scene, layout_scene and layout_photons,
# and descriptors that break two rules at once: the first of the two in the order of the checks is the one reported
def _two_parents(t):
    k = first_children(t["node_child"])
    t["node_child"][0, k[1]] = t["node_child"][0, k[0]]


def _cut_off(t):
    t["node_child"][0, first_children(t["node_child"])[-1]] = -1


def _one_texture(kind, param=(0,) * 8, mat_tex0=-1):
    def edit(t):
        t["tex_kind"], t["tex_param"] = np.array([kind], np.int32), np.array([param], np.float64)
        t["mat_tex"] = np.full((len(t["mats"]), 2), -1, np.int32)
        t["mat_tex"][0, 0] = mat_tex0
        t["tex_pixels"], t["n_tex_pixel_bytes"] = None, 0
    return edit


def _empty_fog_grid(t):
    t["fog"], t["fog_grid_off"], t["fog_grid"] = np.zeros((1, 12)), np.zeros(2, np.int32), np.zeros(1)


def _set(key, value, index=None):
    def edit(t):
        if index is None:
            t[key] = value
        else:
            t[key][index] = value
    return edit


def _both(a, b):
    return lambda t: (a(t), b(t))


SCENE_REFUSALS = {
    "bad_counts": _set("n_mat", 0),
    "null_triangle_tables": _set("tri_nrm", None),
    "null_tables": lambda t: _both(_set("n_mat", len(t["mats"])), _set("mats", None))(t),
    "material_index": lambda t: _set("tri_mat", len(t["mats"]), 0)(t),
    "entity_kind": _set("ent_kind", 2, 0),
    "too_many_materials": _set("n_mat", 1 << 28),
    "null_texture_tables": _set("n_tex", -1),
    "texture_kind": _one_texture(3),
    "image_outside_pixels": _one_texture(2, (1, 1, 4, 4, 0, 0, 0, 0)),
    "material_texture_index": _one_texture(0, mat_tex0=5),
    "leaf_reference_table": _set("node_ent_off", 1, 0),
    "leaf_offsets_not_monotone": lambda t: _set("node_ent_off", t["node_ent_off"][-1] + 1, 1)(t),
    "child_not_later": lambda t: _set("node_child", 0, (0, first_children(t["node_child"])[0]))(t),
    "leaf_reference_range": lambda t: _set("node_ent_idx", len(t["tri_mat"]), 0)(t),
    "two_parents": _two_parents,
    "not_connected": _cut_off,
    "atmosphere_tables": _set("n_fog", -1),
    "empty_fog_grid": _empty_fog_grid,
    # two at once
    "two_parents+empty_fog_grid": _both(_two_parents, _empty_fog_grid),
    "leaf_reference_range+atmosphere_tables": _both(lambda t: _set("node_ent_idx", len(t["tri_mat"]), 0)(t), _set("n_fog", -1)),
    "not_connected+atmosphere_tables": _both(_cut_off, _set("n_fog", -1)),
}


def _swap_root_children(t):
    t["node_child"][0, [0, 1]] = t["node_child"][0, [1, 0]]


def _orphan(t):
    t["node_bbox"] = np.concatenate([t["node_bbox"], t["node_bbox"][-1:]])
    t["node_child"] = np.concatenate([t["node_child"], np.full((1, 8), -1, np.int32)])
    t["node_off"] = np.concatenate([t["node_off"], t["node_off"][-1:]])


PHOTON_REFUSALS = {
    "photons_null_tables": _set("photons", None),
    "photons_leaf_table": _set("node_off", 1, 0),
    "photons_leaf_reference_range": lambda t: _set("node_idx", len(t["photons"]), 0)(t),
    "photons_child_not_later": _set("node_child", 0, (0, 3)),
    "photons_leaf_offsets_not_monotone": lambda t: _set("node_off", t["node_off"][-1] + 1, 1)(t),
    "photons_partial_children": _set("node_child", -1, (0, 0)),
    "photons_not_pre_order": _swap_root_children,
    "photons_not_connected": _orphan,
    # two at once: the offsets of node 0 are looked at before its children
    "photons_leaf_offsets_not_monotone+not_pre_order": _both(_set("node_off", -1, 1), _swap_root_children),
}


def _photon_tables():
    if "photons" not in _CACHE:
        scene = pc.load_scene("cornell")
        scene.build_photon_map(photon_set(scene, 2000))
        _CACHE["photons"] = scene.photon_tables()
        assert (_CACHE["photons"]["node_child"][0] > 0).all()
    return _CACHE["photons"]


def refusal(name):
    """What emul_error says after the damaged descriptor was refused."""
    rt = emul_lib.EmulRayTracer()
    if name in SCENE_REFUSALS:
        t = fresh(_cornell())
        SCENE_REFUSALS[name](t)
        d = desc_of(t)
        rc = rt.E.emul_upload_scene(rt.h, C.byref(d))
    else:
        t = fresh(_photon_tables())
        PHOTON_REFUSALS[name](t)
        d = photon_desc_of(t)
        rc = rt.E.emul_upload_photons(rt.h, C.byref(d))
    assert rc == gi.GI_E_INVALID, (name, rc)
    return rt.E.emul_error(rt.h).decode()


def record():
    out = {"scene " + name: scene_record(name) for name in SCENES}
    out.update({"photons " + name: photon_record(name) for name in PHOTON_SCENES})
    out["refusals"] = {name: refusal(name) for name in list(SCENE_REFUSALS) + list(PHOTON_REFUSALS)}
    return out


@pytest.fixture(scope="module")
def want():
    with open(GOLDEN) as f:
        return json.load(f)


def _compare(got, want, what):
    assert sorted(got) == sorted(want), what
    for k in want:
        assert got[k] == want[k], (what, k)


@pytest.mark.parametrize("name", list(SCENES))
def test_scene_tables(name, want):
    got = scene_record(name)
    assert sorted(got) == sorted(SCENE_TABLES + ("scalars",))
    _compare(got, want["scene " + name], name)
    if name == "made_not_octants":          # no wide records: one dummy entry of cboxes / cuse, nothing made of the trace boxes
        assert got["wnodes"] == got["wleaf_id"] == got["tcboxes"] == got["tcuse"] == EMPTY and got["cboxes"][:2] == got["cuse"][:2] == "4 "
    if name == "made_single_leaf":
        assert got["wnodes"] == EMPTY and got["scalars"]["n_node"] == 1
    assert got["scalars"]["lights_clear"] == (0.0 if name in ("made_light_on_entity", "test_scene") else 1.0)     # (test_scene has no light)


@pytest.mark.parametrize("name", PHOTON_SCENES)
def test_photon_tables(name, want):
    got = photon_record(name)
    _compare(got, want["photons " + name], name)
    assert got["scalars"]["planes_ok"] == (0.0 if name == "made_planes_off" else 1.0) and got["scalars"]["n_photon"] == 20000


def test_refusals(want):
    """One descriptor per refusal of validate_scene, layout_scene and layout_photons: every message is reached, and word for word the recorded one;
    descriptors that break two rules report the one the checks meet first."""
    got = {name: refusal(name) for name in list(SCENE_REFUSALS) + list(PHOTON_REFUSALS)}
    _compare(got, want["refusals"], "refusals")
    singles = [v for k, v in got.items() if "+" not in k]
    assert len(set(singles)) == len(singles) == 26
    assert got["two_parents+empty_fog_grid"] == got["two_parents"] and got["leaf_reference_range+atmosphere_tables"] == got["leaf_reference_range"]
    assert got["not_connected+atmosphere_tables"] == got["not_connected"]
    assert got["photons_leaf_offsets_not_monotone+not_pre_order"] == got["photons_leaf_offsets_not_monotone"]


def test_a_refused_scene_leaves_the_bound_one_as_it_was():
    """emul_upload_scene lays a descriptor out beside the bound scene and swaps on success, as gi_upload_scene does: a refusal changes no table."""
    rt = emul_lib.EmulRayTracer().setScene(pc.load_scene("cornell"))
    before = tables_of(rt, SCENE_TABLES, SCENE_SCALARS)
    t = fresh(_cornell())
    _empty_fog_grid(t)                      # the last refusal of layout_scene
    d = desc_of(t)
    assert rt.E.emul_upload_scene(rt.h, C.byref(d)) == gi.GI_E_INVALID
    assert tables_of(rt, SCENE_TABLES, SCENE_SCALARS) == before


if __name__ == "__main__":   # records the file: python tests/test_layout_tables_cpu.py > tests/golden/layout_tables.json
    rec = record()
    print("{\n" + ",\n".join(json.dumps(k) + ": {\n" + ",\n".join(json.dumps(n) + ": " + json.dumps(v, sort_keys=True) for n, v in sorted(sec.items())) + "\n}"
                             for k, sec in sorted(rec.items())) + "\n}")
