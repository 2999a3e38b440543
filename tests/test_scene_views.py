"""Which tables the walks see under every setting of the switches (gi_layout.h: apply_scene_switches, the one derivation the product and the
emulator share), against the table recorded from the emulator's own derivation before the two were merged (tests/golden/scene_views.json)."""
import ctypes as C
import itertools
import json
import os

import numpy as np
import pytest

import emul_lib
import parity_checks as pc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scene_views.json")
SWITCHES = ("wide", "cull", "entity_boxes", "clip_boxes", "walk_cut")
ENV = {"entity_boxes": "GI_ENTITY_BOXES", "clip_boxes": "GI_CLIP_BOXES", "walk_cut": "GI_WALK_CUT"}
FIELDS = ("wnodes", "cboxes", "leaf_boxes", "trace_boxes", "tcboxes", "tcuse", "shadow_boxes", "scboxes", "scuse", "pn_planes")
TABLES = {0: None, 1: "wnodes", 2: "cboxes", 3: "cuse", 4: "leaf_boxes", 5: "trace_boxes", 6: "tcboxes", 7: "tcuse", -1: "?"}


def scene_views(name, environ=os.environ):
    """{"wide cull entity_boxes clip_boxes walk_cut" as 0/1: {field: table name or None, pn_planes: 0/1, cut_margin: float}} for all 32 settings"""
    E = emul_lib.lib()
    E.emul_scene_views.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_double)]
    rt = emul_lib.EmulRayTracer().setScene(pc.named_scene(name) if isinstance(name, str) else name)
    out = {}
    for bits in itertools.product((0, 1), repeat=len(SWITCHES)):
        on = dict(zip(SWITCHES, bits))
        for k, var in ENV.items():
            environ[var] = str(on[k])
        rt.set_content_culling(on["cull"])
        rt.set_wide_nodes(on["wide"])          # (every setter derives the views again, from all five)
        ids = np.zeros(10, np.int32)
        cut = C.c_double()
        E.emul_scene_views(rt.h, ids.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(cut))
        row = {f: TABLES[int(i)] for f, i in zip(FIELDS[:9], ids[:9])}
        row["pn_planes"] = int(ids[9])
        row["cut_margin"] = cut.value
        out[" ".join(map(str, bits))] = row
    return out


# the last three are BASELINE configs 3, 2 and 4: their tables are the benchmark's.  test_scene has 500 entities of opacity 0 and IOR 1 (an alpha test
# that never passes): since the short cuts of the closest-hit walk depend on the scene it walks on behind its best hit, over whole boxes.
GOLDEN_SCENES = ("test_scene", "caustics", "cornell", "teapot")


@pytest.mark.parametrize("name", GOLDEN_SCENES)
def test_scene_views_follow_the_switches(name, monkeypatch):
    for var in ENV.values():
        monkeypatch.setenv(var, "1")           # restored afterwards; scene_views sets them per setting
    with open(GOLDEN) as f:
        want = json.load(f)[name]
    got = scene_views(name)
    assert sorted(got) == sorted(want) and len(got) == 32
    for setting in want:
        for field in FIELDS + ("cut_margin",):
            assert got[setting][field] == want[setting][field], (name, dict(zip(SWITCHES, setting.split())), field)


def _env_on(monkeypatch):
    for var in ENV.values():
        monkeypatch.setenv(var, "1")


ALL_ON = "1 1 1 1 1"


@pytest.mark.parametrize("name", ["cornell", "caustics", "teapot", "coplanar", "large_opaque"])
def test_scenes_without_an_alpha_test_keep_the_short_cuts(name, monkeypatch):
    """No entity with an alpha test (glass has IOR != 1: no test either): under the default switches the closest-hit walk looks no further than its
    best hit and walks the boxes cut to the leaves, with the content boxes made of them.  large_opaque is large_alpha_scene at opacity 1: the very
    geometry that loses the short cuts once its large triangles are half transparent."""
    _env_on(monkeypatch)
    scene = pc.coplanar_scene() if name == "coplanar" else (pc.large_alpha_scene(opacity=1.0) if name == "large_opaque" else pc.load_scene(name))
    assert not pc.alpha_entities(scene).any()
    row = scene_views(scene)[ALL_ON]
    assert row["cut_margin"] >= 0 and row["trace_boxes"] == "trace_boxes" and row["tcboxes"] == "tcboxes" and row["tcuse"] == "tcuse"
    assert row["leaf_boxes"] == "leaf_boxes" and row["shadow_boxes"] == "trace_boxes" and row["scboxes"] == "tcboxes"


@pytest.mark.parametrize("name", ["large_alpha", "large_alpha_tex", "spheres", "textures"])
def test_scenes_with_an_alpha_test_lose_the_short_cuts_under_every_setting(name, monkeypatch):
    """One entity with an alpha test (opacity < 1 at IOR 1, or an image with an alpha channel) and the closest-hit walk of the whole scene goes on
    behind its best hit (cut_margin -1) over whole entity boxes and the content boxes made of those -- and the shadow walk with it -- whatever the
    five switches say."""
    _env_on(monkeypatch)
    scene = pc.named_scene(name)
    assert pc.alpha_entities(scene).any()
    views = scene_views(scene)
    assert len(views) == 32
    for setting, row in views.items():
        on = dict(zip(SWITCHES, map(int, setting.split())))
        assert row["cut_margin"] == -1.0, (name, on)
        assert row["trace_boxes"] == row["leaf_boxes"] == row["shadow_boxes"] == ("leaf_boxes" if on["entity_boxes"] else None), (name, on, row)
        assert row["tcboxes"] == row["cboxes"] == row["scboxes"] and row["tcuse"] == row["scuse"] == "cuse", (name, on, row)
    if name.startswith("large_alpha"):      # (the two scene files are too small for wide records)
        assert views[ALL_ON]["cboxes"] == "cboxes" and views[ALL_ON]["wnodes"] == "wnodes"


if __name__ == "__main__":   # records the table: python tests/test_scene_views.py > tests/golden/scene_views.json
    print(json.dumps({n: scene_views(n) for n in GOLDEN_SCENES}, indent=0, sort_keys=True))
