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
    rt = emul_lib.EmulRayTracer().setScene(pc.load_scene(name))
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


@pytest.mark.parametrize("name", ["test_scene", "caustics"])
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


if __name__ == "__main__":   # records the table: python tests/test_scene_views.py > tests/golden/scene_views.json
    print(json.dumps({n: scene_views(n) for n in ("test_scene", "caustics")}, indent=0, sort_keys=True))
