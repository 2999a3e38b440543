"""Rays aimed at entity edges, leaf planes and tangents (pc.entity_edge_rays) through the CPU build of the device code: the per-lane walks -- trace,
visible, visible_rays with every switch, and gi_debug_walk's form 0 over plain memory -- against the oracle and a brute force over all entities.
This is what proves the ray set and its expectations without a GPU; tests/test_gpu_entity_edges.py sends the same rays through the HIP library,
the one-ray-per-group walks and the LDS-staged records included."""
import pytest

import emul_lib as el
import parity_checks as pc

SCENES = ["test_scene", "cornell", "spheres_opaque", "textures_opaque", "large_alpha"]
CUTS_OFF = ("GI_CLIP_BOXES", "GI_WALK_CUT")


def contexts_without_cuts(make, scene, monkeypatch):
    """Two more contexts for a scene whose closest-hit short cuts are active: one created under GI_CLIP_BOXES=0, one under GI_WALK_CUT=0."""
    out = []
    for knob in CUTS_OFF:
        for k in CUTS_OFF:
            monkeypatch.delenv(k, raising=False)
        monkeypatch.setenv(knob, "0")
        out.append((f"{knob}=0", make().setScene(scene)))
    for k in CUTS_OFF:
        monkeypatch.delenv(k, raising=False)
    return out


@pytest.mark.parametrize("what", ["closest", "any"])
@pytest.mark.parametrize("name", SCENES)
def test_entity_edge_rays_on_the_cpu_build(name, what, monkeypatch):
    for k in CUTS_OFF + ("GI_ENTITY_BOXES",):
        monkeypatch.delenv(k, raising=False)
    scene = pc.named_scene(name)
    print(f"{name}:")
    others = contexts_without_cuts(el.EmulRayTracer, scene, monkeypatch) if name == "cornell" else ()
    rt = el.EmulRayTracer().setScene(scene)
    n = pc.check_entity_edges(rt, scene, [(0, 0)], what=what, key=name, brute=name != "large_alpha", others=others)
    assert sum(n.values()) >= (1000 if what == "any" else 4000)
