"""Rays aimed at entity edges, leaf planes and tangents (pc.entity_edge_rays; proven on the CPU build by tests/test_entity_edges_cpu.py) through every
form of the octree walk the HIP library has: gi_trace / gi_visible / gi_visible_rays with wide records on and off, content culling off, entity
boxes off, on cornell two contexts without the closest-hit short cuts, and gi_debug_walk -- a ray per lane, per wave and per group of 16 lanes,
records and content boxes from global memory and staged in LDS.  Equality with the oracle, membership in the brute force's tied set, and every
bit equal across the forms (pc.check_entity_edges).  At most 8 000 rays per launch."""
import pytest

import gi_raytracer_amd as gi
import parity_checks as pc
from test_entity_edges_cpu import CUTS_OFF, SCENES, contexts_without_cuts

pytestmark = pytest.mark.gpu
FORMS = [(form, lds) for form in (0, 1, 2) for lds in (0, 1)]


def _check(name, what, monkeypatch):
    for k in CUTS_OFF + ("GI_ENTITY_BOXES",):
        monkeypatch.delenv(k, raising=False)
    scene = pc.named_scene(name)
    print(f"{name}:")
    others = contexts_without_cuts(lambda: gi.RayTracer(0), scene, monkeypatch) if name == "cornell" else ()
    rt = gi.RayTracer(0).setScene(scene)
    n = pc.check_entity_edges(rt, scene, FORMS, what=what, key=name, brute=name != "large_alpha", others=others)
    assert sum(n.values()) >= (1000 if what == "any" else 4000)


@pytest.mark.parametrize("name", SCENES)
def test_closest_hit_on_entity_edge_rays(name, monkeypatch):
    _check(name, "closest", monkeypatch)


@pytest.mark.parametrize("name", SCENES)
def test_any_hit_on_entity_edge_rays(name, monkeypatch):
    _check(name, "any", monkeypatch)
