"""The host side (csrc/gi_host.h): `Scene` over the gih_* builder, the helpers that read its tables, and the 8-bit sink with the image writers."""
import ctypes as C
import os

import numpy as np

from ._abi import DEFAULT_SEED, GiError, PhotonMapDesc, SceneDesc, Settings, _bp, _buf, _f64, _floats, _ip, _np_from, _p, lib


class Scene:
    """Host-side scene = the reference's Octree plus what its loaders write into RayTracer (include/octree.h:39-64,
    include/sceneLoader.cpp).  Build order as in the reference: push entities / lights, `rebuild()`, then render."""

    def __init__(self):
        self.L = lib()
        self.h = C.c_void_p(self.L.gih_scene_create())

    def __del__(self):
        try:
            self.L.gih_scene_destroy(self.h)
        except Exception:
            pass

    def _err(self):
        return self.L.gih_last_error(self.h).decode()

    @classmethod
    def load(cls, scn_path):
        """loadScene(scene, raytracer, path) (include/sceneLoader.cpp:12)."""
        s = cls()
        rc = s.L.gih_load_scn(s.h, os.fsencode(scn_path))
        if rc != 0:
            raise GiError(f"load_scn({scn_path}): {s._err()}")
        return s

    def add_material(self, roughness, opacity, ior, diffuse, emissive=(0, 0, 0)):
        m = _f64([roughness, opacity, ior, *diffuse, *emissive])
        return self.L.gih_add_material(self.h, _p(m))

    def add_color_texture(self, rgb):
        """new texture(col) (include/material.h:10-30); returns the texture index."""
        return self._tex(0, [*rgb, 0, 0, 0, 0, 0], None)

    def add_checkerboard(self, a, b, tiles):
        """new checkerboard(tiles, a, b) (include/material.h:32-50)."""
        return self._tex(1, [*a, *b, tiles, 0], None)

    def add_image_texture(self, rgba, tile=(1, 1), has_alpha=True):
        """new imageTexture(file, tile) (include/material.h:52-81) from decoded pixels [h][w][4] uint8, rows top to bottom."""
        rgba = np.ascontiguousarray(rgba, np.uint8)
        h, w = rgba.shape[:2]
        return self._tex(2, [tile[0], tile[1], w, h, 1 if has_alpha else 0, 0, 0, 0], rgba.reshape(-1))

    def _tex(self, kind, params, pixels):
        par = _f64(params)
        rc = self.L.gih_add_texture(self.h, kind, _p(par), _p(pixels, _bp), len(pixels) if pixels is not None else 0)
        if rc < 0:
            raise GiError(self._err())
        return rc

    def add_material_tex(self, dif_tex, em_tex, roughness, opacity, ior=1.0):
        """new Material(tex[dif], tex[em], roughness, opacity, IOR) (include/material.h:84-100); returns the material index."""
        rc = self.L.gih_add_material_tex(self.h, int(dif_tex), int(em_tex), float(roughness), float(opacity), float(ior))
        if rc < 0:
            raise GiError(self._err())
        return rc

    def add_triangles(self, pos, nrm=None, uv=None, mat_idx=None):
        pos = _f64(pos).reshape(-1, 3, 3)
        n = len(pos)
        nrm = _f64(nrm).reshape(n, 3, 3) if nrm is not None else None
        uv = _f64(uv).reshape(n, 3, 2) if uv is not None else None
        mi = np.ascontiguousarray(mat_idx if mat_idx is not None else np.zeros(n), np.int32)
        rc = self.L.gih_add_triangles(self.h, n, _p(pos), _p(nrm), _p(uv), _p(mi, _ip))
        if rc != 0:
            raise GiError(self._err())

    def add_sphere(self, centre, radius, mat_idx):
        """o->push_back(new sphere(pos, rad, mat)) (include/sceneLoader.cpp:122-130)."""
        if self.L.gih_add_sphere(self.h, _p(_f64(centre)), float(radius), int(mat_idx)) != 0:
            raise GiError(self._err())

    def add_height_fog(self, pos, size, col, density, scatter, noise_scale, grid=None, seed=DEFAULT_SEED):
        """o->push_back(new HeightFog(...)) (include/sceneLoader.cpp:150-158).  grid=None fills the noise grid from the counter RNG
        (the reference fills it with time-seeded drand())."""
        par = _f64([*pos, *size, *col, density, scatter, noise_scale])
        g = _f64(grid) if grid is not None else None
        if self.L.gih_add_height_fog(self.h, _p(par), _p(g), 0 if g is None else len(g), seed) != 0:
            raise GiError(self._err())

    def add_light(self, pos, col, rad):
        self.L.gih_add_light(self.h, _p(_f64(pos)), _p(_f64(col)), float(rad))

    def set_ambient(self, rgb):
        self.L.gih_set_ambient(self.h, _p(_f64(rgb)))

    def set_camera(self, pos, look_at):
        self.L.gih_set_camera(self.h, _p(_f64(pos)), _p(_f64(look_at)))

    @property
    def settings(self):
        st = Settings()
        self.L.gih_get_settings(self.h, C.byref(st))
        return st

    def rebuild(self):
        """Octree::rebuild (include/octree.cpp:53-119)."""
        rc = self.L.gih_build_octree(self.h)
        if rc != 0:
            raise GiError(f"build_octree: {self._err()}")
        return self

    def desc(self):
        d = SceneDesc()
        rc = self.L.gih_get_scene_desc(self.h, C.byref(d))
        if rc != 0:
            raise GiError("scene octree not built: call rebuild() first")
        return d

    def tables(self):
        """Numpy copies of the flattened tables (tests)."""
        d = self.desc()
        nref = _np_from(d.node_ent_off, (d.n_node + 1,), np.int32)[-1]
        return {
            "tri_pos": _np_from(d.tri_pos, (d.n_tri, 3, 3), np.float64), "tri_nrm": _np_from(d.tri_nrm, (d.n_tri, 3, 3), np.float64),
            "tri_uv": _np_from(d.tri_uv, (d.n_tri, 3, 2), np.float64), "tri_mat": _np_from(d.tri_mat, (d.n_tri,), np.int32),
            "mats": _np_from(d.mats, (d.n_mat, 9), np.float64), "lights": _np_from(d.lights, (d.n_light, 11), np.float64),
            "ambient": np.array(list(d.ambient)), "node_bbox": _np_from(d.node_bbox, (d.n_node, 6), np.float64),
            "node_child": _np_from(d.node_child, (d.n_node, 8), np.int32), "node_ent_off": _np_from(d.node_ent_off, (d.n_node + 1,), np.int32),
            "node_ent_idx": _np_from(d.node_ent_idx, (int(nref),), np.int32),
            "ent_kind": _np_from(d.ent_kind, (d.n_tri,), np.int32) if d.ent_kind else np.zeros(d.n_tri, np.int32),
            "fog": _np_from(d.fog, (d.n_fog, 12), np.float64) if d.n_fog else np.zeros((0, 12)),
            "fog_grid_off": _np_from(d.fog_grid_off, (d.n_fog + 1,), np.int32) if d.n_fog else np.zeros(1, np.int32),
            "fog_grid": _np_from(d.fog_grid, (int(_np_from(d.fog_grid_off, (d.n_fog + 1,), np.int32)[-1]),), np.float64) if d.n_fog else np.zeros(0),
            "tex_kind": _np_from(d.tex_kind, (d.n_tex,), np.int32) if d.n_tex else np.zeros(0, np.int32),
            "tex_param": _np_from(d.tex_param, (d.n_tex, 8), np.float64) if d.n_tex else np.zeros((0, 8)),
            "mat_tex": _np_from(d.mat_tex, (d.n_mat, 2), np.int32) if d.n_tex else np.zeros((0, 2), np.int32),
            "tex_pixels": _np_from(d.tex_pixels, (int(d.n_tex_pixel_bytes),), np.uint8) if d.n_tex and d.n_tex_pixel_bytes else np.zeros(0, np.uint8),
        }

    def build_photon_map(self, photons):
        """PhotonMap::push_back x n + rebuild (include/photonMap.cpp:24-47)."""
        ph = _f64(photons).reshape(-1, 9)
        rc = self.L.gih_build_photon_map(self.h, len(ph), _p(ph))
        if rc != 0:
            raise GiError(f"build_photon_map: {self._err()}")
        return self

    def photon_desc(self):
        d = PhotonMapDesc()
        self.L.gih_get_photon_desc(self.h, C.byref(d))
        return d

    def photon_tables(self):
        d = self.photon_desc()
        nref = _np_from(d.node_off, (d.n_node + 1,), np.int32)[-1] if d.n_node else 0
        return {"photons": _np_from(d.photons, (d.n_photon, 9), np.float64), "node_bbox": _np_from(d.node_bbox, (d.n_node, 6), np.float64),
                "node_child": _np_from(d.node_child, (d.n_node, 8), np.int32), "node_off": _np_from(d.node_off, (d.n_node + 1,), np.int32) if d.n_node else np.zeros(1, np.int32),
                "node_idx": _np_from(d.node_idx, (int(nref),), np.int32)}


def probe_grid(box6, nx, ny, nz):
    """A regular grid of probe positions inside the box (min xyz, max xyz): the centres of its nx x ny x nz cells, [nz][ny][nx][3]."""
    b = np.asarray(box6, np.float64).reshape(6)
    ax = [b[k] + (np.arange(n) + 0.5) * ((b[3 + k] - b[k]) / n) for k, n in enumerate((int(nx), int(ny), int(nz)))]
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    return np.ascontiguousarray(np.stack([x, y, z], -1))


def reflection_probe_cells(box6, nx, ny, nz, fade):
    """The table [K][10] of a reflection probe set (RayTracer.run_baked_reflections; include/gi_hip.h: gi_render_baked_reflections_*) that cuts the
    box (min xyz, max xyz) into nx x ny x nz cells, x fastest: one probe per cell at the cell's centre (probe_grid's positions), its influence box
    the cell grown by `fade` on every side, so that neighbours overlap by 2 * fade and blend across that band.  Row = pos xyz, box_min xyz,
    box_max xyz, fade."""
    b = np.asarray(box6, np.float64).reshape(6)
    n = [int(nx), int(ny), int(nz)]
    fade = float(fade)
    if min(n) < 1 or n[0] * n[1] * n[2] > 64:
        raise ValueError(f"reflection_probe_cells: 1 .. 64 cells expected, got {n[0]} x {n[1]} x {n[2]}")
    if not np.isfinite(b).all() or not (b[3:] > b[:3]).all() or not 0.0 <= fade < float("inf"):
        raise ValueError("reflection_probe_cells: a finite box with max > min on every axis and a finite fade >= 0 expected")
    step = [(b[3 + k] - b[k]) / n[k] for k in range(3)]
    lo = [b[k] + np.arange(n[k]) * step[k] for k in range(3)]
    hi = [np.concatenate([lo[k][1:], b[3 + k:4 + k]]) for k in range(3)]      # a cell ends where the next begins; the last at the box
    iz, iy, ix = (q.reshape(-1) for q in np.meshgrid(np.arange(n[2]), np.arange(n[1]), np.arange(n[0]), indexing="ij"))
    out = np.empty((len(ix), 10))
    out[:, 0:3] = probe_grid(b, *n).reshape(-1, 3)
    for k, i in enumerate((ix, iy, iz)):
        out[:, 3 + k] = lo[k][i] - fade
        out[:, 6 + k] = hi[k][i] + fade
    out[:, 9] = fade
    return out


def cube_directions(face, ju=0.5, jv=0.5):
    """Unit directions [6][face][face][3] through the texels of a reflection probe's cube (RayTracer.bake_reflection_probe; include/gi_hip.h:
    gi_cubemap_*) at the place (ju, jv) inside each texel, the centres by default: faces +X, -X, +Y, -Y, +Z, -Z, rows growing downward.  The
    arithmetic is the header's, so the centres are the directions the prefilter uses, bit for bit."""
    n = int(face)
    if n < 1:
        raise ValueError(f"cube_directions: face must be at least 1, got {face}")
    a = (2.0 * (np.arange(n, dtype=np.float64) + float(ju))) / float(n) - 1.0
    b = (2.0 * (np.arange(n, dtype=np.float64) + float(jv))) / float(n) - 1.0
    b, a = np.meshgrid(b, a, indexing="ij")
    one = np.ones_like(a)
    u = np.stack([np.stack(v, -1) for v in ((one, -b, -a), (-one, -b, a), (a, one, b), (a, -one, -b), (a, -b, one), (-a, -b, -one))])
    return np.ascontiguousarray(u * (1.0 / np.sqrt((u[..., 0] * u[..., 0] + u[..., 1] * u[..., 1]) + u[..., 2] * u[..., 2]))[..., None])


def cube_texel_of(directions, face):
    """The texel index t = (f * face + y) * face + x of the cube texel each direction [...][3] (any length but 0) falls into: how a consumer of a
    reflection probe finds its texel.  The face is that of the largest component (the first of equals); (a, b) are the other two over its size."""
    d = np.asarray(directions, np.float64)
    n = int(face)
    m = np.abs(d)
    axis = np.argmax(m, -1)
    size = np.take_along_axis(m, axis[..., None], -1)[..., 0]
    x, y, z = (d[..., k] / size for k in range(3))
    neg = np.take_along_axis(d, axis[..., None], -1)[..., 0] < 0
    f = 2 * axis + neg
    a = np.choose(f, [-z, z, x, x, x, -x])
    b = np.choose(f, [-y, -y, z, -z, -y, -y])
    col = np.clip(np.floor((a + 1.0) * 0.5 * n), 0, n - 1).astype(np.int64)
    row = np.clip(np.floor((b + 1.0) * 0.5 * n), 0, n - 1).astype(np.int64)
    return (f * n + row) * n + col


def _octa_fold(px, py):
    sx, sy = np.where(px >= 0.0, 1.0, -1.0), np.where(py >= 0.0, 1.0, -1.0)
    return (1.0 - np.abs(py)) * sx, (1.0 - np.abs(px)) * sy


def octa_decode(a, b):
    """The unnormalised direction [...][3] of the point (a, b) in [0, 1]^2 of a probe's octahedral visibility map (RayTracer.bake_probe_visibility;
    include/gi_hip.h: gi_probe_visibility_*): the upper half sphere is the square's inner diamond, the lower half its corners folded outward.  The
    arithmetic is the header's, bit for bit.  Texel (x, y) of a map of M x M has its centre at ((x + 0.5) / M, (y + 0.5) / M)."""
    a, b = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64))
    px, py = 2.0 * a - 1.0, 2.0 * b - 1.0
    vz = (1.0 - np.abs(px)) - np.abs(py)
    fx, fy = _octa_fold(px, py)
    low = vz < 0.0
    return np.stack([np.where(low, fx, px), np.where(low, fy, py), vz], -1)


def octa_encode(v):
    """(a, b) of the vectors v [...][3] (any length but 0) in the octahedral map: the inverse of octa_decode up to the length, the header's
    arithmetic bit for bit.  How the look-up of run_baked_visibility finds the texels of a direction."""
    v = np.asarray(v, np.float64)
    s = (np.abs(v[..., 0]) + np.abs(v[..., 1])) + np.abs(v[..., 2])
    with np.errstate(divide="ignore", invalid="ignore"):
        px, py = v[..., 0] / s, v[..., 1] / s
    fx, fy = _octa_fold(px, py)
    low = v[..., 2] < 0.0
    px, py = np.where(low, fx, px), np.where(low, fy, py)
    return (px + 1.0) * 0.5, (py + 1.0) * 0.5


def chart_of_material(scene, material=None):
    """(ent [n], uv [n][3][2]): the default chart of a lightmap (RayTracer.bake_lightmap) for a scene whose texture coordinates are already an
    unwrapped atlas -- the scene's own texture coordinates of all triangle entities of that material index, in entity order; None: of all
    triangles.  Spheres are left out."""
    t = scene.tables()
    keep = t["ent_kind"] != 1
    if material is not None:
        keep &= t["tri_mat"] == int(material)
    ent = np.flatnonzero(keep).astype(np.int32)
    return ent, np.ascontiguousarray(t["tri_uv"][ent], np.float64).reshape(-1, 3, 2)


def save_pfm(path, lin):
    """Linear radiance [h][w][3] (`PF`) or a single-channel image [h][w] / [h][w][1] (`Pf`) as a little-endian PFM (rows bottom to top)."""
    a = np.ascontiguousarray(lin, np.float32)
    if a.ndim == 3 and a.shape[2] == 1:
        a = a[:, :, 0]
    if not (a.ndim == 2 or (a.ndim == 3 and a.shape[2] == 3)):
        raise ValueError(f"save_pfm: [h][w][3] or [h][w] expected, got shape {a.shape}")
    with open(path, "wb") as f:
        f.write(b"%s\n%d %d\n-1.0\n" % (b"PF" if a.ndim == 3 else b"Pf", a.shape[1], a.shape[0]))
        f.write(a[::-1].astype("<f4").tobytes())


def to_rgb8(lin):
    """The reference's display transform: gamma 2.2, clamp to [0, 1], truncating (int)(255 c) (include/raytracer.h:150-157, image.h:15)."""
    a = _floats(lin)
    out = np.zeros(a.shape, np.uint8)
    if lib().gih_to_rgb8(*_buf(a), a.size, _p(out, _bp)) != 0:
        raise GiError("to_rgb8: invalid arguments")
    return out


def save_ppm(path, lin):
    a = to_rgb8(lin)
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (a.shape[1], a.shape[0]))
        f.write(a.tobytes())
