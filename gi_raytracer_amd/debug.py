"""Check and debug entries of a context (gi_trace, gi_visible*, gi_debug_*, gi_kat ...): what the tests compare with the oracle.  A mixin of RayTracer,
whose handle, _check, _seed and parameter builders the methods use."""
import ctypes as C

import numpy as np

from ._abi import BAKE_MODES, BAKE_SH9, BAKE_TEXEL, _dp, _f64, _ip, _p, _up, _fp


class DebugEntries:
    def trace(self, rays):
        rays = _f64(rays).reshape(-1, 6)
        n = len(rays)
        hit = np.zeros(n, np.int32); ent = np.zeros(n, np.int32); res = np.zeros((n, 8))
        self._check(self.L.gi_trace(self.h, n, _p(rays), _p(hit, _ip), _p(ent, _ip), _p(res)), "trace")
        return hit, ent, res

    def visible(self, q):
        q = _f64(q).reshape(-1, 6)
        vis = np.zeros(len(q), np.int32)
        self._check(self.L.gi_visible(self.h, len(q), _p(q), _p(vis, _ip)), "visible")
        return vis

    def visible_rays(self, rays, mt):
        """gi_visible_rays: RayTracer::visible with the reference's own arguments, rays [n][6] = origin, unit direction, mt [n] = squared length."""
        rays = _f64(rays).reshape(-1, 6); mt = _f64(mt).reshape(-1)
        assert len(mt) == len(rays)
        vis = np.zeros(len(rays), np.int32)
        self._check(self.L.gi_visible_rays(self.h, len(rays), _p(rays), _p(mt), _p(vis, _ip)), "visible_rays")
        return vis

    def debug_walk(self, rays, mt=None, form=0, lds=True):
        """gi_debug_walk: rays [n][6] through the walk forms the passes run (form 0 a ray per lane, 1 per wave, 2 per group of 16 lanes; lds: the
        records and content boxes staged in LDS or read from global memory).  mt None: closest hit, returns (hit, ent, res) as trace();
        mt [n]: any hit below that squared length, returns vis as visible_rays()."""
        rays = _f64(rays).reshape(-1, 6)
        n = len(rays)
        hit = np.zeros(n, np.int32)
        if mt is not None:
            mt = _f64(mt).reshape(-1)
            assert len(mt) == n
            self._check(self.L.gi_debug_walk(self.h, n, _p(rays), _p(mt), int(form), 1 if lds else 0, _p(hit, _ip), None, None), "debug_walk")
            return hit
        ent = np.zeros(n, np.int32); res = np.zeros((n, 8))
        self._check(self.L.gi_debug_walk(self.h, n, _p(rays), None, int(form), 1 if lds else 0, _p(hit, _ip), _p(ent, _ip), _p(res)), "debug_walk")
        return hit, ent, res

    def samplePhotons(self, q):
        q = _f64(q).reshape(-1, 6)
        res = np.zeros((len(q), 3)); nc = np.zeros(len(q), np.int32)
        self._check(self.L.gi_gather(self.h, len(q), _p(q), _p(res), _p(nc, _ip)), "gather")
        return res, nc

    def radiance(self, rays, stream, seed=None):
        rays = _f64(rays).reshape(-1, 6)
        stream = np.ascontiguousarray(stream, np.uint32)
        out = np.zeros((len(rays), 3))
        self._check(self.L.gi_radiance(self.h, len(rays), _p(rays), _p(stream, _up), self._seed(seed), _p(out)), "radiance")
        return out

    KAT = {"fastPow": 0, "fastPrecisePow": 1, "hemisphereSample_cos": 2, "sample_phong": 3, "sphereCapSample_cos": 4, "randomUnitVec": 5, "refr": 6, "reflect": 7, "rng": 8,
           "sin": 16, "cos": 17, "acos": 18, "asin": 19, "atan2": 20, "pow": 21, "sqrt": 22}

    def kat(self, what, args):
        """Known answers of the scalar building blocks as the device computes them (include/gi_hip.h: gi_kat); args [n][k] -> [n][3]."""
        a = _f64(args)
        a = a.reshape(len(a), -1)
        out = np.zeros((len(a), 3))
        self._check(self.L.gi_kat(self.h, self.KAT[what], len(a), _p(a), a.shape[1], _p(out)), "kat")
        return out

    def sort_pairs(self, keys, vals, begin_bit=0, end_bit=32):
        """gi_debug_sort_pairs: the pipeline's radix sort on caller data (stable, by bits [begin_bit, end_bit) of the key)."""
        k = np.ascontiguousarray(keys, np.uint32); v = np.ascontiguousarray(vals, np.uint32)
        ko = np.zeros_like(k); vo = np.zeros_like(v)
        self._check(self.L.gi_debug_sort_pairs(self.h, len(k), _p(k, _up), _p(v, _up), begin_bit, end_bit, _p(ko, _up), _p(vo, _up)), "sort_pairs")
        return ko, vo

    def find_leaves(self, pos):
        """gi_debug_find_leaves: (fast, full) photon-map leaf of each position; fast = -2 where the quick descent declines."""
        p = _f64(pos).reshape(-1, 3)
        a = np.zeros(len(p), np.int32); b = np.zeros(len(p), np.int32)
        self._check(self.L.gi_debug_find_leaves(self.h, len(p), _p(p), _p(a, _ip), _p(b, _ip)), "find_leaves")
        return a, b

    GATHER_KERNELS = {"gather": 0, "gather_count": 1, "wave": 2, "wave_count": 3}

    def gather_pass(self, q, kernel, sort=True):
        """gi_debug_gather_pass: a gather pass of the streaming pipeline (k_st_gather / k_st_gather_wave, "*_count" = the counting instance) on
        queries q [n][6] = position, direction, in leaf order (sort) or the caller's.  Returns (caustic term [n][3] of query i, the keys and the
        query order the kernel read, (gather queries, gather candidates) of a counting instance)."""
        q = _f64(q).reshape(-1, 6)
        n = len(q)
        res = np.zeros((n, 3)); keys = np.zeros(n, np.uint32); order = np.zeros(n, np.uint32); cnt = (C.c_int64 * 2)()
        self._check(self.L.gi_debug_gather_pass(self.h, n, _p(q), self.GATHER_KERNELS[kernel], 1 if sort else 0, _p(res), _p(keys, _up), _p(order, _up), cnt), "gather_pass")
        return res, keys, order, (int(cnt[0]), int(cnt[1]))

    def leaf_order(self, rays, cap=256):
        """Octree::intersectSorted as the device walk produces it: per ray the pre-order indices of the non-empty leaves in visiting order."""
        rays = _f64(rays).reshape(-1, 6)
        leaf = np.zeros((len(rays), cap), np.int32); n = np.zeros(len(rays), np.int32)
        self._check(self.L.gi_debug_leaf_order(self.h, len(rays), _p(rays), cap, _p(leaf, _ip), _p(n, _ip)), "leaf_order")
        assert (n <= cap).all(), "leaf_order: cap too small"
        return [leaf[i, :n[i]].copy() for i in range(len(rays))]

    def halton_sample(self, dim, index):
        dim = np.ascontiguousarray(dim, np.uint32); index = np.ascontiguousarray(index, np.uint32)
        out = np.zeros(len(dim), np.float32)
        self._check(self.L.gi_halton_sample(self.h, len(dim), _p(dim, _up), _p(index, _up), _p(out, _fp)), "halton_sample")
        return out

    def halton_index(self, w, h, sxy):
        sxy = np.ascontiguousarray(sxy, np.uint32).reshape(-1, 3)
        out = np.zeros(len(sxy), np.uint32)
        self._check(self.L.gi_halton_index(self.h, w, h, len(sxy), _p(sxy, _up), _p(out, _up)), "halton_index")
        return out

    def photon_tables_on_device(self):
        """The photon-map tables as the gather kernel sees them (gi_debug_photon_tables)."""
        nn, nr, nph = C.c_int32(), C.c_int32(), C.c_int32()
        self._check(self.L.gi_debug_photon_tables(self.h, C.byref(nn), C.byref(nr), C.byref(nph), None, None, None, None), "photon_tables")
        nodes = np.zeros((nn.value, 128), np.uint8); ranges = np.zeros((nr.value, 2), np.int32)
        pos = np.zeros((nph.value, 3)); dircol = np.zeros((nph.value, 6))
        if nn.value:
            self._check(self.L.gi_debug_photon_tables(self.h, None, None, None, _p(nodes, C.c_void_p), _p(ranges, _ip), _p(pos), _p(dircol)), "photon_tables")
        return {"nodes": nodes, "ranges": ranges, "pos": pos, "dircol": dircol}

    def primary_rays(self, p, idx):
        """gi_debug_primary_rays: rays [n][6] = origin, unit direction of the samples with Halton indices idx of the frame p (from params), under
        the context's lens."""
        idx = np.ascontiguousarray(idx, np.uint32).reshape(-1)
        rays = np.zeros((len(idx), 6))
        self._check(self.L.gi_debug_primary_rays(self.h, C.byref(p), len(idx), _p(idx, _up), _p(rays)), "primary_rays")
        return rays

    def bake_rays(self, points, normals, samples, stream_base=0, seed=None):
        """gi_bake_rays: the rays a bake's generator makes -- (rays [n * samples][6] = origin, unit direction, streams [n * samples]), sample k of
        point i in row i * samples + k.  normals None: probes (GI_BAKE_SH9), else texels."""
        rows = self._bake_points(points, normals)
        bp = self.bake_params(BAKE_SH9 if normals is None else BAKE_TEXEL, samples, stream_base, seed)
        rays = np.zeros((len(rows) * bp.n_samples, 6)); streams = np.zeros(len(rows) * bp.n_samples, np.uint32)
        self._check(self.L.gi_bake_rays(self.h, _p(rows), len(rows), C.byref(bp), _p(rays), _p(streams, _up)), "bake_rays")
        return rays, streams

    def bake_fold(self, mode, radiance, dirs=None):
        """gi_bake_fold: the bake's fold kernel on caller data -- radiance [n][samples][3] and, for BAKE_SH9, unit directions [n][samples][3].
        Returns [n][3] (BAKE_TEXEL) or [n][9][3]."""
        mode = BAKE_MODES.get(mode, mode)
        L3 = _f64(radiance)
        n, ns = L3.shape[:2]
        d3 = _f64(dirs) if dirs is not None else None
        if L3.ndim != 3 or L3.shape[2] != 3 or (d3 is not None and d3.shape != L3.shape):
            raise ValueError("bake_fold: radiance and directions [n][samples][3] expected")
        out = np.zeros((n, 3) if mode == BAKE_TEXEL else (n, 9, 3))
        self._check(self.L.gi_bake_fold(self.h, mode, n, ns, _p(d3), _p(L3), _p(out)), "bake_fold")
        return out

    def cubemap_rays(self, pos, face, samples, stream_base=0, seed=None):
        """gi_cubemap_rays: the rays a reflection probe's capture makes -- (rays [6 face^2 samples][6] = origin, unit direction, streams
        [6 face^2 samples]), sample k of texel t in row t * samples + k."""
        p = self.cubemap_params(face, samples, 1, None, stream_base, seed)
        P = _f64(pos).reshape(3)
        n = max(self.L.gi_cubemap_chain_texels(p.face, 1), 0) * max(p.n_samples, 0)
        n = n if n < 2 ** 31 else 0                        # (the library refuses such a call: nothing is written)
        rays = np.zeros((n, 6)); streams = np.zeros(n, np.uint32)
        self._check(self.L.gi_cubemap_rays(self.h, _p(P), C.byref(p), _p(rays), _p(streams, _up)), "cubemap_rays")
        return rays, streams

    def probe_visibility_rays(self, points, size=8, n_samples=16, stream_base=0, seed=None):
        """gi_probe_visibility_rays: the rays bake_probe_visibility's capture makes -- (rays [n size^2 n_samples][6] = origin, unit direction,
        streams [n size^2 n_samples]), sample k of texel t = (i * size + y) * size + x in row t * n_samples + k."""
        pts = self._bake_points(points)
        p = self.probe_visibility_params(size, n_samples, 1.0, stream_base, seed)
        n = len(pts) * max(p.size, 0) ** 2 * max(p.n_samples, 0)
        n = n if n < 2 ** 31 else 0                        # (the library refuses such a call: nothing is written)
        rays = np.zeros((n, 6)); streams = np.zeros(n, np.uint32)
        self._check(self.L.gi_probe_visibility_rays(self.h, _p(pts), len(pts), C.byref(p), _p(rays), _p(streams, _up)), "probe_visibility_rays")
        return rays, streams

    def probe_visibility_fold(self, dist):
        """gi_probe_visibility_fold: the capture's fold on caller distances [n_texels][n_samples].  Returns [n_texels][2] = mean, mean square."""
        d = _f64(dist)
        if d.ndim != 2 or d.shape[1] < 1:
            raise ValueError("probe_visibility_fold: distances [n_texels][n_samples] expected")
        out = np.zeros((d.shape[0], 2))
        self._check(self.L.gi_probe_visibility_fold(self.h, d.shape[0], d.shape[1], _p(d), _p(out)), "probe_visibility_fold")
        return out

    def cubemap_prefilter(self, cube, levels, exponents=None):
        """gi_cubemap_prefilter: the box levels and the lobe filter of a reflection probe on the caller's cube [6][face][face][3].  Returns the list
        of levels bake_reflection_probe returns; level 0 is the input."""
        cube = _f64(cube)
        if cube.ndim != 4 or cube.shape[0] != 6 or cube.shape[1] != cube.shape[2] or cube.shape[3] != 3 or cube.shape[1] < 1:
            raise ValueError(f"cubemap_prefilter: a cube [6][face][face][3] expected, got {cube.shape}")
        p = self.cubemap_params(cube.shape[1], 1, levels, exponents)
        _, o, out = self._cube_levels(p, True)
        self._check(self.L.gi_cubemap_prefilter(self.h, C.byref(p), _p(cube), C.cast(o[0], _dp)), "cubemap_prefilter")
        return out

    def lightmap_texels(self, ent, uv, width, height, flip=False):
        """gi_lightmap_texels: the texel table a lightmap bakes -- (owner [height][width], points [n_cov][3], normals [n_cov][3], texel [n_cov]),
        covered texels in ascending y * width + x."""
        e, c = self._chart(ent, uv)
        p = self.lightmap_params(width, height, 1, 0, flip)
        cap = max(p.width, 0) * max(p.height, 0)
        owner = np.full((max(p.height, 0), max(p.width, 0)), -1, np.int32)
        rows = np.zeros((cap, 6)); texel = np.zeros(cap, np.int32)
        n_cov = C.c_int32(0)
        self._check(self.L.gi_lightmap_texels(self.h, C.byref(p), len(e), _p(e, _ip), _p(c), _p(owner, _ip), C.byref(n_cov), _p(rows), _p(texel, _ip), cap), "lightmap_texels")
        n = n_cov.value
        return owner, np.ascontiguousarray(rows[:n, 0:3]), np.ascontiguousarray(rows[:n, 3:6]), texel[:n].copy()

    def lightmap_dilate(self, values, filled, passes):
        """gi_lightmap_dilate: the lightmap's gutter dilation on caller data -- values [h][w][3], filled [h][w] (truth values), `passes` 0 .. 64.
        Returns [h][w][3]; texels still unfilled are 0 0 0."""
        v = _f64(values)
        f = np.ascontiguousarray(np.asarray(filled) != 0, np.int32)
        if v.ndim != 3 or v.shape[2] != 3 or f.shape != v.shape[:2]:
            raise ValueError("lightmap_dilate: values [h][w][3] and filled [h][w] expected")
        out = np.zeros(v.shape)
        self._check(self.L.gi_lightmap_dilate(self.h, v.shape[1], v.shape[0], int(passes), _p(v), _p(f, _ip), _p(out)), "lightmap_dilate")
        return out
