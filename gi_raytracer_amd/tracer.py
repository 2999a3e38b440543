"""The device context: `RayTracer` over the gi_* entries of include/gi_hip.h."""
import ctypes as C

import numpy as np

from ._abi import (BAKE_MODES, BAKE_SH9, BAKE_TEXEL, CUBEMAP_MAX_LEVELS, DEFAULT_SEED, GI_OK, BakeParams, CubemapParams, DenoiseParams, GiError, Lens,
                   LightmapParams, ProbeVisibilityParams, RenderParams, UpsampleParams, _buf, _dev, _f64, _ip, _out, _p, lib)
from .debug import DebugEntries
from .params import _bake_points, _chart, _fill_params, _filter_array, baked_lightmap_params, baked_params, baked_reflections_params, baked_visibility_params, final_gather_params, lens_params, low_frame_size, occlusion_params, upsample_arrays
from .scene import Scene
from .sessions import ProgressiveRender, parse_checkpoint_header


class RayTracer(DebugEntries):
    """Device context = the reference's RayTracer for this path (include/raytracer.h:23-735)."""

    def __init__(self, device=0):
        self.L = lib()
        h = C.c_void_p()
        rc = self.L.gi_create(C.byref(h), int(device))
        if rc != GI_OK:
            raise GiError(f"gi_create failed ({rc}): no usable HIP device -- this path has no CPU fallback")
        self.h = h
        self.scene = None
        self._adopt(Scene().settings)  # reference defaults (include/util.h:24-29, main.cpp:28)
        self.seed = DEFAULT_SEED

    def __del__(self):
        try:
            self.L.gi_destroy(self.h)
        except Exception:
            pass

    def _adopt(self, st):
        self.photons, self.photon_depth = st.photons, st.photon_depth
        self.min_samples, self.max_samples, self.noise_thresh = st.min_samples, st.max_samples, st.noise_thresh
        self.cam_pos, self.cam_up, self.cam_forward = list(st.cam_pos), list(st.cam_up), list(st.cam_forward)
        self.sensor_diag, self.focal_dist = st.sensor_diag, st.focal_dist

    def _seed(self, seed):
        return self.seed if seed is None else seed

    def _check(self, rc, what):
        if rc < 0:
            raise GiError(f"{what}: {self.L.gi_last_error(self.h).decode()} ({rc})")
        return rc

    def set_stream(self, stream_ptr):
        self._check(self.L.gi_set_stream(self.h, stream_ptr), "set_stream")

    def setScene(self, scene, adopt_settings=True):
        """RayTracer::setScene (include/raytracer.h:35-39) + upload of the flattened tables."""
        d = scene.desc()
        self._check(self.L.gi_upload_scene(self.h, C.byref(d)), "upload_scene")
        self._check(self.L.gi_clear_photons(self.h), "clear_photons")      # a fresh PhotonMap, as RayTracer::setScene allocates
        self.scene = scene
        if adopt_settings:
            self._adopt(scene.settings)
        return self

    def upload_photon_map(self):
        d = self.scene.photon_desc()
        self._check(self.L.gi_upload_photons(self.h, C.byref(d)), "upload_photons")

    def clear_photons(self):
        """Drop the photon map (an empty PhotonMap: samplePhotons returns 0, include/raytracer.h:536-540)."""
        self._check(self.L.gi_clear_photons(self.h), "clear_photons")

    def tracePhotons(self, count=None, max_depth=5, seed=None):
        """RayTracer::tracePhotons(5, photons, ...) on the device, then PhotonMap::rebuild on the host and upload
        (include/raytracer.h:61-72,582-715).  Returns (photons [n][9], emission tries)."""
        count = self.photons if count is None else count
        n_light = self.scene.desc().n_light
        cap = max(count * max(n_light, 1), 1)
        out = np.zeros((cap, 9))
        tries = C.c_int64()
        n = self._check(self.L.gi_emit_photons(self.h, count, max_depth, self._seed(seed), _p(out), cap, C.byref(tries)), "emit_photons")
        ph = out[:n].copy()
        self.scene.build_photon_map(ph)
        self.upload_photon_map()
        return ph, tries.value

    def build_photon_map_on_device(self, photons, box=None):
        """gi_build_photon_map: the photon octree and its candidate ranges built on the device from photons [n][9]."""
        ph = _f64(photons).reshape(-1, 9)
        b = _f64(box) if box is not None else None
        self._check(self.L.gi_build_photon_map(self.h, len(ph), _p(ph), _p(b)), "build_photon_map")

    def tracePhotonsOnDevice(self, count=None, max_depth=5, seed=None):
        """gi_trace_photons: emission and photon-map build without leaving the device; returns (photons stored, emission tries)."""
        count = self.photons if count is None else count
        tries = C.c_int64()
        n = self._check(self.L.gi_trace_photons(self.h, count, max_depth, self._seed(seed), None, C.byref(tries)), "trace_photons")
        return n, tries.value

    def params(self, w, h, stripe_h=None, rank=0, world=1, min_samples=None, max_samples=None, noise_thresh=None, seed=None):
        p = RenderParams()
        p.cam_pos[:] = self.cam_pos; p.cam_up[:] = self.cam_up; p.cam_forward[:] = self.cam_forward
        p.sensor_diag, p.focal_dist = self.sensor_diag, self.focal_dist
        p.width, p.height = w, h
        p.stripe_h, p.stripe_rank, p.stripe_world = (h if stripe_h is None else stripe_h), rank, world
        p.min_samples = self.min_samples if min_samples is None else min_samples
        p.max_samples = self.max_samples if max_samples is None else max_samples
        p.noise_thresh = self.noise_thresh if noise_thresh is None else noise_thresh
        p.seed = self._seed(seed)
        return p

    def local_rows(self, p):
        return self.L.gi_local_rows(C.byref(p))

    def run(self, w, h, f64=True, want_spp=False, **kw):
        """RayTracer::run(w, h) pixel loop -> linear radiance [rows][w][3] on the host."""
        p = self.params(w, h, **kw)
        rows = self.local_rows(p)
        out, o = _out((rows, w, 3), f64)
        spp = np.zeros((rows, w), np.int32) if want_spp else None
        self._check(self.L.gi_render_host(self.h, C.byref(p), *o, _p(spp, C.c_void_p), None), "render_host")
        return (out, spp) if want_spp else out

    def progressive(self, w, h, **kw):
        """A progressive session of the frame run(w, h, **kw) renders (same keywords): ProgressiveRender.step(n) refines it n samples at a time."""
        p = self.params(w, h, **kw)
        self._check(self.L.gi_progressive_begin(self.h, C.byref(p)), "progressive_begin")
        return ProgressiveRender(self, w, self.local_rows(p))

    def resume(self, blob):
        """Open a session from ProgressiveRender.save()'s blob.  The caller has set the same scene and traced the same photons (same seed and count)."""
        blob = bytes(blob)
        self._check(self.L.gi_progressive_restore(self.h, blob, len(blob)), "progressive_restore")
        h = parse_checkpoint_header(blob)
        p = RenderParams()
        p.width, p.height, p.stripe_h, p.stripe_rank, p.stripe_world = h["width"], h["height"], h["stripe_h"], h["stripe_rank"], h["stripe_world"]
        return ProgressiveRender(self, h["width"], self.local_rows(p))

    def run_device(self, p, out_ptr, f64=False, spp_ptr=None):
        """Render into device memory (bench / multi-GPU path); out_ptr is a raw device pointer."""
        self._check(self.L.gi_render_device(self.h, C.byref(p), *_dev(out_ptr, f64), spp_ptr or None, None), "render_device")

    def run_features(self, w, h, n, f64=True, want_ids=True, **kw):
        """First-hit feature buffers of the frame `run` renders (gi_render_features_host; an addition, the reference has no such pass): per pixel the
        mean over samples 0 .. n-1 of the first hit's diffuse colour, normal, distance and coverage, and the entity / material of sample 0's hit.
        Returns a dict of views into one array `features` [rows][w][8]: albedo [rows][w][3], normal [rows][w][3], depth [rows][w], coverage [rows][w],
        and ids [rows][w][2] int32 (None without want_ids).  **kw as for run (stripes, seed); min_samples / max_samples play no part."""
        p = self.params(w, h, **kw)
        rows = self.local_rows(p)
        out, o = _out((rows, w, 8), f64)
        ids = np.zeros((rows, w, 2), np.int32) if want_ids else None
        self._check(self.L.gi_render_features_host(self.h, C.byref(p), int(n), *o, _p(ids, C.c_void_p)), "render_features_host")
        return {"features": out, "albedo": out[:, :, 0:3], "normal": out[:, :, 3:6], "depth": out[:, :, 6], "coverage": out[:, :, 7], "ids": ids}

    def run_features_device(self, p, n, out_ptr, f64=False, ids_ptr=None):
        """The feature pass into device memory; out_ptr ([rows][w][8]) and ids_ptr ([rows][w][2] int32, optional) are raw device pointers."""
        self._check(self.L.gi_render_features_device(self.h, C.byref(p), int(n), *_dev(out_ptr, f64), ids_ptr or None), "render_features_device")

    def _last_ms(self, name):
        """gi_last_<name>_ms of an auxiliary pass."""
        ms = C.c_float()
        self._check(getattr(self.L, f"gi_last_{name}_ms")(self.h, C.byref(ms)), f"last_{name}_ms")
        return ms.value

    def last_features_ms(self):
        """gi_last_features_ms: device time of the last feature pass (last_render_ms / last_kernel_ms keep the last frame's)."""
        return self._last_ms("features")

    def denoise_params(self, w, h, **kw):
        """gi_denoise_default_params with width, height and any of iterations, demodulate, sigma_color, sigma_normal, sigma_depth, sigma_albedo set."""
        p = DenoiseParams()
        self.L.gi_denoise_default_params(C.byref(p))
        p.width, p.height = int(w), int(h)
        return _fill_params(p, kw, ("iterations", "demodulate"), ("sigma_color", "sigma_normal", "sigma_depth", "sigma_albedo"), "denoise")

    def denoise(self, color, features, f64=None, **kw):
        """The edge-avoiding a-trous denoiser (gi_denoise_host; an addition, the reference has no denoiser) on a whole frame: color [h][w][3] as
        `run` returns it, features [h][w][8] as `run_features` returns them (its dict is accepted too), each float32 or float64.  Returns
        [h][w][3], float64 unless f64=False (default: the colour's type).  **kw: iterations (0 .. 8), demodulate, sigma_color, sigma_normal,
        sigma_depth, sigma_albedo; the formula is stated in include/gi_hip.h.  Needs no scene."""
        color, features = _filter_array(color), _filter_array(features)
        if color.ndim != 3 or color.shape[2] != 3 or features.shape != color.shape[:2] + (8,):
            raise ValueError(f"denoise: color [h][w][3] and features [h][w][8] expected, got {color.shape} and {features.shape}")
        if f64 is None:
            f64 = color.dtype == np.float64
        h, w = color.shape[:2]
        p = self.denoise_params(w, h, **kw)
        out, o = _out((h, w, 3), f64)
        self._check(self.L.gi_denoise_host(self.h, C.byref(p), *_buf(color), *_buf(features), *o), "denoise_host")
        return out

    def denoise_device(self, p, color_ptr, features_ptr, out_ptr, color_f64=False, features_f64=False, out_f64=False):
        """The denoiser on device memory, asynchronous on the context's stream; p from denoise_params; raw device pointers to [h][w][3],
        [h][w][8] and [h][w][3]; out_ptr may equal color_ptr."""
        self._check(self.L.gi_denoise_device(self.h, C.byref(p), *_dev(color_ptr, color_f64), *_dev(features_ptr, features_f64), *_dev(out_ptr, out_f64)), "denoise_device")

    def last_denoise_ms(self):
        """gi_last_denoise_ms: device time of the last denoiser pass (the frame's and the feature pass's times keep theirs)."""
        return self._last_ms("denoise")

    def upsample_params(self, w, h, factor, **kw):
        """gi_upsample_default_params with the full size w x h, the factor, the low size (the ceilings) and any of demodulate, sigma_normal,
        sigma_depth, sigma_albedo set."""
        p = UpsampleParams()
        self.L.gi_upsample_default_params(C.byref(p))
        p.width, p.height, p.factor = int(w), int(h), int(factor)
        if p.factor > 0:
            p.low_width, p.low_height = -(-p.width // p.factor), -(-p.height // p.factor)
        return _fill_params(p, kw, ("demodulate",), ("sigma_normal", "sigma_depth", "sigma_albedo"), "upsample")

    def upsample(self, low_color, low_features, features, factor, f64=None, **kw):
        """The guided upsampler (gi_upsample_host; an addition, the reference has none): a full-size frame [h][w][3] from low_color [hl][wl][3] as `run`
        returns it at the reduced size, low_features [hl][wl][8] and features [h][w][8] as `run_features` returns them at the two sizes (its dicts
        are accepted too), wl = ceil(w / factor), hl = ceil(h / factor), each float32 or float64.  Returns float64 unless f64=False (default: the
        colour's type).  **kw: demodulate, sigma_normal, sigma_depth, sigma_albedo; the formula is stated in include/gi_hip.h.  Needs no scene."""
        low_color, low_features, features = upsample_arrays(low_color, low_features, features, factor)
        if f64 is None:
            f64 = low_color.dtype == np.float64
        h, w = features.shape[:2]
        p = self.upsample_params(w, h, factor, **kw)
        out, o = _out((h, w, 3), f64)
        self._check(self.L.gi_upsample_host(self.h, C.byref(p), *_buf(low_color), *_buf(low_features), *_buf(features), *o), "upsample_host")
        return out

    def upsample_device(self, p, low_color_ptr, low_features_ptr, features_ptr, out_ptr, low_color_f64=False, low_features_f64=False, features_f64=False, out_f64=False):
        """The upsampler on device memory, asynchronous on the context's stream; p from upsample_params; raw device pointers to [hl][wl][3],
        [hl][wl][8], [h][w][8] and [h][w][3]; out must not overlap an input."""
        self._check(self.L.gi_upsample_device(self.h, C.byref(p), *_dev(low_color_ptr, low_color_f64), *_dev(low_features_ptr, low_features_f64),
                                              *_dev(features_ptr, features_f64), *_dev(out_ptr, out_f64)), "upsample_device")

    def last_upsample_ms(self):
        """gi_last_upsample_ms: device time of the last upsampler pass (the frame's, the feature pass's and the denoiser's times keep theirs)."""
        return self._last_ms("upsample")

    def occlusion_params(self, **kw):
        """The module's occlusion_params: n, dirs, radius (and width, height for the Halton cap) -> gi_occlusion_params; ValueError for bad values."""
        return occlusion_params(**kw)

    def run_occlusion(self, w, h, n=16, dirs=16, radius=0.0, f64=True, **kw):
        """Ambient occlusion and bent normals of the frame `run` renders (gi_render_occlusion_host; an addition, the reference has no such pass): per
        pixel the mean over samples 0 .. n-1 of the share of `dirs` cosine-distributed segments of length `radius` above the first hit that meet
        nothing, and of the mean direction of those.  radius=0: a tenth of the scene box's diagonal.  Returns a dict of views into one array
        `occlusion` [rows][w][4]: open [rows][w], bent [rows][w][3].  **kw as for run (stripes, seed).  ValueError for a bad n, dirs or radius,
        before the library is called; the definition is stated in include/gi_hip.h."""
        op = occlusion_params(n=n, dirs=dirs, radius=radius, width=w, height=h)
        p = self.params(w, h, **kw)
        rows = self.local_rows(p)
        out, o = _out((rows, w, 4), f64)
        self._check(self.L.gi_render_occlusion_host(self.h, C.byref(p), C.byref(op), *o), "render_occlusion_host")
        return {"occlusion": out, "open": out[:, :, 0], "bent": out[:, :, 1:4]}

    def run_occlusion_device(self, p, op, out_ptr, f64=False):
        """The occlusion pass into device memory, asynchronous on the context's stream; p from params, op from occlusion_params; out_ptr
        ([rows][w][4]) is a raw device pointer."""
        self._check(self.L.gi_render_occlusion_device(self.h, C.byref(p), C.byref(op), *_dev(out_ptr, f64)), "render_occlusion_device")

    def last_occlusion_ms(self):
        """gi_last_occlusion_ms: device time of the last occlusion pass (the frame's and the other passes' times keep theirs)."""
        return self._last_ms("occlusion")

    def bake_params(self, mode, samples, stream_base=0, seed=None):
        """gi_bake_params: mode BAKE_TEXEL / BAKE_SH9 (or "texel" / "sh9"), samples per point, the stream index of sample 0 of point 0, the seed
        (default: the tracer's)."""
        p = BakeParams()
        self.L.gi_bake_default_params(C.byref(p))
        p.mode = BAKE_MODES.get(mode, mode)
        p.n_samples, p.stream_base = int(samples), int(stream_base)
        p.seed = self._seed(seed)
        return p

    _bake_points, _chart = staticmethod(_bake_points), staticmethod(_chart)      # the input shaping of bakes and lightmaps (params.py)

    def _bake(self, rows, bp, f64):
        n = len(rows)
        out, o = _out((n, 3) if bp.mode == BAKE_TEXEL else (n, 9, 3), f64)
        self._check(self.L.gi_bake_host(self.h, _p(rows), n, C.byref(bp), *o), "bake_host")
        return out

    def bake_texels(self, points, normals, samples, stream_base=0, seed=None, f64=True):
        """Lightmap texels (gi_bake_host, GI_BAKE_TEXEL; an addition, the reference starts every path at the camera): per point [n][3] with normal
        [n][3], the mean over `samples` rays in the diffuse bounce's lobe of the radiance the path tracer finds along them -- the factor a
        roughness-1 albedo is multiplied by for its indirect term.  Direct light of the lights at the point is not in it.  Returns [n][3].
        Sample k of point i runs on stream stream_base + i * samples + k; the definition is stated in include/gi_hip.h."""
        return self._bake(self._bake_points(points, normals), self.bake_params(BAKE_TEXEL, samples, stream_base, seed), f64)

    def bake_probes(self, points, samples, stream_base=0, seed=None, f64=True):
        """Light probes (gi_bake_host, GI_BAKE_SH9): per point [n][3] the nine real spherical-harmonic coefficients (bands 0 to 2; the order is the
        header's) of the incident radiance, per colour channel, from `samples` rays uniform over the sphere.  Returns [n][9][3]."""
        return self._bake(self._bake_points(points), self.bake_params(BAKE_SH9, samples, stream_base, seed), f64)

    def bake_device(self, bp, points_ptr, n_points, out_ptr, f64=False):
        """A bake on device memory (raw device pointers: points [n][6] or [n][3] f64, out [n][3] or [n][9][3]); bp from bake_params.  The points are
        not looked at."""
        self._check(self.L.gi_bake_device(self.h, points_ptr, int(n_points), C.byref(bp), *_dev(out_ptr, f64)), "bake_device")

    def last_bake_ms(self):
        """gi_last_bake_ms: device time of the last bake (the frame's and the other passes' times keep theirs)."""
        return self._last_ms("bake")

    def lightmap_params(self, width, height, samples, dilate=2, flip=False, stream_base=0, seed=None):
        """gi_lightmap_params: the atlas size, samples per covered texel, dilation passes, whether the normals are negated, the stream index of
        sample 0 of covered texel 0, the seed (default: the tracer's)."""
        p = LightmapParams()
        self.L.gi_lightmap_default_params(C.byref(p))
        p.width, p.height, p.n_samples, p.dilate, p.flip = int(width), int(height), int(samples), int(dilate), 1 if flip else 0
        p.stream_base = int(stream_base)
        p.seed = self._seed(seed)
        return p

    def bake_lightmap(self, ent, uv, width, height, samples, dilate=2, flip=False, stream_base=0, seed=None, f64=True, want_owner=False):
        """A lightmap atlas (gi_lightmap_host; an addition around the bake): the chart -- ent [n] triangle entities, uv [n][3][2] their chart
        coordinates in [0, 1]^2, v growing with the row -- rasterised into width x height texels, every covered texel baked as bake_texels does with
        `samples` rays, the rows put back into the image and the gutters filled by `dilate` passes.  Returns the atlas [height][width][3], or
        (atlas, owner [height][width] = the chart row of a covered texel or -1, n_covered) with want_owner.  Sample k of the i-th covered texel
        (ascending y * width + x) runs on stream stream_base + i * samples + k; the definition is stated in include/gi_hip.h.  chart_of_material
        gives the chart of a scene whose texture coordinates are an atlas already."""
        e, c = self._chart(ent, uv)
        p = self.lightmap_params(width, height, samples, dilate, flip, stream_base, seed)
        atlas, a = _out((max(p.height, 0), max(p.width, 0), 3), f64)
        owner = np.full((max(p.height, 0), max(p.width, 0)), -1, np.int32) if want_owner else None
        n_cov = C.c_int32(0)
        self._check(self.L.gi_lightmap_host(self.h, C.byref(p), len(e), _p(e, _ip), _p(c), *a, _p(owner, _ip), C.byref(n_cov)), "lightmap_host")
        return (atlas, owner, n_cov.value) if want_owner else atlas

    def lightmap_device(self, p, n_chart, ent_ptr, uv_ptr, atlas_ptr, f64=False, owner_ptr=None):
        """A lightmap on device memory (raw device pointers: ent [n] int32, uv [n][3][2] f64, atlas [h][w][3], owner [h][w] int32 or None); p from
        lightmap_params.  The chart is not looked at.  Returns n_covered."""
        n_cov = C.c_int32(0)
        self._check(self.L.gi_lightmap_device(self.h, C.byref(p), int(n_chart), ent_ptr, uv_ptr, *_dev(atlas_ptr, f64), owner_ptr, C.byref(n_cov)), "lightmap_device")
        return n_cov.value

    def last_lightmap_ms(self):
        """gi_last_lightmap_ms: (device time of the last lightmap, {"raster": .., "bake": .., "dilate": ..} -- raster + rank, bake, scatter + dilate);
        gi_last_bake_ms, the frame's and the other passes' times keep theirs."""
        ms, st = C.c_float(0), (C.c_float * 3)()
        self._check(self.L.gi_last_lightmap_ms(self.h, C.byref(ms), st), "last_lightmap_ms")
        return ms.value, dict(zip(("raster", "bake", "dilate"), (float(x) for x in st)))

    def cubemap_params(self, face, samples, levels=1, exponents=None, stream_base=0, seed=None):
        """gi_cubemap_params: texels per face edge, rays per texel, levels of the chain (1: the capture alone), log2 of the lobe exponent per level
        (a sequence indexed by level, entry 0 ignored; default: the library's 16 - 3 l), the stream index of sample 0 of texel 0, the seed
        (default: the tracer's)."""
        p = CubemapParams()
        self.L.gi_cubemap_default_params(C.byref(p))
        p.face, p.n_samples, p.levels, p.stream_base = int(face), int(samples), int(levels), int(stream_base)
        p.seed = self._seed(seed)
        for l, e in enumerate(exponents if exponents is not None else ()):
            if l >= CUBEMAP_MAX_LEVELS:
                raise ValueError(f"cubemap: at most {CUBEMAP_MAX_LEVELS} exponents, got {len(exponents)}")
            p.log2_exponent[l] = int(e)
        return p

    def _cube_levels(self, p, f64):
        """A zeroed chain for p, its (void*, is_f64) pair, and the views [6][n_l][n_l][3] of its levels."""
        n = self.L.gi_cubemap_chain_texels(p.face, p.levels)
        flat, o = _out((max(n, 0), 3), f64)
        levels, at = [], 0
        for l in range(p.levels if n >= 0 else 0):
            m = p.face >> l
            levels.append(flat[at:at + 6 * m * m].reshape(6, m, m, 3))
            at += 6 * m * m
        return flat, o, levels

    def bake_reflection_probe(self, pos, face, samples, levels=1, exponents=None, stream_base=0, seed=None, f64=True):
        """A reflection probe (gi_cubemap_host; an addition beside the bakes): the cube map of the radiance seen from `pos`, `face` texels per face
        edge and `samples` jittered rays per texel, and the roughness chain filtered from it -- level l is the cube seen through the Phong lobe of
        exponent 2 ** exponents[l].  Returns a list of arrays [6][face >> l][face >> l][3], one per level; level 0 is the capture.  Faces +X, -X,
        +Y, -Y, +Z, -Z, rows growing downward: cube_directions gives the texels' directions, cube_texel_of the texel of a direction.  The lights
        themselves are not in it (no ray hits an analytic light).  Sample k of texel t runs on stream stream_base + t * samples + k; the
        definition is stated in include/gi_hip.h."""
        p = self.cubemap_params(face, samples, levels, exponents, stream_base, seed)
        P = _f64(pos).reshape(3)
        _, o, out = self._cube_levels(p, f64)
        self._check(self.L.gi_cubemap_host(self.h, _p(P), C.byref(p), *o), "cubemap_host")
        return out

    def cubemap_device(self, p, pos, out_ptr, f64=False):
        """A reflection probe into device memory (out_ptr: a raw device pointer to the whole chain, gi_cubemap_chain_texels texels of 3); p from
        cubemap_params, pos a host position, taken as it is."""
        P = _f64(pos).reshape(3)
        self._check(self.L.gi_cubemap_device(self.h, _p(P), C.byref(p), *_dev(out_ptr, f64)), "cubemap_device")

    def last_cubemap_ms(self):
        """gi_last_cubemap_ms: (device time of the last reflection probe, {"capture": .., "prefilter": ..}); gi_last_bake_ms, the frame's and the
        other passes' times keep theirs."""
        ms, st = C.c_float(0), (C.c_float * 2)()
        self._check(self.L.gi_last_cubemap_ms(self.h, C.byref(ms), st), "last_cubemap_ms")
        return ms.value, dict(zip(("capture", "prefilter"), (float(x) for x in st)))

    def baked_params(self, **kw):
        """The module's baked_params: n, sh, grid_box, chain, exponents, terms (and width, height for the Halton cap) -> (gi_baked_params, sh,
        chain); ValueError for bad values and shapes."""
        return baked_params(**kw)

    def run_baked(self, w, h, n, sh=None, grid_box=None, chain=None, exponents=None, terms=None, f64=True, **kw):
        """The baked-light pass on the frame `run` renders (gi_render_baked_host; an addition, the consumer of the bakes): per pixel the mean over
        samples 0 .. n-1 of the first hit shaded from the analytic lights (direct), the probe grid sh [nz][ny][nx][9][3] in grid_box (diffuse:
        bake_probes(probe_grid(grid_box, nx, ny, nz)) reshaped) and the reflection probe's chain (specular: the list bake_reflection_probe returns,
        filtered with `exponents`), plus the surface's emission.  terms: BAKED_* bits, default whatever data was given plus direct and emissive.
        Returns a dict of views into one array `baked` [rows][w][12]: beauty, direct, diffuse, specular, [rows][w][3] each.  **kw as for run
        (stripes, seed).  ValueError for bad values and shapes, before the library is called; the definition is stated in include/gi_hip.h."""
        bp, sh, chain = baked_params(n=n, sh=sh, grid_box=grid_box, chain=chain, exponents=exponents, terms=terms, width=w, height=h)
        p = self.params(w, h, **kw)
        rows = self.local_rows(p)
        out, o = _out((rows, w, 12), f64)
        self._check(self.L.gi_render_baked_host(self.h, C.byref(p), C.byref(bp), _p(sh), _p(chain), *o), "render_baked_host")
        return {"baked": out, "beauty": out[:, :, 0:3], "direct": out[:, :, 3:6], "diffuse": out[:, :, 6:9], "specular": out[:, :, 9:12]}

    def run_baked_device(self, p, bp, sh_ptr, chain_ptr, out_ptr, f64=False):
        """The baked-light pass on device memory, asynchronous on the context's stream; p from params, bp from baked_params; sh_ptr
        ([nz][ny][nx][9][3] f64), chain_ptr (the whole chain, f64) and out_ptr ([rows][w][12]) are raw device pointers, the first two None where
        their term is off."""
        self._check(self.L.gi_render_baked_device(self.h, C.byref(p), C.byref(bp), sh_ptr or None, chain_ptr or None, *_dev(out_ptr, f64)), "render_baked_device")

    def run_final_gather(self, w, h, n, dirs=16, sh=None, grid_box=None, chain=None, exponents=None, terms=None, want_ids=False, f64=True, **kw):
        """The final-gather pass on the frame `run` renders (gi_render_final_gather_host; an addition, one bounce from the first hits into the
        baked light): run_baked, except that the diffuse term of a first hit on the diffuse lobe is its colour times the mean over `dirs`
        cosine-distributed rays of what they hit, shaded from the analytic lights, the probe grid sh, the chain and emission (the ambient colour
        on a miss).  A chain given without the SPECULAR bit serves the secondary hits alone.  Returns run_baked's dict under the key
        `final_gather` for the array [rows][w][12]; with want_ids also `ids` [rows][w][n][dirs] int32: the entity each gather ray hit, -1 on a
        miss, -2 where the sample gathered nothing.  **kw as for run (stripes, seed).  ValueError for bad values and shapes, before the library
        is called; the definition is stated in include/gi_hip.h."""
        fp, sh, chain = final_gather_params(n=n, dirs=dirs, sh=sh, grid_box=grid_box, chain=chain, exponents=exponents, terms=terms, width=w, height=h)
        p = self.params(w, h, **kw)
        rows = self.local_rows(p)
        out, o = _out((rows, w, 12), f64)
        ids = np.zeros((rows, w, fp.baked.n_samples, fp.n_dirs), np.int32) if want_ids else None
        self._check(self.L.gi_render_final_gather_host(self.h, C.byref(p), C.byref(fp), _p(sh), _p(chain), *o, _p(ids, _ip)), "render_final_gather_host")
        res = {"final_gather": out, "beauty": out[:, :, 0:3], "direct": out[:, :, 3:6], "diffuse": out[:, :, 6:9], "specular": out[:, :, 9:12]}
        if want_ids:
            res["ids"] = ids
        return res

    def run_final_gather_device(self, p, fp, sh_ptr, chain_ptr, out_ptr, f64=False, ids_ptr=None):
        """The final-gather pass on device memory, asynchronous on the context's stream; p from params, fp from final_gather_params; sh_ptr
        ([nz][ny][nx][9][3] f64), chain_ptr (the whole chain, f64), out_ptr ([rows][w][12]) and ids_ptr ([rows][w][n][dirs] int32) are raw device
        pointers, None where they are not needed."""
        self._check(self.L.gi_render_final_gather_device(self.h, C.byref(p), C.byref(fp), sh_ptr or None, chain_ptr or None, *_dev(out_ptr, f64), ids_ptr or None),
                    "render_final_gather_device")

    def last_final_gather_ms(self):
        """gi_last_final_gather_ms: device time of the last final-gather pass (the frame's and the other passes' times keep theirs)."""
        return self._last_ms("final_gather")

    def run_baked_lightmap(self, w, h, n, atlas, ent, uv, filter="bilinear", sh=None, grid_box=None, chain=None, exponents=None, terms=None, f64=True, **kw):
        """The baked-light pass with a lightmap (gi_render_baked_lightmap_host; an addition, the reader of bake_lightmap's atlas): run_baked, except
        that a first hit on a diffuse surface whose entity has a row in the chart -- ent [n_chart], uv [n_chart][3][2], the chart the atlas
        [height][width][3] was baked for -- takes its irradiance from the atlas at the hit's chart coordinate, filtered "bilinear" or "nearest".  Diffuse
        hits on entities without a row read the probe grid sh if it is given and have no diffuse term otherwise.  terms: BAKED_* bits, default
        direct, diffuse and emissive, plus specular with a chain.  Returns the dict run_baked returns.  ValueError for bad values and shapes, before
        the library is called; the definition is stated in include/gi_hip.h."""
        bp, sh, chain = baked_params(n=n, sh=sh, grid_box=grid_box, chain=chain, exponents=exponents, terms=terms, width=w, height=h, lightmap=True)
        lp, atlas, e, c = baked_lightmap_params(atlas, ent, uv, filter)
        p = self.params(w, h, **kw)
        rows = self.local_rows(p)
        out, o = _out((rows, w, 12), f64)
        self._check(self.L.gi_render_baked_lightmap_host(self.h, C.byref(p), C.byref(bp), C.byref(lp), _p(sh), _p(chain), *_buf(atlas), _p(e, _ip), _p(c), *o),
                    "render_baked_lightmap_host")
        return {"baked": out, "beauty": out[:, :, 0:3], "direct": out[:, :, 3:6], "diffuse": out[:, :, 6:9], "specular": out[:, :, 9:12]}

    def run_baked_lightmap_device(self, p, bp, lp, sh_ptr, chain_ptr, atlas_ptr, ent_ptr, uv_ptr, out_ptr, f64=False):
        """The baked-light pass with a lightmap on device memory, asynchronous on the context's stream; p from params, bp from baked_params (with
        lightmap=True), lp from baked_lightmap_params; sh_ptr, chain_ptr, atlas_ptr ([height][width][3] f64), ent_ptr ([n_chart] int32), uv_ptr
        ([n_chart][3][2] f64) and out_ptr ([rows][w][12]) are raw device pointers, None where they are not needed.  The chart is not looked at."""
        self._check(self.L.gi_render_baked_lightmap_device(self.h, C.byref(p), C.byref(bp), C.byref(lp), sh_ptr or None, chain_ptr or None, atlas_ptr or None,
                                                           ent_ptr or None, uv_ptr or None, *_dev(out_ptr, f64)), "render_baked_lightmap_device")

    def probe_visibility_params(self, size=8, samples=16, max_dist=None, stream_base=0, seed=None):
        """gi_probe_visibility_params: texels per map edge, rays per texel, the distance a miss counts as (None: the diagonal of the scene's root
        box, or the library's 1e30 without a scene), the stream index of sample 0 of texel 0 of point 0, the seed (default: the tracer's)."""
        p = ProbeVisibilityParams()
        self.L.gi_probe_visibility_default_params(C.byref(p))
        p.size, p.n_samples, p.stream_base = int(size), int(samples), int(stream_base)
        p.seed = self._seed(seed)
        if max_dist is not None:
            p.max_dist = float(max_dist)
        elif self.scene is not None:
            b = self.scene.tables()["node_bbox"][0]
            p.max_dist = float(np.sqrt(((b[3] - b[0]) ** 2 + (b[4] - b[1]) ** 2) + (b[5] - b[2]) ** 2))
        return p

    def bake_probe_visibility(self, points, size=8, n_samples=16, max_dist=None, stream_base=0, seed=None, f64=True):
        """Probe visibility maps (gi_probe_visibility_host; an addition beside bake_probes): per point [n][3] an octahedral map of size x size
        texels holding the mean and the mean squared distance to the nearest surface over n_samples jittered rays per texel, distances cut at
        max_dist (None: the scene's diagonal), which is also what a miss counts as.  Returns [n][size][size][2]; octa_decode gives a texel's
        direction.  run_baked_visibility reads the maps of a probe grid (reshaped [nz][ny][nx][size][size][2]) so that probes behind a wall do
        not light a hit.  Sample k of texel t = (i * size + y) * size + x runs on stream stream_base + t * n_samples + k; the definition is
        stated in include/gi_hip.h."""
        pts = self._bake_points(points)
        p = self.probe_visibility_params(size, n_samples, max_dist, stream_base, seed)
        m = max(p.size, 0)
        out, o = _out((len(pts), m, m, 2), f64)
        self._check(self.L.gi_probe_visibility_host(self.h, _p(pts), len(pts), C.byref(p), *o), "probe_visibility_host")
        return out

    def probe_visibility_device(self, p, points_ptr, n_points, out_ptr, f64=False):
        """Probe visibility maps on device memory (raw device pointers: points [n][3] f64, out [n][size][size][2]); p from probe_visibility_params.
        The points are not looked at."""
        self._check(self.L.gi_probe_visibility_device(self.h, points_ptr, int(n_points), C.byref(p), *_dev(out_ptr, f64)), "probe_visibility_device")

    def last_probe_visibility_ms(self):
        """gi_last_probe_visibility_ms: device time of the last capture of visibility maps (the frame's and the other passes' times keep theirs)."""
        return self._last_ms("probe_visibility")

    def run_baked_visibility(self, w, h, n, vis, sh=None, grid_box=None, chain=None, exponents=None, terms=None, normal_bias=None, vis_floor=None, f64=True, **kw):
        """The baked-light pass with probe visibility (gi_render_baked_visibility_host; an addition, the reader of bake_probe_visibility's maps):
        run_baked, except that the eight probes around a diffuse hit are not interpolated trilinearly but weighted by the trilinear weight, a
        back-face term and a Chebyshev test of the hit (moved normal_bias along its normal) against each probe's map, never below vis_floor -- a
        probe on the far side of a wall counts for little.  vis [nz][ny][nx][M][M][2] for the grid of sh; None gives run_baked's result bit for
        bit.  Returns the dict run_baked returns.  ValueError for bad values and shapes, before the library is called; the definition is stated in
        include/gi_hip.h."""
        bp, sh, chain = baked_params(n=n, sh=sh, grid_box=grid_box, chain=chain, exponents=exponents, terms=terms, width=w, height=h)
        vp, vis = baked_visibility_params(vis, None if sh is None else sh.shape[:3], normal_bias, vis_floor)
        if vis is not None and sh is None:
            raise ValueError("baked_visibility: the maps belong to a probe grid, sh")
        p = self.params(w, h, **kw)
        rows = self.local_rows(p)
        out, o = _out((rows, w, 12), f64)
        v = _buf(vis) if vis is not None else (None, 1)
        self._check(self.L.gi_render_baked_visibility_host(self.h, C.byref(p), C.byref(bp), C.byref(vp), _p(sh), _p(chain), *v, *o), "render_baked_visibility_host")
        return {"baked": out, "beauty": out[:, :, 0:3], "direct": out[:, :, 3:6], "diffuse": out[:, :, 6:9], "specular": out[:, :, 9:12]}

    def run_baked_visibility_device(self, p, bp, vp, sh_ptr, chain_ptr, vis_ptr, out_ptr, f64=False):
        """The baked-light pass with probe visibility on device memory, asynchronous on the context's stream; p from params, bp from baked_params,
        vp from baked_visibility_params; sh_ptr, chain_ptr, vis_ptr ([nz][ny][nx][M][M][2] f64) and out_ptr ([rows][w][12]) are raw device
        pointers, None where they are not needed."""
        self._check(self.L.gi_render_baked_visibility_device(self.h, C.byref(p), C.byref(bp), C.byref(vp), sh_ptr or None, chain_ptr or None, vis_ptr or None,
                                                             *_dev(out_ptr, f64)), "render_baked_visibility_device")

    def bake_reflection_probes(self, positions, face, samples, levels=1, exponents=None, stream_base=0, seed=None):
        """The chains of a reflection probe set: bake_reflection_probe once per position [K][3], every chain concatenated as the library holds it.
        Returns [K][texels][3] float64, texels = the sum over the levels of 6 (face >> l)^2 -- the `chains` of run_baked_reflections."""
        pts = self._bake_points(positions)
        return np.ascontiguousarray(np.stack([np.concatenate([c.reshape(-1, 3) for c in self.bake_reflection_probe(q, face, samples, levels, exponents, stream_base, seed)])
                                              for q in pts])) if len(pts) else np.zeros((0, 0, 3))

    def _reflections_blocks(self, w, h, n, probes, chains, sh, grid_box, chain, exponents, terms, face, levels):
        """(gi_baked_params, gi_baked_reflections_params, sh, chain, probes, chains) of run_baked_reflections: a chain of the set's shape stands in
        for the one chain where baked_params checks face, levels and exponents; without a set the one chain is run_baked's."""
        rp, t, c, f, lv = baked_reflections_params(probes, chains)
        if t is None:
            bp, sh, chain = baked_params(n=n, sh=sh, grid_box=grid_box, chain=chain, exponents=exponents, terms=terms, width=w, height=h)
            return bp, rp, sh, chain, None, None
        if f is None:                                      # chains [K][texels][3]: the caller states the face; the levels follow from the texels
            if face is None:
                raise ValueError("baked_reflections: chains [K][texels][3] need face= (and levels=, if not 1)")
            f, lv = int(face), int(levels or 1)
        if f < 1 or not 1 <= lv <= CUBEMAP_MAX_LEVELS or f % (1 << (lv - 1)) or c.shape[1] != sum(6 * (f >> l) ** 2 for l in range(lv)):
            raise ValueError(f"baked_reflections: chains of {c.shape[1]} texels do not fit face {f} with {lv} levels")
        first = [np.zeros((6, f >> l, f >> l, 3)) for l in range(lv)]
        bp, sh, _ = baked_params(n=n, sh=sh, grid_box=grid_box, chain=first, exponents=exponents, terms=terms, width=w, height=h)
        return bp, rp, sh, None, t, c

    def run_baked_reflections(self, w, h, n, probes, chains, sh=None, grid_box=None, exponents=None, terms=None, f64=True, chain=None, face=None, levels=None, **kw):
        """The baked-light pass with a reflection probe set (gi_render_baked_reflections_host; an addition): run_baked, except that the specular
        term of a mirror or glossy first hit blends the probes whose influence boxes contain the hit, each probe's cube read in the direction
        from the probe to the point where the reflection ray leaves its box -- reflections line up with the walls they show, and every room
        shows its own.  A hit in no box reads the nearest probe as run_baked would.  probes [K][10] = pos, box_min, box_max, fade per probe
        (reflection_probe_cells); chains the K chains, a list of bake_reflection_probe results or bake_reflection_probes' [K][texels][3] (then
        with face= and levels=), filtered with `exponents`.  With probes None (or of no rows) the pass is run_baked's on `chain`, bit for bit;
        with a set, `chain` is not read.  Returns the dict run_baked returns.  ValueError for bad values and shapes, before
        the library is called; the definition is stated in include/gi_hip.h."""
        bp, rp, sh, chain, t, c = self._reflections_blocks(w, h, n, probes, chains, sh, grid_box, chain, exponents, terms, face, levels)
        p = self.params(w, h, **kw)
        rows = self.local_rows(p)
        out, o = _out((rows, w, 12), f64)
        self._check(self.L.gi_render_baked_reflections_host(self.h, C.byref(p), C.byref(bp), C.byref(rp), _p(sh), _p(chain), _p(t), _p(c), *o), "render_baked_reflections_host")
        return {"baked": out, "beauty": out[:, :, 0:3], "direct": out[:, :, 3:6], "diffuse": out[:, :, 6:9], "specular": out[:, :, 9:12]}

    def run_baked_reflections_device(self, p, bp, rp, sh_ptr, chain_ptr, probes_ptr, chains_ptr, out_ptr, f64=False):
        """The baked-light pass with a reflection probe set on device memory, asynchronous on the context's stream; p from params, bp from
        baked_params, rp from baked_reflections_params; sh_ptr, chain_ptr, probes_ptr ([K][10] f64), chains_ptr ([K][texels][3] f64) and out_ptr
        ([rows][w][12]) are raw device pointers, None where they are not needed.  The table is not looked at."""
        self._check(self.L.gi_render_baked_reflections_device(self.h, C.byref(p), C.byref(bp), C.byref(rp), sh_ptr or None, chain_ptr or None, probes_ptr or None,
                                                              chains_ptr or None, *_dev(out_ptr, f64)), "render_baked_reflections_device")

    def last_baked_ms(self):
        """gi_last_baked_ms: device time of the last baked-light pass, with a lightmap or without (the frame's and the other passes' times keep theirs)."""
        return self._last_ms("baked")

    def set_lens(self, radius=None, blades=None, rotation=None, lens=None):
        """gi_set_lens: the thin lens every pass of this context makes its primary rays through -- run (all render modes), progressive sessions,
        run_features, run_occlusion, run_upsampled.  radius in scene units (0: the pinhole), blades 3 .. 16, rotation in radians; or a Lens.  The
        plane focal_dist in front of the camera stays sharp (focus_at moves it).  ValueError for bad values, before the library is called; GiError
        (code -4) while a progressive session is open.  Returns self."""
        l = lens if lens is not None else lens_params(radius, blades, rotation)
        self._check(self.L.gi_set_lens(self.h, C.byref(l)), "set_lens")
        return self

    @property
    def lens(self):
        """gi_get_lens: the context's lens (radius 0, 6 blades, rotation 0 until set_lens)."""
        l = Lens()
        self._check(self.L.gi_get_lens(self.h, C.byref(l)), "get_lens")
        return l

    def focus_distance(self, w, h, x, y, **kw):
        """gi_focus_distance: the distance, along cam_forward, of the first surface behind the centre of pixel (x, y) of a w x h frame, seen through
        the pinhole; None on a miss.  focus_at(that) makes it the sharp plane."""
        p = self.params(w, h, **kw)
        d = C.c_double()
        rc = self._check(self.L.gi_focus_distance(self.h, C.byref(p), int(x), int(y), C.byref(d)), "focus_distance")
        return None if rc == 1 else d.value

    def focus_at(self, dist):
        """Move the sharp plane to `dist` in front of the camera: sensor_diag and focal_dist are both multiplied by dist / focal_dist, so the field
        of view is kept.  Returns self."""
        dist = float(dist)
        if not (0.0 < dist < float("inf")):
            raise ValueError(f"focus_at: the distance must be finite and > 0, got {dist}")
        k = dist / self.focal_dist
        self.sensor_diag, self.focal_dist = self.sensor_diag * k, self.focal_dist * k
        return self

    def run_upsampled(self, w, h, factor, feature_samples, denoise=False, f64=True, **kw):
        """A w x h frame from a (w / factor) x (h / factor) render: `run` at the reduced size with **kw (min_samples, max_samples, noise_thresh,
        seed; whole frames, so no stripes), `run_features` with feature_samples samples at both sizes, optionally `denoise` (default parameters) on
        the low frame, then `upsample` (default parameters).  factor must divide w and h (ValueError): only then does the reduced-size frame see
        the view of the full-size one."""
        if any(k in kw for k in ("stripe_h", "rank", "world")):
            raise ValueError("run_upsampled: whole frames only, no stripe keywords")
        wl, hl = low_frame_size(w, h, factor)
        low = self.run(wl, hl, f64=f64, **kw)
        fl = self.run_features(wl, hl, feature_samples, f64=f64, want_ids=False, **kw)
        ff = self.run_features(w, h, feature_samples, f64=f64, want_ids=False, **kw)
        if denoise:
            low = self.denoise(low, fl)
        return self.upsample(low, fl, ff, factor)

    def set_render_mode(self, mode):
        """'wavefront' (default), 'megakernel' or 'rounds' (the wavefront passes in synchronous rounds, fixed-spp frames too):
        schedules of the same per-path arithmetic."""
        self._check(self.L.gi_set_render_mode(self.h, {"wavefront": 0, "megakernel": 1, "rounds": 2}[mode]), "set_render_mode")

    def set_wide_nodes(self, on):
        """Octree walk over wide records (default) or one box test per node record; returns whether the wide walk is in use."""
        rc = self.L.gi_set_wide_nodes(self.h, 1 if on else 0)
        if rc < 0:
            self._check(rc, "set_wide_nodes")
        self.photon_planes = bool(rc & 2)      # the photon octree's one-record-per-level descent is in use
        return bool(rc & 1)

    def set_content_culling(self, on):
        """Skip children of the octree walk in whose sub-tree the ray cannot hit anything (default on); returns whether it is in use."""
        return bool(self._check(self.L.gi_set_content_culling(self.h, 1 if on else 0), "set_content_culling"))

    def set_entity_boxes(self, on):
        """Run the entity tests of a leaf only on the references whose own box the ray touches (default on); returns whether it is in use."""
        return bool(self._check(self.L.gi_set_entity_boxes(self.h, 1 if on else 0), "set_entity_boxes"))

    def set_pool_slots(self, slots):
        self._check(self.L.gi_set_pool_slots(self.h, int(slots)), "set_pool_slots")

    def last_render_ms(self):
        ms, n = C.c_float(), C.c_int32()
        self._check(self.L.gi_last_render_ms(self.h, C.byref(ms), C.byref(n)), "last_render_ms")
        return ms.value, n.value

    STAGES = ("regen", "trace", "shade", "sort", "gather", "finish", "accum", "other")

    def last_stage_ms(self):
        out = (C.c_float * 8)()
        self._check(self.L.gi_last_stage_ms(self.h, out), "last_stage_ms")
        return dict(zip(self.STAGES, [float(v) for v in out]))

    KERNELS = ("regen", "trace", "shade", "sort", "gather", "finish", "accum", "other", "shadow", "reserved")

    def last_kernel_ms(self):
        """gi_last_kernel_ms: device time of the last frame per kernel family ('shade' = k_st_shade alone, 'shadow' = k_st_shadow)."""
        out = (C.c_float * 10)()
        self._check(self.L.gi_last_kernel_ms(self.h, out), "last_kernel_ms")
        return {k: float(v) for k, v in zip(self.KERNELS, out) if k != "reserved"}

    def set_counters(self, mode):
        """0 / False: off; 1 / True: the reference's visits (megakernel, per-node walk); 2 or "stream": what the streaming kernels execute."""
        m = {"stream": 2, True: 1, False: 0}.get(mode, mode)
        self._check(self.L.gi_set_counters(self.h, int(m)), "set_counters")

    STREAM_COUNTERS = ("trace_walks", "trace_records", "trace_child_boxes", "trace_content_boxes", "trace_leaves", "trace_tris", "trace_rays",
                       "shadow_walks", "shadow_records", "shadow_child_boxes", "shadow_content_boxes", "shadow_leaves", "shadow_tris", "shadow_rays",
                       "gather_queries", "gather_candidates", "shaded", "trace_entity_boxes", "shadow_entity_boxes")

    def stream_counters(self):
        """gi_get_stream_counters: the executed work of the last frame rendered with set_counters("stream"), as a dict."""
        out = (C.c_int64 * 19)()
        self._check(self.L.gi_get_stream_counters(self.h, out), "get_stream_counters")
        return dict(zip(self.STREAM_COUNTERS, [int(v) for v in out]))

    def counters(self):
        out = (C.c_int64 * 8)()
        self._check(self.L.gi_get_counters(self.h, out), "get_counters")
        return np.array(list(out), np.int64)
