"""gi_raytracer_amd -- Python host mirror of the MI355X render hot path of GI_Raytracer.

Thin ctypes binding over the C ABI (include/gi_hip.h, gi_raytracer_amd/csrc/gi_host.h) of libgi_raytracer_hip.so.
The names mirror the reference's C++ surface for this path: `Scene` plays Octree (+ the loaders that fill it),
`RayTracer` plays RayTracer (setScene / run / trace / visible / samplePhotons / tracePhotons).  There is no CPU
implementation behind these classes: creating a RayTracer without the HIP library or without a GPU raises.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# The product library, in-tree.  An experimental build of the same library (tools/build_exp.sh -> exp/*.so) is loaded instead only when
# BOTH GI_EXPERIMENTAL=1 and GI_LIB_PATH are set (the tuning scripts under tools/ set them); bench.py prints the path it resolved.
LIB_PATH = os.path.join(_HERE, "libgi_raytracer_hip.so")
if os.environ.get("GI_EXPERIMENTAL") == "1" and os.environ.get("GI_LIB_PATH"):
    LIB_PATH = os.environ["GI_LIB_PATH"]
DEFAULT_SEED = 0x9E3779B97F4A7C15

GI_OK, GI_E_NO_DEVICE, GI_E_INVALID, GI_E_HIP, GI_E_STATE, GI_E_CANCELLED = 0, -1, -2, -3, -4, -5

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)
_up = C.POINTER(C.c_uint32)


class GiError(RuntimeError):
    pass


class SceneDesc(C.Structure):
    _fields_ = [("n_tri", C.c_int32), ("tri_pos", _dp), ("tri_nrm", _dp), ("tri_uv", _dp), ("tri_mat", _ip),
                ("n_mat", C.c_int32), ("mats", _dp), ("n_light", C.c_int32), ("lights", _dp), ("ambient", C.c_double * 3),
                ("n_node", C.c_int32), ("node_bbox", _dp), ("node_child", _ip), ("node_ent_off", _ip), ("node_ent_idx", _ip),
                ("ent_kind", _ip), ("n_fog", C.c_int32), ("fog", _dp), ("fog_grid_off", _ip), ("fog_grid", _dp),
                ("n_tex", C.c_int32), ("tex_kind", _ip), ("tex_param", _dp), ("mat_tex", _ip), ("tex_pixels", C.POINTER(C.c_uint8)),
                ("n_tex_pixel_bytes", C.c_int64)]


class PhotonMapDesc(C.Structure):
    _fields_ = [("n_photon", C.c_int32), ("photons", _dp), ("n_node", C.c_int32), ("node_bbox", _dp), ("node_child", _ip),
                ("node_off", _ip), ("node_idx", _ip)]


class RenderParams(C.Structure):
    _fields_ = [("cam_pos", C.c_double * 3), ("cam_up", C.c_double * 3), ("cam_forward", C.c_double * 3),
                ("sensor_diag", C.c_double), ("focal_dist", C.c_double), ("width", C.c_int32), ("height", C.c_int32),
                ("stripe_h", C.c_int32), ("stripe_rank", C.c_int32), ("stripe_world", C.c_int32),
                ("min_samples", C.c_int32), ("max_samples", C.c_int32), ("noise_thresh", C.c_double), ("seed", C.c_uint64)]


class DenoiseParams(C.Structure):
    """gi_denoise_params (include/gi_hip.h)."""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("iterations", C.c_int32), ("demodulate", C.c_int32),
                ("sigma_color", C.c_double), ("sigma_normal", C.c_double), ("sigma_depth", C.c_double), ("sigma_albedo", C.c_double)]


class UpsampleParams(C.Structure):
    """gi_upsample_params (include/gi_hip.h)."""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("low_width", C.c_int32), ("low_height", C.c_int32), ("factor", C.c_int32),
                ("demodulate", C.c_int32), ("sigma_normal", C.c_double), ("sigma_depth", C.c_double), ("sigma_albedo", C.c_double)]


class OcclusionParams(C.Structure):
    """gi_occlusion_params (include/gi_hip.h)."""
    _fields_ = [("n_samples", C.c_int32), ("n_dirs", C.c_int32), ("radius", C.c_double)]


class Lens(C.Structure):
    """gi_lens (include/gi_hip.h): the thin lens of a context; radius 0 is the pinhole."""
    _fields_ = [("radius", C.c_double), ("rotation", C.c_double), ("blades", C.c_int32), ("reserved", C.c_int32)]


class BakeParams(C.Structure):
    """gi_bake_params (include/gi_hip.h)."""
    _fields_ = [("mode", C.c_int32), ("n_samples", C.c_int32), ("stream_base", C.c_uint32), ("seed", C.c_uint64)]


BAKE_TEXEL, BAKE_SH9 = 0, 1


class LightmapParams(C.Structure):
    """gi_lightmap_params (include/gi_hip.h)."""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("n_samples", C.c_int32), ("dilate", C.c_int32), ("flip", C.c_int32),
                ("stream_base", C.c_uint32), ("seed", C.c_uint64)]


class Settings(C.Structure):
    _fields_ = [("photons", C.c_int32), ("photon_depth", C.c_int32), ("min_samples", C.c_int32), ("max_samples", C.c_int32),
                ("noise_thresh", C.c_double), ("ambient", C.c_double * 3), ("cam_pos", C.c_double * 3), ("cam_up", C.c_double * 3),
                ("cam_forward", C.c_double * 3), ("sensor_diag", C.c_double), ("focal_dist", C.c_double)]


_LIB = None

# every symbol include/gi_hip.h and csrc/gi_host.h declare (tests check the library exports all of them)
ABI_SYMBOLS = [
    "gi_create", "gi_destroy", "gi_last_error", "gi_set_stream", "gi_upload_scene", "gi_upload_photons", "gi_local_rows",
    "gi_render_device", "gi_render_host", "gi_render_features_device", "gi_render_features_host", "gi_last_features_ms",
    "gi_denoise_default_params", "gi_denoise_device", "gi_denoise_host", "gi_last_denoise_ms",
    "gi_upsample_default_params", "gi_upsample_device", "gi_upsample_host", "gi_last_upsample_ms",
    "gi_occlusion_default_params", "gi_render_occlusion_device", "gi_render_occlusion_host", "gi_last_occlusion_ms", "gi_set_render_mode", "gi_set_wide_nodes", "gi_set_content_culling", "gi_set_entity_boxes", "gi_set_pool_slots", "gi_last_render_ms", "gi_last_stage_ms", "gi_last_kernel_ms", "gi_set_counters", "gi_get_counters", "gi_get_stream_counters", "gi_trace", "gi_visible",
    "gi_gather", "gi_radiance", "gi_emit_photons", "gi_halton_sample", "gi_halton_index", "gi_debug_leaf_order", "gi_debug_sort_pairs", "gi_debug_find_leaves", "gi_debug_gather_pass", "gi_debug_walk", "gi_kat", "gi_visible_rays", "gi_build_photon_map", "gi_trace_photons", "gi_debug_photon_tables", "gi_clear_photons", "gi_group_clear_photons",
    "gi_progressive_begin", "gi_progressive_step_device", "gi_progressive_step_host", "gi_progressive_status", "gi_progressive_state_bytes",
    "gi_progressive_save", "gi_progressive_restore", "gi_progressive_end",
    "gi_lens_default", "gi_set_lens", "gi_get_lens", "gi_lens_vertices", "gi_group_set_lens", "gi_debug_primary_rays", "gi_focus_distance",
    "gi_bake_default_params", "gi_bake_device", "gi_bake_host", "gi_last_bake_ms", "gi_bake_rays", "gi_bake_fold",
    "gi_lightmap_default_params", "gi_lightmap_host", "gi_lightmap_device", "gi_last_lightmap_ms", "gi_lightmap_texels", "gi_lightmap_dilate",
    "gi_device_count", "gi_group_create", "gi_group_destroy", "gi_group_size", "gi_group_ctx", "gi_group_last_error", "gi_group_upload_scene", "gi_group_upload_photons", "gi_group_render_host", "gi_group_render_device",
    "gih_scene_create", "gih_scene_destroy", "gih_last_error", "gih_load_scn", "gih_add_material", "gih_add_triangles",
    "gih_add_texture", "gih_add_material_tex", "gih_load_png", "gih_free",
    "gih_add_light", "gih_add_sphere", "gih_add_height_fog", "gih_set_ambient", "gih_get_settings", "gih_set_camera", "gih_build_octree", "gih_get_scene_desc",
    "gih_counts", "gih_build_photon_map", "gih_get_photon_desc", "gih_to_rgb8", "gih_entity_bbox", "gih_entity_overlaps_box", "gih_box_mesh", "gih_fog_grid", "gih_build_photon_map_in_box", "gih_add_height_fog_grid", "gih_load_obj",
]


def lib():
    """Load libgi_raytracer_hip.so (built by __graft_entry__.build() / csrc/Makefile).  Raises if it is missing."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise GiError(f"{LIB_PATH} not built: run `python -c 'import __graft_entry__ as g; g.build()'` (hipcc, gfx950)")
    L = C.CDLL(LIB_PATH)
    vp = C.c_void_p
    L.gi_create.argtypes = [C.POINTER(vp), C.c_int]
    L.gi_destroy.argtypes = [vp]
    L.gi_last_error.argtypes = [vp]
    L.gi_last_error.restype = C.c_char_p
    L.gi_set_stream.argtypes = [vp, vp]
    L.gi_upload_scene.argtypes = [vp, C.POINTER(SceneDesc)]
    L.gi_upload_photons.argtypes = [vp, C.POINTER(PhotonMapDesc)]
    L.gi_local_rows.argtypes = [C.POINTER(RenderParams)]
    L.gi_render_device.argtypes = [vp, C.POINTER(RenderParams), vp, C.c_int, vp, vp]
    L.gi_render_host.argtypes = [vp, C.POINTER(RenderParams), vp, C.c_int, vp, vp]
    L.gi_render_features_device.argtypes = [vp, C.POINTER(RenderParams), C.c_int32, vp, C.c_int, vp]
    L.gi_render_features_host.argtypes = [vp, C.POINTER(RenderParams), C.c_int32, vp, C.c_int, vp]
    L.gi_last_features_ms.argtypes = [vp, C.POINTER(C.c_float)]
    L.gi_denoise_default_params.argtypes = [C.POINTER(DenoiseParams)]
    L.gi_denoise_default_params.restype = None
    L.gi_denoise_device.argtypes = [vp, C.POINTER(DenoiseParams), vp, C.c_int, vp, C.c_int, vp, C.c_int]
    L.gi_denoise_host.argtypes = [vp, C.POINTER(DenoiseParams), vp, C.c_int, vp, C.c_int, vp, C.c_int]
    L.gi_last_denoise_ms.argtypes = [vp, C.POINTER(C.c_float)]
    L.gi_upsample_default_params.argtypes = [C.POINTER(UpsampleParams)]
    L.gi_upsample_default_params.restype = None
    L.gi_upsample_device.argtypes = [vp, C.POINTER(UpsampleParams), vp, C.c_int, vp, C.c_int, vp, C.c_int, vp, C.c_int]
    L.gi_upsample_host.argtypes = [vp, C.POINTER(UpsampleParams), vp, C.c_int, vp, C.c_int, vp, C.c_int, vp, C.c_int]
    L.gi_last_upsample_ms.argtypes = [vp, C.POINTER(C.c_float)]
    L.gi_occlusion_default_params.argtypes = [C.POINTER(OcclusionParams)]
    L.gi_occlusion_default_params.restype = None
    L.gi_render_occlusion_device.argtypes = [vp, C.POINTER(RenderParams), C.POINTER(OcclusionParams), vp, C.c_int]
    L.gi_render_occlusion_host.argtypes = [vp, C.POINTER(RenderParams), C.POINTER(OcclusionParams), vp, C.c_int]
    L.gi_last_occlusion_ms.argtypes = [vp, C.POINTER(C.c_float)]
    L.gi_set_render_mode.argtypes = [vp, C.c_int]
    L.gi_set_wide_nodes.argtypes = [vp, C.c_int]
    L.gi_set_content_culling.argtypes = [vp, C.c_int]
    L.gi_set_entity_boxes.argtypes = [vp, C.c_int]
    L.gi_set_pool_slots.argtypes = [vp, C.c_int64]
    L.gi_last_render_ms.argtypes = [vp, C.POINTER(C.c_float), _ip]
    L.gi_last_stage_ms.argtypes = [vp, C.POINTER(C.c_float)]
    L.gi_last_kernel_ms.argtypes = [vp, C.POINTER(C.c_float)]
    L.gi_set_counters.argtypes = [vp, C.c_int]
    L.gi_get_counters.argtypes = [vp, C.POINTER(C.c_int64)]
    L.gi_get_stream_counters.argtypes = [vp, C.POINTER(C.c_int64)]
    L.gi_trace.argtypes = [vp, C.c_int32, _dp, _ip, _ip, _dp]
    L.gi_visible.argtypes = [vp, C.c_int32, _dp, _ip]
    L.gi_gather.argtypes = [vp, C.c_int32, _dp, _dp, _ip]
    L.gi_radiance.argtypes = [vp, C.c_int32, _dp, _up, C.c_uint64, _dp]
    L.gi_emit_photons.argtypes = [vp, C.c_int32, C.c_int32, C.c_uint64, _dp, C.c_int32, C.POINTER(C.c_int64)]
    L.gi_halton_sample.argtypes = [vp, C.c_int32, _up, _up, C.POINTER(C.c_float)]
    L.gi_halton_index.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, _up, _up]
    L.gi_debug_leaf_order.argtypes = [vp, C.c_int32, _dp, C.c_int32, _ip, _ip]
    L.gi_debug_sort_pairs.argtypes = [vp, C.c_int32, _up, _up, C.c_int32, C.c_int32, _up, _up]
    L.gi_debug_find_leaves.argtypes = [vp, C.c_int32, _dp, _ip, _ip]
    L.gi_debug_gather_pass.argtypes = [vp, C.c_int32, _dp, C.c_int32, C.c_int32, _dp, _up, _up, C.POINTER(C.c_int64)]
    L.gi_debug_walk.argtypes = [vp, C.c_int32, _dp, _dp, C.c_int32, C.c_int32, _ip, _ip, _dp]
    L.gi_visible_rays.argtypes = [vp, C.c_int32, _dp, _dp, _ip]
    L.gi_kat.argtypes = [vp, C.c_int32, C.c_int32, _dp, C.c_int32, _dp]
    L.gi_clear_photons.argtypes = [vp]
    L.gi_group_clear_photons.argtypes = [vp]
    L.gi_build_photon_map.argtypes = [vp, C.c_int32, _dp, _dp]
    L.gi_trace_photons.argtypes = [vp, C.c_int32, C.c_int32, C.c_uint64, _dp, C.POINTER(C.c_int64)]
    L.gi_debug_photon_tables.argtypes = [vp, _ip, _ip, _ip, vp, _ip, _dp, _dp]
    L.gi_progressive_begin.argtypes = [vp, C.POINTER(RenderParams)]
    L.gi_progressive_step_device.argtypes = [vp, C.c_int32, vp, C.c_int, vp, vp]
    L.gi_progressive_step_host.argtypes = [vp, C.c_int32, vp, C.c_int, vp, vp]
    L.gi_progressive_status.argtypes = [vp, _ip, C.POINTER(C.c_int64)]
    L.gi_progressive_state_bytes.argtypes = [vp, C.POINTER(C.c_int64)]
    L.gi_progressive_save.argtypes = [vp, vp, C.c_int64]
    L.gi_progressive_restore.argtypes = [vp, vp, C.c_int64]
    L.gi_progressive_end.argtypes = [vp]
    L.gi_lens_default.argtypes = [C.POINTER(Lens)]
    L.gi_lens_default.restype = None
    L.gi_set_lens.argtypes = [vp, C.POINTER(Lens)]
    L.gi_get_lens.argtypes = [vp, C.POINTER(Lens)]
    L.gi_lens_vertices.argtypes = [C.POINTER(Lens), _dp]
    L.gi_group_set_lens.argtypes = [vp, C.POINTER(Lens)]
    L.gi_debug_primary_rays.argtypes = [vp, C.POINTER(RenderParams), C.c_int32, _up, _dp]
    L.gi_focus_distance.argtypes = [vp, C.POINTER(RenderParams), C.c_int32, C.c_int32, _dp]
    L.gi_bake_default_params.argtypes = [C.POINTER(BakeParams)]
    L.gi_bake_default_params.restype = None
    L.gi_bake_device.argtypes = [vp, vp, C.c_int32, C.POINTER(BakeParams), vp, C.c_int]
    L.gi_bake_host.argtypes = [vp, _dp, C.c_int32, C.POINTER(BakeParams), vp, C.c_int]
    L.gi_last_bake_ms.argtypes = [vp, C.POINTER(C.c_float)]
    L.gi_bake_rays.argtypes = [vp, _dp, C.c_int32, C.POINTER(BakeParams), _dp, _up]
    L.gi_bake_fold.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, _dp, _dp, _dp]
    L.gi_lightmap_default_params.argtypes = [C.POINTER(LightmapParams)]
    L.gi_lightmap_default_params.restype = None
    L.gi_lightmap_host.argtypes = [vp, C.POINTER(LightmapParams), C.c_int32, _ip, _dp, vp, C.c_int, _ip, _ip]
    L.gi_lightmap_device.argtypes = [vp, C.POINTER(LightmapParams), C.c_int32, vp, vp, vp, C.c_int, vp, _ip]
    L.gi_last_lightmap_ms.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.gi_lightmap_texels.argtypes = [vp, C.POINTER(LightmapParams), C.c_int32, _ip, _dp, _ip, _ip, _dp, _ip, C.c_int32]
    L.gi_lightmap_dilate.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, _dp, _ip, _dp]
    L.gi_group_create.argtypes = [C.POINTER(vp), C.c_int32, _ip]
    L.gi_group_destroy.argtypes = [vp]
    L.gi_group_size.argtypes = [vp]
    L.gi_group_ctx.argtypes = [vp, C.c_int32]
    L.gi_group_ctx.restype = vp
    L.gi_group_last_error.argtypes = [vp]
    L.gi_group_last_error.restype = C.c_char_p
    L.gi_group_upload_scene.argtypes = [vp, C.POINTER(SceneDesc)]
    L.gi_group_upload_photons.argtypes = [vp, C.POINTER(PhotonMapDesc)]
    L.gi_group_render_host.argtypes = [vp, C.POINTER(RenderParams), C.c_int32, C.c_int32, C.c_int32, vp, C.c_int, vp, vp]
    L.gi_group_render_device.argtypes = [vp, C.POINTER(RenderParams), C.c_int32, vp, C.c_int, vp]
    L.gih_scene_create.restype = vp
    L.gih_scene_destroy.argtypes = [vp]
    L.gih_last_error.argtypes = [vp]
    L.gih_last_error.restype = C.c_char_p
    L.gih_load_scn.argtypes = [vp, C.c_char_p]
    L.gih_add_material.argtypes = [vp, _dp]
    L.gih_add_texture.argtypes = [vp, C.c_int32, _dp, C.POINTER(C.c_uint8), C.c_int64]
    L.gih_add_material_tex.argtypes = [vp, C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_double]
    L.gih_load_png.argtypes = [C.c_char_p, _ip, _ip, _ip, C.POINTER(C.POINTER(C.c_uint8)), C.c_char_p, C.c_int32]
    L.gih_free.argtypes = [vp]
    L.gih_add_triangles.argtypes = [vp, C.c_int32, _dp, _dp, _dp, _ip]
    L.gih_add_light.argtypes = [vp, _dp, _dp, C.c_double]
    L.gih_add_sphere.argtypes = [vp, _dp, C.c_double, C.c_int32]
    L.gih_add_height_fog.argtypes = [vp, _dp, _dp, C.c_int32, C.c_uint64]
    L.gih_set_ambient.argtypes = [vp, _dp]
    L.gih_get_settings.argtypes = [vp, C.POINTER(Settings)]
    L.gih_set_camera.argtypes = [vp, _dp, _dp]
    L.gih_build_octree.argtypes = [vp]
    L.gih_get_scene_desc.argtypes = [vp, C.POINTER(SceneDesc)]
    L.gih_counts.argtypes = [vp, _ip, _ip, _ip, _ip, _ip]
    L.gih_build_photon_map.argtypes = [vp, C.c_int32, _dp]
    L.gih_get_photon_desc.argtypes = [vp, C.POINTER(PhotonMapDesc)]
    L.gih_to_rgb8.argtypes = [vp, C.c_int32, C.c_int64, C.POINTER(C.c_uint8)]
    _LIB = L
    return L


def _f64(a):
    return np.ascontiguousarray(a, np.float64)


def _p(a, ty=_dp):
    return a.ctypes.data_as(ty) if a is not None else None


def _np_from(ptr, shape, dtype):
    n = int(np.prod(shape))
    if n == 0:
        return np.zeros(shape, dtype)
    return np.ctypeslib.as_array(ptr, shape=(n,)).reshape(shape).copy()


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
        rc = self.L.gih_add_texture(self.h, kind, _p(par), pixels.ctypes.data_as(C.POINTER(C.c_uint8)) if pixels is not None else None,
                                    len(pixels) if pixels is not None else 0)
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
        if self.L.gih_add_height_fog(self.h, _p(par), _p(g), 0 if g is None else len(g), C.c_uint64(seed)) != 0:
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


def halton_sample_cap(w, h):
    """Samples per pixel a w x h frame can take before the Halton index leaves 32 bits: index = offset + s * inc with offset < inc = 2^a 3^b,
    the smallest such powers >= w and >= h (Halton_enum, include/halton_enum.h:69-114)."""
    pw, ph = 1, 1
    while pw < w:
        pw *= 2
    while ph < h:
        ph *= 3
    return (1 << 32) // (pw * ph)


def to_rgb8(lin):
    """The reference's display transform: gamma 2.2, clamp to [0, 1], truncating (int)(255 c) (include/raytracer.h:150-157, image.h:15)."""
    a = np.asarray(lin)
    a = np.ascontiguousarray(a, np.float32 if a.dtype == np.float32 else np.float64)
    out = np.zeros(a.shape, np.uint8)
    if lib().gih_to_rgb8(a.ctypes.data_as(C.c_void_p), 1 if a.dtype == np.float64 else 0, a.size, out.ctypes.data_as(C.POINTER(C.c_uint8))) != 0:
        raise GiError("to_rgb8: invalid arguments")
    return out


def save_ppm(path, lin):
    a = to_rgb8(lin)
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (a.shape[1], a.shape[0]))
        f.write(a.tobytes())


def probe_grid(box6, nx, ny, nz):
    """A regular grid of probe positions inside the box (min xyz, max xyz): the centres of its nx x ny x nz cells, [nz][ny][nx][3]."""
    b = np.asarray(box6, np.float64).reshape(6)
    ax = [b[k] + (np.arange(n) + 0.5) * ((b[3 + k] - b[k]) / n) for k, n in enumerate((int(nx), int(ny), int(nz)))]
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    return np.ascontiguousarray(np.stack([x, y, z], -1))


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


UPSAMPLE_FACTORS = range(2, 9)


def low_frame_size(w, h, factor):
    """(w / factor, h / factor): the size of the render RayTracer.run_upsampled scales up.  ValueError unless factor is 2 .. 8 and divides both."""
    w, h, factor = int(w), int(h), int(factor)
    if factor not in UPSAMPLE_FACTORS:
        raise ValueError(f"upsample: factor must be {UPSAMPLE_FACTORS[0]} .. {UPSAMPLE_FACTORS[-1]}, got {factor}")
    if w < 1 or h < 1 or w % factor or h % factor:
        raise ValueError(f"upsample: factor {factor} does not divide the frame size {w} x {h}")
    return w // factor, h // factor


def _filter_array(a):
    """An input of denoise / upsample as a contiguous float32 or float64 array; of a dict of run_features, its features."""
    a = np.asarray(a["features"] if isinstance(a, dict) else a)
    return np.ascontiguousarray(a, np.float32 if a.dtype == np.float32 else np.float64)


def _fill_params(p, kw, ints, floats, what):
    """Sets the fields of p that kw names: those in `ints` as int, those in `floats` as float; TypeError for any other name."""
    for k, v in kw.items():
        if k not in ints + floats:
            raise TypeError(f"{what}: unknown parameter {k!r}")
        setattr(p, k, int(v) if k in ints else float(v))
    return p


def upsample_arrays(low_color, low_features, features, factor):
    """The three inputs of RayTracer.upsample as contiguous float32 / float64 arrays (dicts of run_features are accepted for the features);
    ValueError unless low_color is [hl][wl][3], low_features [hl][wl][8], features [h][w][8] with wl = ceil(w / factor), hl = ceil(h / factor)."""
    low_color, low_features, features = _filter_array(low_color), _filter_array(low_features), _filter_array(features)
    factor = int(factor)
    if factor not in UPSAMPLE_FACTORS:
        raise ValueError(f"upsample: factor must be {UPSAMPLE_FACTORS[0]} .. {UPSAMPLE_FACTORS[-1]}, got {factor}")
    if features.ndim != 3 or features.shape[2] != 8 or features.shape[0] < 1 or features.shape[1] < 1:
        raise ValueError(f"upsample: features [h][w][8] expected, got {features.shape}")
    h, w = features.shape[:2]
    hl, wl = -(-h // factor), -(-w // factor)
    if low_color.shape != (hl, wl, 3) or low_features.shape != (hl, wl, 8):
        raise ValueError(f"upsample: a {w} x {h} frame at factor {factor} takes low_color [{hl}][{wl}][3] and low_features [{hl}][{wl}][8], "
                         f"got {low_color.shape} and {low_features.shape}")
    return low_color, low_features, features


OCCLUSION_MAX_DIRS = 64


def occlusion_params(n=None, dirs=None, radius=None, width=None, height=None):
    """gi_occlusion_default_params (16 samples, 16 directions, radius 0 = a tenth of the scene box's diagonal) with any of n, dirs, radius set.
    No device needed.  ValueError for what the library would refuse: n < 1 (or, when the frame size is given, beyond halton_sample_cap(width,
    height)), dirs outside 1 .. 64, a negative, NaN or infinite radius."""
    p = OcclusionParams()
    lib().gi_occlusion_default_params(C.byref(p))
    if n is not None:
        p.n_samples = _whole("n", n)
    if dirs is not None:
        p.n_dirs = _whole("dirs", dirs)
    if radius is not None:
        radius = float(radius)
        if not (0.0 <= radius < float("inf")):
            raise ValueError(f"occlusion: radius must be finite and >= 0 (0: a tenth of the scene box's diagonal), got {radius}")
        p.radius = radius
    if p.n_samples < 1:
        raise ValueError(f"occlusion: n must be at least 1, got {p.n_samples}")
    if width is not None and height is not None and p.n_samples > halton_sample_cap(width, height):
        raise ValueError(f"occlusion: n = {p.n_samples} takes the Halton index of a {width} x {height} frame beyond 32 bits "
                         f"(at most {halton_sample_cap(width, height)})")
    if not 1 <= p.n_dirs <= OCCLUSION_MAX_DIRS:
        raise ValueError(f"occlusion: dirs must be 1 .. {OCCLUSION_MAX_DIRS}, got {p.n_dirs}")
    return p


def _whole(name, v, what="occlusion"):
    """An integer argument of occlusion_params / lens_params: ValueError for anything that is not a whole number an int32 holds."""
    try:
        i = int(v)
    except (TypeError, ValueError, OverflowError):
        raise ValueError(f"{what}: {name} must be a whole number, got {v!r}") from None
    if i != v or not -2 ** 31 <= i < 2 ** 31:
        raise ValueError(f"{what}: {name} must be a whole number, got {v!r}")
    return i


LENS_BLADES = range(3, 17)


def lens_params(radius=None, blades=None, rotation=None):
    """gi_lens_default (radius 0 = the pinhole, 6 blades, rotation 0) with any of radius (scene units), blades, rotation (radians) set.  No device
    needed.  ValueError for what gi_set_lens would refuse: a negative, NaN or infinite radius, blades outside 3 .. 16, a rotation that is not finite."""
    l = Lens()
    lib().gi_lens_default(C.byref(l))
    if radius is not None:
        try:
            radius = float(radius)
        except (TypeError, ValueError):
            raise ValueError(f"lens: radius must be a number, got {radius!r}") from None
        if not (0.0 <= radius < float("inf")):
            raise ValueError(f"lens: radius must be finite and >= 0 (0: the pinhole), got {radius}")
        l.radius = radius
    if blades is not None:
        l.blades = _whole("blades", blades, "lens")
    if rotation is not None:
        try:
            rotation = float(rotation)
        except (TypeError, ValueError):
            raise ValueError(f"lens: rotation must be a number, got {rotation!r}") from None
        if not (-float("inf") < rotation < float("inf")):
            raise ValueError(f"lens: rotation must be finite (radians), got {rotation}")
        l.rotation = rotation
    if l.blades not in LENS_BLADES:
        raise ValueError(f"lens: blades must be {LENS_BLADES[0]} .. {LENS_BLADES[-1]}, got {l.blades}")
    return l


def lens_vertices(lens):
    """gi_lens_vertices: the aperture polygon's unit vertices [blades + 1][2] as the kernels read them (the last a copy of the first).  No device."""
    xy = np.zeros((lens.blades + 1 if 0 <= lens.blades <= 64 else 1, 2))
    if lib().gi_lens_vertices(C.byref(lens), _p(xy)) != GI_OK:
        raise ValueError("lens_vertices: not a lens gi_set_lens accepts")
    return xy


def lens_tag(lens):
    """The lens tag of a checkpoint header (include/gi_hip.h): 0 for a pinhole, else the low 32 bits of 64-bit FNV-1a over the 24 bytes of gi_lens,
    0 replaced by 1."""
    if not lens.radius > 0:
        return 0
    h = 0xcbf29ce484222325
    for b in bytes(lens):
        h = ((h ^ b) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return (h & 0xFFFFFFFF) or 1


# The header of a progressive checkpoint (include/gi_hip.h: gi_progressive_save), little-endian, 192 bytes; the 72-byte pixel records follow.
CHECKPOINT_MAGIC = b"GIPROGR\0"
CHECKPOINT_VERSION = 1
CHECKPOINT_HEADER = "<8sII11d7i4xdQiiQIIiiiI"
CHECKPOINT_RECORD_BYTES = 72
_CHECKPOINT_FIELDS = ("width", "height", "stripe_h", "stripe_rank", "stripe_world", "min_samples", "max_samples", "noise_thresh", "seed",
                      "schedule", "sample_end", "n_records", "record_bytes", "reserved0", "n_entity", "n_node", "n_photon", "lens_tag")


def parse_checkpoint_header(blob):
    """The fields of a checkpoint's header as a dict (no device needed); ValueError when the blob is not a checkpoint of this format."""
    import struct
    n = struct.calcsize(CHECKPOINT_HEADER)
    if len(blob) < n:
        raise ValueError(f"checkpoint: {len(blob)} bytes, the header alone has {n}")
    v = struct.unpack(CHECKPOINT_HEADER, bytes(blob[:n]))
    if v[0] != CHECKPOINT_MAGIC:
        raise ValueError("checkpoint: bad magic")
    h = {"magic": v[0], "version": v[1], "header_bytes": v[2], "cam_pos": v[3:6], "cam_up": v[6:9], "cam_forward": v[9:12],
         "sensor_diag": v[12], "focal_dist": v[13]}
    h.update(zip(_CHECKPOINT_FIELDS, v[14:]))
    h["reserved1"] = h["lens_tag"]      # the field's name before it became the lens tag
    if h["version"] != CHECKPOINT_VERSION or h["header_bytes"] != n or h["record_bytes"] != CHECKPOINT_RECORD_BYTES:
        raise ValueError(f"checkpoint: version {h['version']}, header {h['header_bytes']} bytes, records of {h['record_bytes']} bytes: not this format")
    if len(blob) != n + h["n_records"] * CHECKPOINT_RECORD_BYTES:
        raise ValueError(f"checkpoint: {len(blob)} bytes, {n + h['n_records'] * CHECKPOINT_RECORD_BYTES} expected (truncated?)")
    return h


class ProgressiveRender:
    """A progressive render session of a RayTracer (gi_progressive_*, include/gi_hip.h): the frame is refined in steps, and a frame built in steps
    has the bits of the frame `run` builds in one call.  From RayTracer.progressive(w, h, **kw) or RayTracer.resume(blob); a context manager.
    A context has one session: opening another, or uploading a scene or photons, ends this one (its next step raises GiError, code -4).
    An object whose session was replaced by a newer one of the same RayTracer is stale: it raises the same error and its close() does nothing,
    so closing an old object never ends the newer session."""

    def __init__(self, rt, width, rows):
        self.rt, self.width, self.rows = rt, width, rows
        rt._session_serial = self.serial = getattr(rt, "_session_serial", 0) + 1

    def _mine(self):
        """Raise unless the context's session is still the one this object opened."""
        if self.rt._session_serial != self.serial:
            raise GiError(f"progressive: this session was replaced by a newer one of the same RayTracer ({GI_E_STATE})")

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def _status(self):
        self._mine()
        e, n = C.c_int32(), C.c_int64()
        self.rt._check(self.rt.L.gi_progressive_status(self.rt.h, C.byref(e), C.byref(n)), "progressive_status")
        return e.value, n.value

    @property
    def sample_end(self):
        """E: every pixel has been offered samples [0, E)."""
        return self._status()[0]

    @property
    def pixels_wanting(self):
        """Pixels of this rank that would still take a sample under the session's max_samples."""
        return self._status()[1]

    @property
    def done(self):
        return self.pixels_wanting == 0

    def step(self, n, f64=True, want_spp=False, cancel=None):
        """Take up to n more samples per pixel and return the frame so far, [rows][w][3] linear (and the samples taken per pixel with want_spp).
        cancel: an optional ctypes c_int polled during the step; a cancelled step raises GiError (code -5) and the session goes on."""
        self._mine()
        out = np.zeros((self.rows, self.width, 3), np.float64 if f64 else np.float32)
        spp = np.zeros((self.rows, self.width), np.int32) if want_spp else None
        self.rt._check(self.rt.L.gi_progressive_step_host(self.rt.h, int(n), out.ctypes.data_as(C.c_void_p), 1 if f64 else 0,
                                                          spp.ctypes.data_as(C.c_void_p) if want_spp else None,
                                                          C.addressof(cancel) if cancel is not None else None), "progressive_step")
        return (out, spp) if want_spp else out

    def frame(self, f64=True, want_spp=False):
        """The frame as it stands (step(0): no path kernel runs)."""
        return self.step(0, f64=f64, want_spp=want_spp)

    def step_device(self, n, out_ptr, f64=False, spp_ptr=None):
        """A step into device memory (raw device pointers), asynchronous on the context's stream."""
        self._mine()
        self.rt._check(self.rt.L.gi_progressive_step_device(self.rt.h, int(n), C.c_void_p(out_ptr), 1 if f64 else 0, C.c_void_p(spp_ptr) if spp_ptr else None, None), "progressive_step")

    def save(self):
        """The session as a checkpoint blob (bytes) for RayTracer.resume on a context with the same scene and photons."""
        self._mine()
        n = C.c_int64()
        self.rt._check(self.rt.L.gi_progressive_state_bytes(self.rt.h, C.byref(n)), "progressive_state_bytes")
        buf = C.create_string_buffer(n.value)
        self.rt._check(self.rt.L.gi_progressive_save(self.rt.h, buf, n.value), "progressive_save")
        return buf.raw

    def close(self):
        """End the session and free its records; nothing when a newer session has replaced this one."""
        if self.rt._session_serial == self.serial:
            self.rt.L.gi_progressive_end(self.rt.h)


class RayTracerGroup:
    """Several devices driven from one process through the C ABI's gi_group_* entries (include/gi_hip.h): what the C++ RayTracer::run uses when
    more than one GPU is visible.  `devices` may repeat an ordinal (several contexts on one device)."""

    def __init__(self, devices):
        self.L = lib()
        h = C.c_void_p()
        dv = np.ascontiguousarray(devices, np.int32)
        rc = self.L.gi_group_create(C.byref(h), len(dv), _p(dv, _ip))
        if rc != GI_OK:
            raise GiError(f"gi_group_create failed ({rc}): no usable HIP device -- this path has no CPU fallback")
        self.h = h
        self.n = self.L.gi_group_size(h)

    def __del__(self):
        try:
            self.L.gi_group_destroy(self.h)
        except Exception:
            pass

    def _check(self, rc, what):
        if rc < 0:
            raise GiError(f"{what}: {self.L.gi_group_last_error(self.h).decode()} ({rc})")

    def setScene(self, scene, photons=None):
        d = scene.desc()
        self._check(self.L.gi_group_upload_scene(self.h, C.byref(d)), "group upload_scene")
        self.L.gi_group_clear_photons(self.h)
        if photons is not None:
            scene.build_photon_map(photons)
            pd = scene.photon_desc()
            self._check(self.L.gi_group_upload_photons(self.h, C.byref(pd)), "group upload_photons")
        return self

    def set_lens(self, radius=None, blades=None, rotation=None, lens=None):
        """gi_group_set_lens: the thin lens of every member context (RayTracer.set_lens)."""
        l = lens if lens is not None else lens_params(radius, blades, rotation)
        self._check(self.L.gi_group_set_lens(self.h, C.byref(l)), "group set_lens")
        return self

    def run(self, params, stripe_h=16, first_stripe=0, n_stripes=None, f64=True, frame=None):
        """gi_group_render_host: the stripes of the window into a whole-frame host buffer (rows outside the window keep what `frame` held)."""
        w, h = params.width, params.height
        total = (h + stripe_h - 1) // stripe_h
        n_stripes = total if n_stripes is None else n_stripes
        out = np.zeros((h, w, 3), np.float64 if f64 else np.float32) if frame is None else frame
        self._check(self.L.gi_group_render_host(self.h, C.byref(params), stripe_h, first_stripe, n_stripes, out.ctypes.data_as(C.c_void_p), 1 if f64 else 0, None, None), "group render_host")
        return out

    def run_device(self, params, out_ptr, stripe_h=16, f64=False):
        """gi_group_render_device: the whole frame gathered on the first context's device (raw device pointer)."""
        self._check(self.L.gi_group_render_device(self.h, C.byref(params), stripe_h, C.c_void_p(out_ptr), 1 if f64 else 0, None), "group render_device")


class RayTracer:
    """Device context = the reference's RayTracer for this path (include/raytracer.h:23-735)."""

    def __init__(self, device=0):
        self.L = lib()
        h = C.c_void_p()
        rc = self.L.gi_create(C.byref(h), int(device))
        if rc != GI_OK:
            raise GiError(f"gi_create failed ({rc}): no usable HIP device -- this path has no CPU fallback")
        self.h = h
        self.scene = None
        st = Scene().settings  # reference defaults (include/util.h:24-29, main.cpp:28)
        self.photons, self.photon_depth = st.photons, st.photon_depth
        self.min_samples, self.max_samples, self.noise_thresh = st.min_samples, st.max_samples, st.noise_thresh
        self.cam_pos, self.cam_up, self.cam_forward = list(st.cam_pos), list(st.cam_up), list(st.cam_forward)
        self.sensor_diag, self.focal_dist = st.sensor_diag, st.focal_dist
        self.seed = DEFAULT_SEED

    def __del__(self):
        try:
            self.L.gi_destroy(self.h)
        except Exception:
            pass

    def _check(self, rc, what):
        if rc < 0:
            raise GiError(f"{what}: {self.L.gi_last_error(self.h).decode()} ({rc})")
        return rc

    def set_stream(self, stream_ptr):
        self._check(self.L.gi_set_stream(self.h, C.c_void_p(stream_ptr)), "set_stream")

    def setScene(self, scene, adopt_settings=True):
        """RayTracer::setScene (include/raytracer.h:35-39) + upload of the flattened tables."""
        d = scene.desc()
        self._check(self.L.gi_upload_scene(self.h, C.byref(d)), "upload_scene")
        self._check(self.L.gi_clear_photons(self.h), "clear_photons")      # a fresh PhotonMap, as RayTracer::setScene allocates
        self.scene = scene
        if adopt_settings:
            st = scene.settings
            self.photons, self.photon_depth = st.photons, st.photon_depth
            self.min_samples, self.max_samples, self.noise_thresh = st.min_samples, st.max_samples, st.noise_thresh
            self.cam_pos, self.cam_up, self.cam_forward = list(st.cam_pos), list(st.cam_up), list(st.cam_forward)
            self.sensor_diag, self.focal_dist = st.sensor_diag, st.focal_dist
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
        n = self._check(self.L.gi_emit_photons(self.h, count, max_depth, C.c_uint64(self.seed if seed is None else seed), _p(out), cap, C.byref(tries)), "emit_photons")
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
        n = self._check(self.L.gi_trace_photons(self.h, count, max_depth, C.c_uint64(self.seed if seed is None else seed), None, C.byref(tries)), "trace_photons")
        return n, tries.value

    def photon_tables_on_device(self):
        """The photon-map tables as the gather kernel sees them (gi_debug_photon_tables)."""
        nn, nr, nph = C.c_int32(), C.c_int32(), C.c_int32()
        self._check(self.L.gi_debug_photon_tables(self.h, C.byref(nn), C.byref(nr), C.byref(nph), None, None, None, None), "photon_tables")
        nodes = np.zeros((nn.value, 128), np.uint8); ranges = np.zeros((nr.value, 2), np.int32)
        pos = np.zeros((nph.value, 3)); dircol = np.zeros((nph.value, 6))
        if nn.value:
            self._check(self.L.gi_debug_photon_tables(self.h, None, None, None, nodes.ctypes.data_as(C.c_void_p), _p(ranges, _ip), _p(pos), _p(dircol)), "photon_tables")
        return {"nodes": nodes, "ranges": ranges, "pos": pos, "dircol": dircol}

    def params(self, w, h, stripe_h=None, rank=0, world=1, min_samples=None, max_samples=None, noise_thresh=None, seed=None):
        p = RenderParams()
        p.cam_pos[:] = self.cam_pos; p.cam_up[:] = self.cam_up; p.cam_forward[:] = self.cam_forward
        p.sensor_diag, p.focal_dist = self.sensor_diag, self.focal_dist
        p.width, p.height = w, h
        p.stripe_h, p.stripe_rank, p.stripe_world = (h if stripe_h is None else stripe_h), rank, world
        p.min_samples = self.min_samples if min_samples is None else min_samples
        p.max_samples = self.max_samples if max_samples is None else max_samples
        p.noise_thresh = self.noise_thresh if noise_thresh is None else noise_thresh
        p.seed = self.seed if seed is None else seed
        return p

    def local_rows(self, p):
        return self.L.gi_local_rows(C.byref(p))

    def run(self, w, h, f64=True, want_spp=False, **kw):
        """RayTracer::run(w, h) pixel loop -> linear radiance [rows][w][3] on the host."""
        p = self.params(w, h, **kw)
        rows = self.local_rows(p)
        out = np.zeros((rows, w, 3), np.float64 if f64 else np.float32)
        spp = np.zeros((rows, w), np.int32) if want_spp else None
        self._check(self.L.gi_render_host(self.h, C.byref(p), out.ctypes.data_as(C.c_void_p), 1 if f64 else 0,
                                          spp.ctypes.data_as(C.c_void_p) if want_spp else None, None), "render_host")
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
        self._check(self.L.gi_render_device(self.h, C.byref(p), C.c_void_p(out_ptr), 1 if f64 else 0, C.c_void_p(spp_ptr) if spp_ptr else None, None), "render_device")

    def run_features(self, w, h, n, f64=True, want_ids=True, **kw):
        """First-hit feature buffers of the frame `run` renders (gi_render_features_host; an addition, the reference has no such pass): per pixel the
        mean over samples 0 .. n-1 of the first hit's diffuse colour, normal, distance and coverage, and the entity / material of sample 0's hit.
        Returns a dict of views into one array `features` [rows][w][8]: albedo [rows][w][3], normal [rows][w][3], depth [rows][w], coverage [rows][w],
        and ids [rows][w][2] int32 (None without want_ids).  **kw as for run (stripes, seed); min_samples / max_samples play no part."""
        p = self.params(w, h, **kw)
        rows = self.local_rows(p)
        out = np.zeros((rows, w, 8), np.float64 if f64 else np.float32)
        ids = np.zeros((rows, w, 2), np.int32) if want_ids else None
        self._check(self.L.gi_render_features_host(self.h, C.byref(p), int(n), out.ctypes.data_as(C.c_void_p), 1 if f64 else 0,
                                                   ids.ctypes.data_as(C.c_void_p) if want_ids else None), "render_features_host")
        return {"features": out, "albedo": out[:, :, 0:3], "normal": out[:, :, 3:6], "depth": out[:, :, 6], "coverage": out[:, :, 7], "ids": ids}

    def run_features_device(self, p, n, out_ptr, f64=False, ids_ptr=None):
        """The feature pass into device memory; out_ptr ([rows][w][8]) and ids_ptr ([rows][w][2] int32, optional) are raw device pointers."""
        self._check(self.L.gi_render_features_device(self.h, C.byref(p), int(n), C.c_void_p(out_ptr), 1 if f64 else 0, C.c_void_p(ids_ptr) if ids_ptr else None), "render_features_device")

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
        out = np.zeros((h, w, 3), np.float64 if f64 else np.float32)
        self._check(self.L.gi_denoise_host(self.h, C.byref(p), color.ctypes.data_as(C.c_void_p), 1 if color.dtype == np.float64 else 0,
                                           features.ctypes.data_as(C.c_void_p), 1 if features.dtype == np.float64 else 0,
                                           out.ctypes.data_as(C.c_void_p), 1 if f64 else 0), "denoise_host")
        return out

    def denoise_device(self, p, color_ptr, features_ptr, out_ptr, color_f64=False, features_f64=False, out_f64=False):
        """The denoiser on device memory, asynchronous on the context's stream; p from denoise_params; raw device pointers to [h][w][3],
        [h][w][8] and [h][w][3]; out_ptr may equal color_ptr."""
        self._check(self.L.gi_denoise_device(self.h, C.byref(p), C.c_void_p(color_ptr), 1 if color_f64 else 0, C.c_void_p(features_ptr), 1 if features_f64 else 0,
                                             C.c_void_p(out_ptr), 1 if out_f64 else 0), "denoise_device")

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
        out = np.zeros((h, w, 3), np.float64 if f64 else np.float32)
        self._check(self.L.gi_upsample_host(self.h, C.byref(p), low_color.ctypes.data_as(C.c_void_p), 1 if low_color.dtype == np.float64 else 0,
                                            low_features.ctypes.data_as(C.c_void_p), 1 if low_features.dtype == np.float64 else 0,
                                            features.ctypes.data_as(C.c_void_p), 1 if features.dtype == np.float64 else 0,
                                            out.ctypes.data_as(C.c_void_p), 1 if f64 else 0), "upsample_host")
        return out

    def upsample_device(self, p, low_color_ptr, low_features_ptr, features_ptr, out_ptr, low_color_f64=False, low_features_f64=False, features_f64=False, out_f64=False):
        """The upsampler on device memory, asynchronous on the context's stream; p from upsample_params; raw device pointers to [hl][wl][3],
        [hl][wl][8], [h][w][8] and [h][w][3]; out must not overlap an input."""
        self._check(self.L.gi_upsample_device(self.h, C.byref(p), C.c_void_p(low_color_ptr), 1 if low_color_f64 else 0, C.c_void_p(low_features_ptr), 1 if low_features_f64 else 0,
                                              C.c_void_p(features_ptr), 1 if features_f64 else 0, C.c_void_p(out_ptr), 1 if out_f64 else 0), "upsample_device")

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
        out = np.zeros((rows, w, 4), np.float64 if f64 else np.float32)
        self._check(self.L.gi_render_occlusion_host(self.h, C.byref(p), C.byref(op), out.ctypes.data_as(C.c_void_p), 1 if f64 else 0), "render_occlusion_host")
        return {"occlusion": out, "open": out[:, :, 0], "bent": out[:, :, 1:4]}

    def run_occlusion_device(self, p, op, out_ptr, f64=False):
        """The occlusion pass into device memory, asynchronous on the context's stream; p from params, op from occlusion_params; out_ptr
        ([rows][w][4]) is a raw device pointer."""
        self._check(self.L.gi_render_occlusion_device(self.h, C.byref(p), C.byref(op), C.c_void_p(out_ptr), 1 if f64 else 0), "render_occlusion_device")

    def last_occlusion_ms(self):
        """gi_last_occlusion_ms: device time of the last occlusion pass (the frame's and the other passes' times keep theirs)."""
        return self._last_ms("occlusion")

    def bake_params(self, mode, samples, stream_base=0, seed=None):
        """gi_bake_params: mode BAKE_TEXEL / BAKE_SH9 (or "texel" / "sh9"), samples per point, the stream index of sample 0 of point 0, the seed
        (default: the tracer's)."""
        p = BakeParams()
        self.L.gi_bake_default_params(C.byref(p))
        p.mode = {"texel": BAKE_TEXEL, "sh9": BAKE_SH9}.get(mode, mode)
        p.n_samples, p.stream_base = int(samples), int(stream_base)
        p.seed = self.seed if seed is None else seed
        return p

    @staticmethod
    def _bake_points(points, normals=None):
        pts = _f64(points).reshape(-1, 3)
        if normals is None:
            return pts
        nrm = _f64(normals).reshape(-1, 3)
        if len(nrm) != len(pts):
            raise ValueError(f"bake: {len(pts)} points and {len(nrm)} normals")
        return np.ascontiguousarray(np.concatenate([pts, nrm], 1))

    def _bake(self, rows, bp, f64):
        n = len(rows)
        out = np.zeros((n, 3) if bp.mode == BAKE_TEXEL else (n, 9, 3), np.float64 if f64 else np.float32)
        self._check(self.L.gi_bake_host(self.h, _p(rows), n, C.byref(bp), out.ctypes.data_as(C.c_void_p), 1 if f64 else 0), "bake_host")
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
        self._check(self.L.gi_bake_device(self.h, C.c_void_p(points_ptr), int(n_points), C.byref(bp), C.c_void_p(out_ptr), 1 if f64 else 0), "bake_device")

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
        mode = {"texel": BAKE_TEXEL, "sh9": BAKE_SH9}.get(mode, mode)
        L3 = _f64(radiance)
        n, ns = L3.shape[:2]
        d3 = _f64(dirs) if dirs is not None else None
        if L3.ndim != 3 or L3.shape[2] != 3 or (d3 is not None and d3.shape != L3.shape):
            raise ValueError("bake_fold: radiance and directions [n][samples][3] expected")
        out = np.zeros((n, 3) if mode == BAKE_TEXEL else (n, 9, 3))
        self._check(self.L.gi_bake_fold(self.h, mode, n, ns, _p(d3), _p(L3), _p(out)), "bake_fold")
        return out

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
        p.seed = self.seed if seed is None else seed
        return p

    @staticmethod
    def _chart(ent, uv):
        e = np.ascontiguousarray(ent, np.int32).reshape(-1)
        c = _f64(uv).reshape(-1, 3, 2)
        if len(c) != len(e):
            raise ValueError(f"lightmap: {len(e)} entities and {len(c)} chart triangles")
        return e, c

    def bake_lightmap(self, ent, uv, width, height, samples, dilate=2, flip=False, stream_base=0, seed=None, f64=True, want_owner=False):
        """A lightmap atlas (gi_lightmap_host; an addition around the bake): the chart -- ent [n] triangle entities, uv [n][3][2] their chart
        coordinates in [0, 1]^2, v growing with the row -- rasterised into width x height texels, every covered texel baked as bake_texels does with
        `samples` rays, the rows put back into the image and the gutters filled by `dilate` passes.  Returns the atlas [height][width][3], or
        (atlas, owner [height][width] = the chart row of a covered texel or -1, n_covered) with want_owner.  Sample k of the i-th covered texel
        (ascending y * width + x) runs on stream stream_base + i * samples + k; the definition is stated in include/gi_hip.h.  chart_of_material
        gives the chart of a scene whose texture coordinates are an atlas already."""
        e, c = self._chart(ent, uv)
        p = self.lightmap_params(width, height, samples, dilate, flip, stream_base, seed)
        atlas = np.zeros((max(p.height, 0), max(p.width, 0), 3), np.float64 if f64 else np.float32)
        owner = np.full((max(p.height, 0), max(p.width, 0)), -1, np.int32) if want_owner else None
        n_cov = C.c_int32(0)
        self._check(self.L.gi_lightmap_host(self.h, C.byref(p), len(e), _p(e, _ip), _p(c), atlas.ctypes.data_as(C.c_void_p), 1 if f64 else 0,
                                            _p(owner, _ip), C.byref(n_cov)), "lightmap_host")
        return (atlas, owner, n_cov.value) if want_owner else atlas

    def lightmap_device(self, p, n_chart, ent_ptr, uv_ptr, atlas_ptr, f64=False, owner_ptr=None):
        """A lightmap on device memory (raw device pointers: ent [n] int32, uv [n][3][2] f64, atlas [h][w][3], owner [h][w] int32 or None); p from
        lightmap_params.  The chart is not looked at.  Returns n_covered."""
        n_cov = C.c_int32(0)
        self._check(self.L.gi_lightmap_device(self.h, C.byref(p), int(n_chart), C.c_void_p(ent_ptr), C.c_void_p(uv_ptr), C.c_void_p(atlas_ptr),
                                              1 if f64 else 0, C.c_void_p(owner_ptr), C.byref(n_cov)), "lightmap_device")
        return n_cov.value

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

    def last_lightmap_ms(self):
        """gi_last_lightmap_ms: (device time of the last lightmap, {"raster": .., "bake": .., "dilate": ..} -- raster + rank, bake, scatter + dilate);
        gi_last_bake_ms, the frame's and the other passes' times keep theirs."""
        ms, st = C.c_float(0), (C.c_float * 3)()
        self._check(self.L.gi_last_lightmap_ms(self.h, C.byref(ms), st), "last_lightmap_ms")
        return ms.value, dict(zip(("raster", "bake", "dilate"), (float(x) for x in st)))

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

    def primary_rays(self, p, idx):
        """gi_debug_primary_rays: rays [n][6] = origin, unit direction of the samples with Halton indices idx of the frame p (from params), under
        the context's lens."""
        idx = np.ascontiguousarray(idx, np.uint32).reshape(-1)
        rays = np.zeros((len(idx), 6))
        self._check(self.L.gi_debug_primary_rays(self.h, C.byref(p), len(idx), _p(idx, _up), _p(rays)), "primary_rays")
        return rays

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
        self._check(self.L.gi_radiance(self.h, len(rays), _p(rays), _p(stream, _up), C.c_uint64(self.seed if seed is None else seed), _p(out)), "radiance")
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
        self._check(self.L.gi_halton_sample(self.h, len(dim), _p(dim, _up), _p(index, _up), out.ctypes.data_as(C.POINTER(C.c_float))), "halton_sample")
        return out

    def halton_index(self, w, h, sxy):
        sxy = np.ascontiguousarray(sxy, np.uint32).reshape(-1, 3)
        out = np.zeros(len(sxy), np.uint32)
        self._check(self.L.gi_halton_index(self.h, w, h, len(sxy), _p(sxy, _up), _p(out, _up)), "halton_index")
        return out
