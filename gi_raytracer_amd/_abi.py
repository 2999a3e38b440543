"""The C ABI of libgi_raytracer_hip.so as ctypes sees it: constants, the mirrors of the header structs, one signature table for every symbol
include/gi_hip.h and csrc/gi_host.h declare, the loader, and the numpy / ctypes helpers of the binding.  tests/test_abi.py checks the table
against the headers' declarations, tests/test_abi_layout.py the structs against the headers' layouts."""
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
BAKE_TEXEL, BAKE_SH9 = 0, 1
BAKE_MODES = {"texel": BAKE_TEXEL, "sh9": BAKE_SH9}
CUBEMAP_MAX_LEVELS = 12
PROBE_VISIBILITY_MAX_SIZE = 64
REFLECTIONS_MAX_PROBES = 64
BAKED_DIRECT, BAKED_DIFFUSE, BAKED_SPECULAR, BAKED_EMISSIVE = 1, 2, 4, 8
LM_NEAREST, LM_BILINEAR = 0, 1
LM_FILTERS = {"nearest": LM_NEAREST, "bilinear": LM_BILINEAR}

_dp, _ip, _up, _fp, _lp, _bp = (C.POINTER(t) for t in (C.c_double, C.c_int32, C.c_uint32, C.c_float, C.c_int64, C.c_uint8))


class GiError(RuntimeError):
    pass


class SceneDesc(C.Structure):
    _fields_ = [("n_tri", C.c_int32), ("tri_pos", _dp), ("tri_nrm", _dp), ("tri_uv", _dp), ("tri_mat", _ip), ("n_mat", C.c_int32), ("mats", _dp),
                ("n_light", C.c_int32), ("lights", _dp), ("ambient", C.c_double * 3), ("n_node", C.c_int32), ("node_bbox", _dp), ("node_child", _ip),
                ("node_ent_off", _ip), ("node_ent_idx", _ip), ("ent_kind", _ip), ("n_fog", C.c_int32), ("fog", _dp), ("fog_grid_off", _ip),
                ("fog_grid", _dp), ("n_tex", C.c_int32), ("tex_kind", _ip), ("tex_param", _dp), ("mat_tex", _ip), ("tex_pixels", _bp),
                ("n_tex_pixel_bytes", C.c_int64)]


class PhotonMapDesc(C.Structure):
    _fields_ = [("n_photon", C.c_int32), ("photons", _dp), ("n_node", C.c_int32), ("node_bbox", _dp), ("node_child", _ip), ("node_off", _ip),
                ("node_idx", _ip)]


class RenderParams(C.Structure):
    _fields_ = [("cam_pos", C.c_double * 3), ("cam_up", C.c_double * 3), ("cam_forward", C.c_double * 3), ("sensor_diag", C.c_double),
                ("focal_dist", C.c_double), ("width", C.c_int32), ("height", C.c_int32), ("stripe_h", C.c_int32), ("stripe_rank", C.c_int32),
                ("stripe_world", C.c_int32), ("min_samples", C.c_int32), ("max_samples", C.c_int32), ("noise_thresh", C.c_double),
                ("seed", C.c_uint64)]


class DenoiseParams(C.Structure):
    """gi_denoise_params (include/gi_hip.h)."""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("iterations", C.c_int32), ("demodulate", C.c_int32), ("sigma_color", C.c_double),
                ("sigma_normal", C.c_double), ("sigma_depth", C.c_double), ("sigma_albedo", C.c_double)]


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


class LightmapParams(C.Structure):
    """gi_lightmap_params (include/gi_hip.h)."""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("n_samples", C.c_int32), ("dilate", C.c_int32), ("flip", C.c_int32),
                ("stream_base", C.c_uint32), ("seed", C.c_uint64)]


class CubemapParams(C.Structure):
    """gi_cubemap_params (include/gi_hip.h)."""
    _fields_ = [("face", C.c_int32), ("n_samples", C.c_int32), ("levels", C.c_int32), ("stream_base", C.c_uint32), ("seed", C.c_uint64),
                ("log2_exponent", C.c_int32 * CUBEMAP_MAX_LEVELS)]


class BakedParams(C.Structure):
    """gi_baked_params (include/gi_hip.h)."""
    _fields_ = [("n_samples", C.c_int32), ("terms", C.c_int32), ("grid_min", C.c_double * 3), ("grid_max", C.c_double * 3), ("nx", C.c_int32),
                ("ny", C.c_int32), ("nz", C.c_int32), ("face", C.c_int32), ("levels", C.c_int32), ("log2_exponent", C.c_int32 * CUBEMAP_MAX_LEVELS)]


class BakedLightmapParams(C.Structure):
    """gi_baked_lightmap_params (include/gi_hip.h)."""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("filter", C.c_int32), ("n_chart", C.c_int32)]


class ProbeVisibilityParams(C.Structure):
    """gi_probe_visibility_params (include/gi_hip.h)."""
    _fields_ = [("size", C.c_int32), ("n_samples", C.c_int32), ("stream_base", C.c_uint32), ("seed", C.c_uint64), ("max_dist", C.c_double)]


class BakedVisibilityParams(C.Structure):
    """gi_baked_visibility_params (include/gi_hip.h)."""
    _fields_ = [("size", C.c_int32), ("normal_bias", C.c_double), ("vis_floor", C.c_double)]


class BakedReflectionsParams(C.Structure):
    """gi_baked_reflections_params (include/gi_hip.h)."""
    _fields_ = [("n_probes", C.c_int32)]


class FinalGatherParams(C.Structure):
    """gi_final_gather_params (include/gi_hip.h)."""
    _fields_ = [("baked", BakedParams), ("n_dirs", C.c_int32), ("reserved", C.c_int32)]


class Settings(C.Structure):
    _fields_ = [("photons", C.c_int32), ("photon_depth", C.c_int32), ("min_samples", C.c_int32), ("max_samples", C.c_int32),
                ("noise_thresh", C.c_double), ("ambient", C.c_double * 3), ("cam_pos", C.c_double * 3), ("cam_up", C.c_double * 3),
                ("cam_forward", C.c_double * 3), ("sensor_diag", C.c_double), ("focal_dist", C.c_double)]


# header type -> its mirror (tests/test_abi_layout.py compiles sizeof / offsetof of every field against the headers)
STRUCTS = {"gi_scene_desc": SceneDesc, "gi_photon_map_desc": PhotonMapDesc, "gi_render_params": RenderParams, "gi_denoise_params": DenoiseParams,
           "gi_upsample_params": UpsampleParams, "gi_occlusion_params": OcclusionParams, "gi_lens": Lens, "gi_bake_params": BakeParams,
           "gi_lightmap_params": LightmapParams, "gi_cubemap_params": CubemapParams, "gi_baked_params": BakedParams,
           "gi_baked_lightmap_params": BakedLightmapParams, "gi_probe_visibility_params": ProbeVisibilityParams,
           "gi_baked_visibility_params": BakedVisibilityParams, "gi_baked_reflections_params": BakedReflectionsParams,
           "gi_final_gather_params": FinalGatherParams, "gih_settings": Settings}


def _signatures():
    """name -> (restype, argtypes) of every symbol the two headers declare, in the headers' order.  `int` and `int32_t` are one ctypes type."""
    i, i32, i64, u64, d, vp, s = C.c_int, C.c_int32, C.c_int64, C.c_uint64, C.c_double, C.c_void_p, C.c_char_p
    P, ms, knob = C.POINTER, (i, [vp, _fp]), (i, [vp, i])
    scene, photons, rp = P(SceneDesc), P(PhotonMapDesc), P(RenderParams)
    dn, us, oc, lens, bake, lm = P(DenoiseParams), P(UpsampleParams), P(OcclusionParams), P(Lens), P(BakeParams), P(LightmapParams)
    cm, bk, bl = P(CubemapParams), P(BakedParams), P(BakedLightmapParams)
    pv, bv, br = P(ProbeVisibilityParams), P(BakedVisibilityParams), P(BakedReflectionsParams)
    fg = P(FinalGatherParams)
    return {
        # include/gi_hip.h: context, uploads, frames
        "gi_create": (i, [P(vp), i]), "gi_destroy": (None, [vp]), "gi_last_error": (s, [vp]), "gi_set_stream": (i, [vp, vp]),
        "gi_upload_scene": (i, [vp, scene]), "gi_upload_photons": (i, [vp, photons]), "gi_clear_photons": (i, [vp]), "gi_local_rows": (i, [rp]),
        "gi_render_device": (i, [vp, rp, vp, i, vp, vp]), "gi_render_host": (i, [vp, rp, vp, i, vp, vp]), "gi_set_render_mode": knob,
        "gi_set_wide_nodes": knob, "gi_set_content_culling": knob, "gi_set_entity_boxes": knob, "gi_set_pool_slots": (i, [vp, i64]),
        "gi_last_render_ms": (i, [vp, _fp, _ip]), "gi_last_stage_ms": ms, "gi_last_kernel_ms": ms, "gi_set_counters": knob,
        "gi_get_counters": (i, [vp, _lp]), "gi_get_stream_counters": (i, [vp, _lp]),
        # feature buffers, denoiser, upsampler, occlusion
        "gi_render_features_device": (i, [vp, rp, i32, vp, i, vp]), "gi_render_features_host": (i, [vp, rp, i32, vp, i, vp]),
        "gi_last_features_ms": ms, "gi_denoise_default_params": (None, [dn]), "gi_denoise_device": (i, [vp, dn, vp, i, vp, i, vp, i]),
        "gi_denoise_host": (i, [vp, dn, vp, i, vp, i, vp, i]), "gi_last_denoise_ms": ms, "gi_upsample_default_params": (None, [us]),
        "gi_upsample_device": (i, [vp, us, vp, i, vp, i, vp, i, vp, i]), "gi_upsample_host": (i, [vp, us, vp, i, vp, i, vp, i, vp, i]),
        "gi_last_upsample_ms": ms, "gi_occlusion_default_params": (None, [oc]), "gi_render_occlusion_device": (i, [vp, rp, oc, vp, i]),
        "gi_render_occlusion_host": (i, [vp, rp, oc, vp, i]), "gi_last_occlusion_ms": ms,
        # check entries
        "gi_trace": (i, [vp, i32, _dp, _ip, _ip, _dp]), "gi_visible": (i, [vp, i32, _dp, _ip]), "gi_visible_rays": (i, [vp, i32, _dp, _dp, _ip]),
        "gi_gather": (i, [vp, i32, _dp, _dp, _ip]), "gi_radiance": (i, [vp, i32, _dp, _up, u64, _dp]),
        "gi_emit_photons": (i, [vp, i32, i32, u64, _dp, i32, _lp]), "gi_halton_sample": (i, [vp, i32, _up, _up, _fp]),
        "gi_halton_index": (i, [vp, i32, i32, i32, _up, _up]), "gi_build_photon_map": (i, [vp, i32, _dp, _dp]),
        "gi_trace_photons": (i, [vp, i32, i32, u64, _dp, _lp]), "gi_debug_photon_tables": (i, [vp, _ip, _ip, _ip, vp, _ip, _dp, _dp]),
        # device groups
        "gi_device_count": (i, []), "gi_group_create": (i, [P(vp), i32, _ip]), "gi_group_destroy": (None, [vp]), "gi_group_size": (i, [vp]),
        "gi_group_ctx": (vp, [vp, i32]), "gi_group_last_error": (s, [vp]), "gi_group_upload_scene": (i, [vp, scene]),
        "gi_group_upload_photons": (i, [vp, photons]), "gi_group_clear_photons": (i, [vp]),
        "gi_group_render_host": (i, [vp, rp, i32, i32, i32, vp, i, vp, vp]), "gi_group_render_device": (i, [vp, rp, i32, vp, i, vp]),
        # debug entries
        "gi_debug_leaf_order": (i, [vp, i32, _dp, i32, _ip, _ip]), "gi_debug_sort_pairs": (i, [vp, i32, _up, _up, i32, i32, _up, _up]),
        "gi_debug_find_leaves": (i, [vp, i32, _dp, _ip, _ip]), "gi_debug_gather_pass": (i, [vp, i32, _dp, i32, i32, _dp, _up, _up, _lp]),
        "gi_debug_walk": (i, [vp, i32, _dp, _dp, i32, i32, _ip, _ip, _dp]), "gi_kat": (i, [vp, i32, i32, _dp, i32, _dp]),
        # progressive sessions
        "gi_progressive_begin": (i, [vp, rp]), "gi_progressive_step_device": (i, [vp, i32, vp, i, vp, vp]),
        "gi_progressive_step_host": (i, [vp, i32, vp, i, vp, vp]), "gi_progressive_status": (i, [vp, _ip, _lp]),
        "gi_progressive_state_bytes": (i, [vp, _lp]), "gi_progressive_save": (i, [vp, vp, i64]), "gi_progressive_restore": (i, [vp, vp, i64]),
        "gi_progressive_end": (i, [vp]),
        # lens
        "gi_lens_default": (None, [lens]), "gi_set_lens": (i, [vp, lens]), "gi_get_lens": (i, [vp, lens]), "gi_lens_vertices": (i, [lens, _dp]),
        "gi_group_set_lens": (i, [vp, lens]), "gi_debug_primary_rays": (i, [vp, rp, i32, _up, _dp]),
        "gi_focus_distance": (i, [vp, rp, i32, i32, _dp]),
        # bakes and lightmaps
        "gi_bake_default_params": (None, [bake]), "gi_bake_device": (i, [vp, vp, i32, bake, vp, i]), "gi_bake_host": (i, [vp, _dp, i32, bake, vp, i]),
        "gi_last_bake_ms": ms, "gi_bake_rays": (i, [vp, _dp, i32, bake, _dp, _up]), "gi_bake_fold": (i, [vp, i32, i32, i32, _dp, _dp, _dp]),
        "gi_lightmap_default_params": (None, [lm]), "gi_lightmap_host": (i, [vp, lm, i32, _ip, _dp, vp, i, _ip, _ip]),
        "gi_lightmap_device": (i, [vp, lm, i32, vp, vp, vp, i, vp, _ip]), "gi_last_lightmap_ms": (i, [vp, _fp, _fp]),
        "gi_lightmap_texels": (i, [vp, lm, i32, _ip, _dp, _ip, _ip, _dp, _ip, i32]), "gi_lightmap_dilate": (i, [vp, i32, i32, i32, _dp, _ip, _dp]),
        # reflection probes
        "gi_cubemap_default_params": (None, [cm]), "gi_cubemap_chain_texels": (i64, [i32, i32]), "gi_cubemap_host": (i, [vp, _dp, cm, vp, i]),
        "gi_cubemap_device": (i, [vp, _dp, cm, vp, i]), "gi_last_cubemap_ms": (i, [vp, _fp, _fp]), "gi_cubemap_rays": (i, [vp, _dp, cm, _dp, _up]),
        "gi_cubemap_prefilter": (i, [vp, cm, _dp, _dp]),
        # the baked-light pass
        "gi_baked_default_params": (None, [bk]), "gi_render_baked_device": (i, [vp, rp, bk, vp, vp, vp, i]),
        "gi_render_baked_host": (i, [vp, rp, bk, _dp, _dp, vp, i]), "gi_last_baked_ms": ms,
        "gi_baked_lightmap_default_params": (None, [bl]), "gi_render_baked_lightmap_host": (i, [vp, rp, bk, bl, _dp, _dp, vp, i, _ip, _dp, vp, i]),
        "gi_render_baked_lightmap_device": (i, [vp, rp, bk, bl, vp, vp, vp, vp, vp, vp, i]),
        # probe visibility: the capture, and the baked-light pass that reads the maps
        "gi_probe_visibility_default_params": (None, [pv]), "gi_probe_visibility_device": (i, [vp, vp, i32, pv, vp, i]),
        "gi_probe_visibility_host": (i, [vp, _dp, i32, pv, vp, i]), "gi_last_probe_visibility_ms": ms,
        "gi_probe_visibility_rays": (i, [vp, _dp, i32, pv, _dp, _up]), "gi_probe_visibility_fold": (i, [vp, i32, i32, _dp, _dp]),
        "gi_baked_visibility_default_params": (None, [bv]), "gi_render_baked_visibility_device": (i, [vp, rp, bk, bv, vp, vp, vp, vp, i]),
        "gi_render_baked_visibility_host": (i, [vp, rp, bk, bv, _dp, _dp, vp, i, vp, i]),
        # reflection probe sets: the baked-light pass with box-projected, blended cube look-ups
        "gi_baked_reflections_default_params": (None, [br]), "gi_render_baked_reflections_device": (i, [vp, rp, bk, br, vp, vp, vp, vp, vp, i]),
        "gi_render_baked_reflections_host": (i, [vp, rp, bk, br, _dp, _dp, _dp, _dp, vp, i]),
        # the final-gather pass: one bounce from the first hits into the baked light
        "gi_final_gather_default_params": (None, [fg]), "gi_render_final_gather_device": (i, [vp, rp, fg, vp, vp, vp, i, vp]),
        "gi_render_final_gather_host": (i, [vp, rp, fg, _dp, _dp, vp, i, _ip]), "gi_last_final_gather_ms": ms,
        # csrc/gi_host.h: the host scene builder
        "gih_scene_create": (vp, []), "gih_scene_destroy": (None, [vp]), "gih_last_error": (s, [vp]), "gih_load_scn": (i, [vp, s]),
        "gih_load_obj": (i, [vp, s, _dp, _dp, i32]), "gih_add_material": (i, [vp, _dp]), "gih_add_texture": (i, [vp, i32, _dp, _bp, i64]),
        "gih_add_material_tex": (i, [vp, i32, i32, d, d, d]), "gih_load_png": (i, [s, _ip, _ip, _ip, P(_bp), s, i32]), "gih_free": (None, [vp]),
        "gih_add_triangles": (i, [vp, i32, _dp, _dp, _dp, _ip]), "gih_add_sphere": (i, [vp, _dp, d, i32]),
        "gih_add_height_fog": (i, [vp, _dp, _dp, i32, u64]), "gih_add_height_fog_grid": (i, [vp, _dp, _dp, i32]),
        "gih_add_light": (i, [vp, _dp, _dp, d]), "gih_set_ambient": (i, [vp, _dp]), "gih_get_settings": (i, [vp, P(Settings)]),
        "gih_set_camera": (i, [vp, _dp, _dp]), "gih_build_octree": (i, [vp]), "gih_get_scene_desc": (i, [vp, scene]),
        "gih_counts": (i, [vp, _ip, _ip, _ip, _ip, _ip]), "gih_build_photon_map": (i, [vp, i32, _dp]),
        "gih_build_photon_map_in_box": (i, [vp, _dp, i32, _dp]), "gih_get_photon_desc": (i, [vp, photons]), "gih_entity_bbox": (i, [i32, _dp, _dp]),
        "gih_entity_overlaps_box": (i, [i32, _dp, _dp]), "gih_box_mesh": (i, [_dp, _dp, _dp, _dp]), "gih_fog_grid": (i, [_dp, u64, _dp, i32]),
        "gih_to_rgb8": (i, [vp, i32, i64, _bp]),
    }


SIGNATURES = _signatures()
ABI_SYMBOLS = list(SIGNATURES)      # tests check that the headers declare exactly these and the library exports all of them
_LIB = None


def lib():
    """Load libgi_raytracer_hip.so (built by __graft_entry__.build() / csrc/Makefile).  Raises if it is missing."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise GiError(f"{LIB_PATH} not built: run `python -c 'import __graft_entry__ as g; g.build()'` (hipcc, gfx950)")
    L = C.CDLL(LIB_PATH)
    for name, (restype, argtypes) in SIGNATURES.items():
        f = getattr(L, name)
        f.restype, f.argtypes = restype, argtypes
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


def _floats(a):
    """a as a contiguous array of the library's two float types: float32 stays, anything else becomes float64."""
    a = np.asarray(a)
    return np.ascontiguousarray(a, np.float32 if a.dtype == np.float32 else np.float64)


def _buf(a):
    """(void*, is_f64): the pair the library takes for a host buffer that may hold float32 or float64."""
    return a.ctypes.data_as(C.c_void_p), 1 if a.dtype == np.float64 else 0


def _out(shape, f64):
    """A zeroed output array of that shape, float64 or float32, and its (void*, is_f64) pair."""
    a = np.zeros(shape, np.float64 if f64 else np.float32)
    return a, _buf(a)


def _dev(ptr, f64):
    """(void*, is_f64) of a raw device pointer."""
    return C.c_void_p(ptr), 1 if f64 else 0
