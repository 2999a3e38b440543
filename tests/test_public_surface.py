"""The public surface of the package as it stood before the split into modules: every module-level name of gi_raytracer_amd and every attribute of its
four classes is still there (new names are allowed).  Captured with dir() at the commit before the split.  Of the double-underscore names only
those the classes define themselves are kept (__del__, __enter__, __exit__); the rest (__doc__, __eq__ ...) come with any module or class."""
import pytest

import gi_raytracer_amd as gi

MODULE = """
    ABI_SYMBOLS BAKE_SH9 BAKE_TEXEL BakeParams C CHECKPOINT_HEADER CHECKPOINT_MAGIC CHECKPOINT_RECORD_BYTES CHECKPOINT_VERSION DEFAULT_SEED
    DenoiseParams GI_E_CANCELLED GI_E_HIP GI_E_INVALID GI_E_NO_DEVICE GI_E_STATE GI_OK GiError LENS_BLADES LIB_PATH Lens LightmapParams
    OCCLUSION_MAX_DIRS OcclusionParams PhotonMapDesc ProgressiveRender RayTracer RayTracerGroup RenderParams Scene SceneDesc Settings UPSAMPLE_FACTORS
    UpsampleParams _CHECKPOINT_FIELDS _HERE _LIB _dp _f64 _fill_params _filter_array _ip _np_from _p _up _whole chart_of_material halton_sample_cap
    lens_params lens_tag lens_vertices lib low_frame_size np occlusion_params os parse_checkpoint_header probe_grid save_pfm save_ppm to_rgb8
    upsample_arrays
""".split()

RAYTRACER = """
    __del__ GATHER_KERNELS KAT KERNELS STAGES STREAM_COUNTERS _bake _bake_points _chart _check _last_ms bake_device bake_fold bake_lightmap bake_params
    bake_probes bake_rays bake_texels build_photon_map_on_device clear_photons counters debug_walk denoise denoise_device denoise_params find_leaves
    focus_at focus_distance gather_pass halton_index halton_sample kat last_bake_ms last_denoise_ms last_features_ms last_kernel_ms last_lightmap_ms
    last_occlusion_ms last_render_ms last_stage_ms last_upsample_ms leaf_order lens lightmap_device lightmap_dilate lightmap_params lightmap_texels
    local_rows occlusion_params params photon_tables_on_device primary_rays progressive radiance resume run run_device run_features
    run_features_device run_occlusion run_occlusion_device run_upsampled samplePhotons setScene set_content_culling set_counters set_entity_boxes
    set_lens set_pool_slots set_render_mode set_stream set_wide_nodes sort_pairs stream_counters trace tracePhotons tracePhotonsOnDevice
    upload_photon_map upsample upsample_device upsample_params visible visible_rays
""".split()

SCENE = """
    __del__ _err _tex add_checkerboard add_color_texture add_height_fog add_image_texture add_light add_material add_material_tex add_sphere add_triangles
    build_photon_map desc load photon_desc photon_tables rebuild set_ambient set_camera settings tables
""".split()

PROGRESSIVERENDER = """
    __enter__ __exit__ _mine _status close done frame pixels_wanting sample_end save step step_device
""".split()

RAYTRACERGROUP = """
    __del__ _check run run_device setScene set_lens
""".split()


@pytest.mark.parametrize("owner, names", [("gi", MODULE), ("RayTracer", RAYTRACER), ("Scene", SCENE), ("ProgressiveRender", PROGRESSIVERENDER),
                                          ("RayTracerGroup", RAYTRACERGROUP)])
def test_every_name_is_still_there(owner, names):
    obj = gi if owner == "gi" else getattr(gi, owner)
    missing = [n for n in names if not hasattr(obj, n)]
    assert not missing, f"{owner} lost {missing}"


def test_init_only_re_exports():
    import ast
    tree = ast.parse(open(gi.__file__).read())
    assert all(isinstance(n, (ast.Import, ast.ImportFrom)) or (isinstance(n, ast.Expr) and isinstance(n.value, ast.Constant)) for n in tree.body)
