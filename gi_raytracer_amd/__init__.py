"""gi_raytracer_amd -- Python host mirror of the MI355X render hot path of GI_Raytracer.

Thin ctypes binding over the C ABI (include/gi_hip.h, gi_raytracer_amd/csrc/gi_host.h) of libgi_raytracer_hip.so.
The names mirror the reference's C++ surface for this path: `Scene` plays Octree (+ the loaders that fill it),
`RayTracer` plays RayTracer (setScene / run / trace / visible / samplePhotons / tracePhotons).  There is no CPU
implementation behind these classes: creating a RayTracer without the HIP library or without a GPU raises.
"""
import ctypes as C  # noqa: F401
import os  # noqa: F401

import numpy as np  # noqa: F401

# LIB_PATH and _LIB are copies taken at import: the live values, the ones lib() reads and sets, are in _abi
from ._abi import (ABI_SYMBOLS, BAKE_MODES, BAKE_SH9, BAKE_TEXEL, BAKED_DIFFUSE, BAKED_DIRECT, BAKED_EMISSIVE, BAKED_SPECULAR, CUBEMAP_MAX_LEVELS, DEFAULT_SEED, GI_E_CANCELLED, GI_E_HIP, GI_E_INVALID,  # noqa: F401
                   GI_E_NO_DEVICE, GI_E_STATE, GI_OK, LIB_PATH, LM_BILINEAR, LM_FILTERS, LM_NEAREST, PROBE_VISIBILITY_MAX_SIZE, REFLECTIONS_MAX_PROBES, SIGNATURES, STRUCTS, BakedLightmapParams, BakedParams, BakedReflectionsParams, BakedVisibilityParams, BakeParams, CubemapParams, DenoiseParams, FinalGatherParams, GiError, Lens,
                   LightmapParams, OcclusionParams, PhotonMapDesc, ProbeVisibilityParams, RenderParams, SceneDesc, Settings, UpsampleParams, _HERE, _LIB, _dp, _f64, _ip,
                   _np_from, _p, _up, lib)
from .params import (FINAL_GATHER_MAX_DIRS, LENS_BLADES, OCCLUSION_MAX_DIRS, UPSAMPLE_FACTORS, _fill_params, _filter_array, _whole, baked_lightmap_params, baked_params, baked_reflections_params, baked_visibility_params, final_gather_params, halton_sample_cap,  # noqa: F401
                     lens_params, lens_tag, lens_vertices, low_frame_size, occlusion_params, upsample_arrays)
from .scene import Scene, chart_of_material, cube_directions, cube_texel_of, octa_decode, octa_encode, probe_grid, reflection_probe_cells, save_pfm, save_ppm, to_rgb8  # noqa: F401
from .sessions import (CHECKPOINT_HEADER, CHECKPOINT_MAGIC, CHECKPOINT_RECORD_BYTES, CHECKPOINT_VERSION, _CHECKPOINT_FIELDS,  # noqa: F401
                       ProgressiveRender, RayTracerGroup, parse_checkpoint_header)
from .tracer import RayTracer  # noqa: F401
