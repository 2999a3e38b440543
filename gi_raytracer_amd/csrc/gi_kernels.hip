// gi_kernels.hip -- the translation unit of the gfx950 kernels and of the C ABI of include/gi_hip.h: the name hipcc compiles.
//
// It holds no kernel and no type of its own.  Everything stands in the parts below, by topic: a .h holds device-side types and functions
// (no kernel, no host code), an .inc a topic's kernels together with the host code that launches them.  The parts are included in this
// order, each needs parts above it, and only gi_stages.inc includes another (gi_gather.inc, in front of the finisher that calls into it).
// Per-lane device functions are in gi_device.h and its parts.  No CPU fallback exists: every entry needs a HIP device.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/gi_hip.h"
#include "gi_device.h"
#include "gi_layout.h"

using namespace gi;

#define GI_BLOCK 256

// ------------------------------------------------------------------------------------------------- the streaming pipeline, device side
#include "gi_lds.h"              // the octree top in LDS (LdsNodes, LdsWideT, LdsSrc) and the executed-work counters
#include "gi_pool.h"             // the path pool: one array per group of fields, PathRef, the named moves, wave_append, sample_of
#include "gi_pixels.inc"         // the per-pixel records: PixRec, the two record orders, k_render, k_pix_*, k_ad_*, k_pixel_table, k_st_accum
#include "gi_stages.inc"         // the stage kernels: k_st_trace, k_st_shade, k_st_shadow, k_st_compact, the gather (gi_gather.inc), k_st_finish
#include "gi_photon_tables.inc"  // the photon map's derived tables, made at upload: k_pleaf_rank, k_pcand_*, k_pdescent, k_pjump

// ------------------------------------------------------------------------------------------------- host side, and the kernels that stand with it
#include "gi_context.inc"        // gi_ctx and its parts: scene, photon map, tuning, stage clock, stream workspaces, auxiliary passes
#include "gi_instances.inc"      // the kernel instances with dynamic LDS, their tables and selectors
#include "gi_sort.inc"           // the radix sort of the queues: kernels and rs_sort_pairs
#include "gi_photon_build.inc"   // the photon map built on the device: kernels and build_photon_map_on_device
#include "gi_stream.inc"         // the scheduler: stream_samples, run_rounds, stream_passes
#include "gi_api.inc"            // create / destroy, uploads, setters, the frame, its timers and counters
#include "gi_progressive.inc"    // progressive sessions (gi_progressive_*)
#include "gi_denoise.inc"        // the a-trous denoiser: kernels and gi_denoise_*
#include "gi_upsample.inc"       // the guided upsampler: kernel and gi_upsample_*
#include "gi_features.inc"       // first-hit feature buffers: k_aov and gi_render_features_*; the host frame of the per-pixel passes
#include "gi_occlusion.inc"      // ambient occlusion: k_ao and gi_render_occlusion_*
#include "gi_entries.inc"        // function-level entries (parity tests, public C++ methods) and the debug entries
#include "gi_lens.inc"           // the thin lens: gi_set_lens, its vertex table, gi_debug_primary_rays, gi_focus_distance
#include "gi_bake.inc"           // light baking: k_bake_gen, k_bake_fold and gi_bake_*
#include "gi_lightmap.inc"       // lightmap atlases: k_lm_raster, k_lm_point, the rank, k_lm_scatter, k_lm_dilate and gi_lightmap_*
#include "gi_cubemap.inc"        // reflection probes: the capture's source for k_bake_gen, k_cm_box, k_cm_filter, k_cm_resolve and gi_cubemap_*
#include "gi_baked.inc"          // the baked-light pass: k_lit and gi_render_baked_*, the consumer of probes and cube chains
#include "gi_finalgather.inc"    // the final gather: k_fg and gi_render_final_gather_*, one bounce from the first hits into the baked light
#include "gi_visibility.inc"     // probe visibility: k_pv_capture and gi_probe_visibility_*; gi_render_baked_visibility_*, the PV instances of k_lit
#include "gi_reflections.inc"    // reflection probe sets: gi_render_baked_reflections_*, the RS instances of k_lit
#include "gi_group.inc"          // one frame over several devices (gi_group_*)
