// gi_device.h -- per-lane device functions of the MI355X render hot path (one ray / one pixel per lane): the name everything includes.
//
// The functions stand in the parts below, by topic.  All of them are plain scalar-per-lane code marked GI_HD so that the very same
// functions can also be compiled for the host by tests/host_emul (a CPU build used ONLY by unit tests and sanitizers to check the
// kernel logic without a GPU; the product library never contains it).  Wave-level code (ballots, atomics, LDS carving, launches)
// lives in the parts of gi_kernels.hip (gi_lds.h, gi_pool.h, the .inc files); the per-lane halves of the additions (features, occlusion, bake, lightmap, denoiser)
// stand beside their kernels there, since no CPU build names them.
//
// The parts are included in this order inside namespace gi, and each needs exactly the parts above it; none includes another.
// Each part's header comment names the lines of the reference (moepforfreedom/GI_Raytracer, file:line) its functions follow.
// Arithmetic keeps the reference's operand order (glm 0.9.8 conventions) and is compiled with -ffp-contract=off so that
// hit/miss and traversal decisions agree with the CPU path; see DESIGN.md "Numerics".
#pragma once
#include <stdint.h>
#include <math.h>

namespace gi {

#include "gi_scene.h"       // GI_HD and the constants, the HBM tables, Scene, Counters
#include "gi_math.h"        // V3, Ray, the counter RNG, Halton, the samplers
#include "gi_intersect.h"   // boxes, the height fog, triangle and sphere tests, textures, the entity test
#include "gi_walk.h"        // the octree walks: wide-node (per lane, cooperative) and per-node; trace, visible; the diagnostics
#include "gi_gather.h"      // the photon gather: the leaf lookup, the selection, gather_in_leaf, gather, gather_add
#include "gi_path.h"        // shading and the path stages (the gather's stage glue among them), the camera and pixel loop, photon emission

}  // namespace gi
