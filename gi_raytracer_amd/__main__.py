"""Headless renderer: what the reference's main.cpp + Viewer do, without Qt.

    python -m gi_raytracer_amd scene.scn -o out.ppm [--pfm out.pfm] [--width 1000 --height 1000] [--samples MIN MAX [THRESH]] [--photons N]
                               [--features PREFIX [--feature-samples N]]
                               [--denoise OUT.ppm [--denoise-pfm OUT.pfm] [--denoise-iterations N] [--denoise-sigmas C N Z A]]
                               [--progressive N [--time-limit SECONDS] [--checkpoint FILE]]
                               [--upsample S [--upsample-pfm LOW.pfm]]
                               [--occlusion PREFIX [--occlusion-samples N] [--occlusion-dirs K] [--occlusion-radius R]]
                               [--aperture R [--blades N] [--blade-rotation DEG] [--focus D | --focus-pixel X Y]]
                               [--baked PREFIX [--baked-samples N] [--baked-probes NX NY NZ] [--baked-reflection X Y Z]
                                [--baked-lightmap W H [--lightmap-samples N]] [--probe-visibility M]
                                [--baked-reflections NX NY NZ [--baked-reflection-fade F]] [--final-gather DIRS]]
    python -m gi_raytracer_amd scene.scn --probes NX NY NZ [--probe-samples N] [--photons N] -o OUT.npy
    python -m gi_raytracer_amd scene.scn --lightmap W H [--lightmap-material M] [--lightmap-samples N] [--lightmap-dilate D] [--photons N]
                               -o OUT.ppm [--pfm OUT.pfm]
    python -m gi_raytracer_amd scene.scn --reflection-probe X Y Z [--probe-face N] [--probe-samples N] [--probe-levels L] [--photons N] -o OUT.npz

The scene file's own `samples` / `photons` / `camera` lines apply unless overridden, exactly as loadScene sets RayTracer's fields
(include/sceneLoader.cpp:160-179); the frame size defaults to the reference window, 1000 x 1000 (main.cpp:43).
--features PREFIX (an addition to the reference's program) also writes the first-hit feature buffers of the frame: PREFIX_albedo.pfm,
PREFIX_normal.pfm (three channels), PREFIX_depth.pfm, PREFIX_coverage.pfm (one channel).
--denoise OUT.ppm (an addition as well) runs the feature pass and the edge-avoiding a-trous denoiser on the frame and writes the result next to
the frame, which is written as without the flag.
--progressive N (an addition too) renders the frame in steps of N samples per pixel and rewrites -o (and --pfm) after every step, through a
temporary file and a rename, so a viewer never reads half a file; the last step leaves the bytes of the run without the flag.  --time-limit
SECONDS takes no further step once the frame's budget is spent (at least one step is taken); --checkpoint FILE resumes from FILE when it exists
-- the scene, --photons and the frame size must be those of the run that wrote it; its sample settings apply -- and saves to it after every step.
--features and --denoise act on the last frame written.
--upsample S (an addition again, S = 2 .. 8 dividing --width and --height) renders the frame at 1/S of the size -- 1/S^2 of the paths -- and scales it
up with the guided upsampler, led by feature buffers of both sizes; --width and --height stay the size of what is written: -o and --pfm get the
upsampled frame, --features the full-size buffers, and --denoise the low frame denoised and then upsampled.  --upsample-pfm LOW.pfm also keeps the
reduced-size render itself.  Not together with --progressive.
--occlusion PREFIX (one more addition) also writes the ambient occlusion of the frame, at --width x --height: PREFIX.open.pfm (one channel, 1 = nothing
within the radius) and PREFIX.bent.pfm (three channels, the mean free direction).  --occlusion-samples N samples per pixel and --occlusion-dirs K
segments per sample (default 16 and 16), --occlusion-radius R their length (default 0: a tenth of the scene box's diagonal).
--aperture R (a further addition) renders through a thin lens of radius R (scene units; 0 = the pinhole) instead of the reference's pinhole: depth
of field.  --blades N (3 .. 16, default 6) and --blade-rotation DEG shape the aperture, a regular polygon.  The plane that stays sharp is the
camera's sensor plane, focal_dist in front of it; --focus D moves it to distance D, --focus-pixel X Y to the first surface behind the centre of
that pixel (the field of view is kept).  Every other flag renders under the lens: --features, --occlusion, --progressive (a checkpoint resumes
only under the lens it was written with), --denoise, --upsample.
--probes NX NY NZ (an addition as well) renders no frame: it bakes a regular grid of light probes inside the octree's root box, one at the centre
of each of the NX x NY x NZ cells, with --probe-samples N rays each (default 256), after the photon pass, and writes their spherical-harmonic
coefficients to -o as a numpy array [NZ][NY][NX][9][3] (float32; include/gi_hip.h: GI_BAKE_SH9).  The frame's flags do not go with it.
--lightmap W H (an addition too) renders no frame either: it bakes a W x H lightmap atlas (include/gi_hip.h: gi_lightmap_*) over the scene's own
texture coordinates, read as an unwrapped chart (v grows downwards) -- of the triangles of material index --lightmap-material M, or of all triangles
-- with --lightmap-samples N rays per covered texel (default 256) and --lightmap-dilate D gutter passes (default 2), after the photon pass.  -o gets
the 8-bit PPM of the display transform, --pfm the linear atlas; one line gives the number of covered texels and the device time.
--reflection-probe X Y Z (one more addition) renders no frame either: it captures a reflection probe at that position (include/gi_hip.h:
gi_cubemap_*) -- a cube map of --probe-face N texels per face edge (default 32) with --probe-samples N rays per texel (default 64) -- and filters
--probe-levels L levels of its roughness chain (default 1: the capture alone; N must be divisible by 2^(L-1)), after the photon pass.  -o gets a
numpy .npz with the keys level0, level1 ... as float32 [6][N >> l][N >> l][3].  Not together with --probes or --lightmap.
--baked PREFIX (the consumer of those bakes; include/gi_hip.h: gi_render_baked_*) also writes a preview of the frame shaded from baked light, at
--width x --height: after the photon pass it bakes a grid of --baked-probes NX NY NZ light probes (default 4 4 4, 256 rays each) in the octree's
root box and a reflection probe at --baked-reflection X Y Z (default: the middle of that box; face 32, 64 rays per texel, 6 levels), then shades
every pixel's first hit with --baked-samples N samples (default 4) from the lights, the probes and the cube.  PREFIX.ppm gets the display
transform of the preview, PREFIX_direct.pfm, PREFIX_diffuse.pfm and PREFIX_specular.pfm its three terms.  It goes with the frame's flags as
--occlusion does, not with --probes, --lightmap or --reflection-probe.  If -o is not given and PREFIX.ppm is the frame's default name, the frame
goes to PREFIX_frame.ppm.
--baked-lightmap W H (with --baked; include/gi_hip.h: gi_render_baked_lightmap_*) also bakes a W x H lightmap atlas over the scene's texture
coordinates, as --lightmap does for all triangles, with --lightmap-samples N rays per covered texel (default 256) and 2 gutter passes, and the
preview's diffuse surfaces read it: a first hit on a charted triangle takes its diffuse light from the atlas, every other one from the probes.  One
more line names the atlas size and the texels covered.
--probe-visibility M (with --baked; include/gi_hip.h: gi_probe_visibility_*, gi_render_baked_visibility_*) also bakes an M x M octahedral visibility
map (M = 1 .. 64, 16 rays per texel, distances up to the scene box's diagonal) at every probe of the --baked-probes grid -- the grid probe_grid
gives -- and the preview looks the probes up through them: a probe behind a wall no longer lights the hit.  It needs that grid, so it is refused
without --baked, and it does not go with --baked-lightmap (the lightmap entry takes no maps).
--baked-reflections NX NY NZ (with --baked; include/gi_hip.h: gi_render_baked_reflections_*) bakes a SET of reflection probes instead of the one:
the scene's box is cut into NX x NY x NZ cells (at most 64), a chain is baked at every cell's centre, every cell grown by --baked-reflection-fade F
(default: a tenth of the cell's shortest edge) is its probe's influence box, and the preview's mirror and glossy surfaces read each cube at the
direction projected onto that box, blending where boxes overlap: reflections line up with the walls they show.  One more line names the set.
--baked-reflection X Y Z has no part in it; it does not go with --baked-lightmap or --probe-visibility (one look-up per call).
--final-gather DIRS (with --baked; include/gi_hip.h: gi_render_final_gather_*) renders the same four images from the same grid and chain through the
final-gather pass: a diffuse first hit shoots DIRS (1 .. 64) cosine-distributed rays and takes the mean of what they hit, shaded from the lights, the
grid, the chain and emission, so the grid is read one bounce away.  It reads the plain grid and one chain: not together with --baked-lightmap,
--probe-visibility or --baked-reflections.
"""
import argparse
import os
import sys
import time

import gi_raytracer_amd as gi


FEATURE_FILES = ("albedo", "normal", "depth", "coverage")
PROBE_SAMPLES = 256
LIGHTMAP_SAMPLES = 256
REFLECTION_FACE, REFLECTION_SAMPLES = 32, 64
BAKED_SAMPLES, BAKED_PROBES, BAKED_LEVELS = 4, (4, 4, 4), 6
BAKED_FILES = ("direct", "diffuse", "specular")
VISIBILITY_SAMPLES, VISIBILITY_MAX_SIZE = 16, gi.PROBE_VISIBILITY_MAX_SIZE
REFLECTIONS_MAX_PROBES, REFLECTIONS_FADE = gi.REFLECTIONS_MAX_PROBES, 0.1      # the default fade: this share of a cell's shortest edge


def parser():
    ap = argparse.ArgumentParser(prog="python -m gi_raytracer_amd", description=__doc__.split("\n")[0])
    ap.add_argument("scene")
    ap.add_argument("-o", "--output", default=None, help="(default out.ppm) " + "8-bit PPM of the display transform (gamma 2.2, clamp)")
    ap.add_argument("--pfm", default=None, help="also write the linear radiance as PFM")
    ap.add_argument("--width", type=int, default=1000)
    ap.add_argument("--height", type=int, default=1000)
    ap.add_argument("--samples", type=float, nargs="+", default=None, metavar="N", help="min max [noise threshold]")
    ap.add_argument("--photons", type=int, default=None)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--features", default=None, metavar="PREFIX", help="also write the first-hit feature buffers as PREFIX_{albedo,normal,depth,coverage}.pfm")
    ap.add_argument("--feature-samples", type=int, default=None, metavar="N",
                    help="samples per pixel of the feature buffers (default: the frame's max samples, cut to what the Halton index of the frame size allows)")
    ap.add_argument("--denoise", default=None, metavar="OUT.ppm", help="also write the denoised frame (a-trous filter guided by the feature buffers) as 8-bit PPM")
    ap.add_argument("--denoise-pfm", default=None, metavar="OUT.pfm", help="with --denoise: the denoised linear radiance as PFM")
    ap.add_argument("--denoise-iterations", type=int, default=None, metavar="N", help="levels of the filter, 0 .. 8 (default 5)")
    ap.add_argument("--denoise-sigmas", type=float, nargs=4, default=None, metavar=("C", "N", "Z", "A"),
                    help="sigmas of colour, normal, depth and albedo (default 1.0 0.5 0.1 0.25; 0 switches a term off)")
    ap.add_argument("--progressive", type=int, default=None, metavar="N", help="render in steps of N samples per pixel, rewriting the output after every step")
    ap.add_argument("--time-limit", type=float, default=None, metavar="SECONDS", help="with --progressive: take no further step once this much time went into the frame")
    ap.add_argument("--checkpoint", default=None, metavar="FILE", help="with --progressive: resume from FILE when it exists, save the session to it after every step")
    ap.add_argument("--upsample", type=int, default=None, metavar="S", help="render at 1/S of --width x --height (S = 2 .. 8, dividing both) and scale up with the guided upsampler")
    ap.add_argument("--upsample-pfm", default=None, metavar="LOW.pfm", help="with --upsample: also write the reduced-size render (linear radiance) as PFM")
    ap.add_argument("--occlusion", default=None, metavar="PREFIX", help="also write ambient occlusion and bent normals as PREFIX.open.pfm and PREFIX.bent.pfm")
    ap.add_argument("--occlusion-samples", type=int, default=None, metavar="N", help="with --occlusion: samples per pixel (default 16)")
    ap.add_argument("--occlusion-dirs", type=int, default=None, metavar="K", help="with --occlusion: segments per sample, 1 .. 64 (default 16)")
    ap.add_argument("--occlusion-radius", type=float, default=None, metavar="R", help="with --occlusion: length of a segment (default 0: a tenth of the scene box's diagonal)")
    ap.add_argument("--aperture", type=float, default=None, metavar="R", help="render through a thin lens of radius R in scene units (0: the pinhole)")
    ap.add_argument("--blades", type=int, default=None, metavar="N", help="with --aperture: blades of the aperture, 3 .. 16 (default 6)")
    ap.add_argument("--blade-rotation", type=float, default=None, metavar="DEG", help="with --aperture: rotation of the aperture in degrees (default 0)")
    ap.add_argument("--focus", type=float, default=None, metavar="D", help="with --aperture: distance of the plane that stays sharp (default: the camera's focal distance)")
    ap.add_argument("--focus-pixel", type=int, nargs=2, default=None, metavar=("X", "Y"), help="with --aperture: focus on the first surface behind the centre of this pixel")
    ap.add_argument("--probes", type=int, nargs=3, default=None, metavar=("NX", "NY", "NZ"), help="bake a grid of light probes in the scene's box instead of a frame; -o gets a .npy [NZ][NY][NX][9][3]")
    ap.add_argument("--probe-samples", type=int, default=None, metavar="N", help="with --probes: rays per probe (default 256); with --reflection-probe: rays per texel (default 64)")
    ap.add_argument("--reflection-probe", type=float, nargs=3, default=None, metavar=("X", "Y", "Z"), help="capture a reflection probe at this position instead of a frame; -o gets a .npz of level0, level1 ...")
    ap.add_argument("--probe-face", type=int, default=None, metavar="N", help="with --reflection-probe: texels per face edge (default 32)")
    ap.add_argument("--probe-levels", type=int, default=None, metavar="L", help="with --reflection-probe: levels of the roughness chain, 1 .. 12 (default 1: the capture alone)")
    ap.add_argument("--lightmap", type=int, nargs=2, default=None, metavar=("W", "H"), help="bake a W x H lightmap atlas over the scene's texture coordinates instead of a frame")
    ap.add_argument("--lightmap-material", type=int, default=None, metavar="M", help="with --lightmap: only the triangles of this material index (default: all triangles)")
    ap.add_argument("--lightmap-samples", type=int, default=None, metavar="N", help="with --lightmap: rays per covered texel (default 256)")
    ap.add_argument("--lightmap-dilate", type=int, default=None, metavar="D", help="with --lightmap: gutter dilation passes, 0 .. 64 (default 2)")
    ap.add_argument("--baked", default=None, metavar="PREFIX", help="also write a preview shaded from baked light as PREFIX.ppm and its terms as PREFIX_{direct,diffuse,specular}.pfm")
    ap.add_argument("--baked-samples", type=int, default=None, metavar="N", help="with --baked: samples per pixel (default 4)")
    ap.add_argument("--baked-probes", type=int, nargs=3, default=None, metavar=("NX", "NY", "NZ"), help="with --baked: the light-probe grid in the scene's box (default 4 4 4)")
    ap.add_argument("--baked-lightmap", type=int, nargs=2, default=None, metavar=("W", "H"), help="with --baked: bake a W x H lightmap over the scene's texture coordinates and shade charted diffuse surfaces from it")
    ap.add_argument("--probe-visibility", type=int, default=None, metavar="M", help="with --baked: bake an M x M visibility map per probe of the grid and look the probes up through them (no light leaks through walls)")
    ap.add_argument("--baked-reflections", type=int, nargs=3, default=None, metavar=("NX", "NY", "NZ"), help="with --baked: bake one reflection probe per cell of the scene's box cut NX x NY x NZ and shade mirror and glossy surfaces from the set, box-projected and blended")
    ap.add_argument("--baked-reflection-fade", type=float, default=None, metavar="F", help="with --baked-reflections: how far every cell's influence box reaches beyond the cell, the band probes blend over (default: a tenth of the cell's shortest edge)")
    ap.add_argument("--final-gather", type=int, default=None, metavar="DIRS", help="with --baked: shade diffuse first hits by a final gather of DIRS (1 .. 64) rays into the baked light instead of reading the grid at the hit")
    ap.add_argument("--baked-reflection", type=float, nargs=3, default=None, metavar=("X", "Y", "Z"), help="with --baked: position of the reflection probe (default: the middle of the scene's box)")
    return ap


def lens_of(a):
    """The Lens the --aperture flags ask for (ValueError for bad values), or None without --aperture."""
    if a.aperture is None:
        return None
    import math
    return gi.lens_params(radius=a.aperture, blades=a.blades, rotation=None if a.blade_rotation is None else math.radians(a.blade_rotation))


def check_args(ap, a):
    """The rules between the flags; ap.error (exit status 2) on a breach.  Runs before anything touches the device."""
    explicit_output = a.output is not None
    if not explicit_output:
        a.output = "out.ppm"
    if a.baked is None and (a.baked_samples is not None or a.baked_probes is not None or a.baked_reflection is not None or a.baked_lightmap is not None):
        ap.error("--baked-samples, --baked-probes, --baked-reflection and --baked-lightmap need --baked PREFIX")
    if a.baked is None and (a.baked_reflections is not None or a.baked_reflection_fade is not None):
        ap.error("--baked-reflections NX NY NZ and --baked-reflection-fade F need --baked PREFIX")
    if a.baked_reflections is None and a.baked_reflection_fade is not None:
        ap.error("--baked-reflection-fade F needs --baked-reflections NX NY NZ")
    if a.baked is None and a.final_gather is not None:
        ap.error("--final-gather DIRS needs the grid and the chain of --baked PREFIX")
    if a.baked is None and a.probe_visibility is not None:
        ap.error("--probe-visibility M needs the probe grid of --baked PREFIX [--baked-probes NX NY NZ]")
    if a.baked is not None:
        if a.probes is not None or a.lightmap is not None or a.reflection_probe is not None:
            ap.error("--baked does not go together with --probes, --lightmap or --reflection-probe")
        ns = BAKED_SAMPLES if a.baked_samples is None else a.baked_samples
        if ns < 1 or ns > gi.halton_sample_cap(a.width, a.height):
            ap.error(f"--baked-samples N: from 1 to {gi.halton_sample_cap(a.width, a.height)} for a {a.width} x {a.height} frame")
        grid = a.baked_probes or BAKED_PROBES
        if min(grid) < 1 or grid[0] * grid[1] * grid[2] * PROBE_SAMPLES > 2 ** 32:
            ap.error("--baked-probes NX NY NZ: three numbers >= 1; probes x 256 samples must keep the stream index within 32 bits")
        if a.baked_reflection is not None and not all(-float("inf") < v < float("inf") for v in a.baked_reflection):
            ap.error("--baked-reflection X Y Z: three finite numbers")
        if a.baked_lightmap is not None:
            w, h = a.baked_lightmap
            if not (1 <= w <= 8192 and 1 <= h <= 8192):
                ap.error("--baked-lightmap W H: two numbers from 1 to 8192")
            if a.lightmap_samples is not None and a.lightmap_samples < 1:
                ap.error("--lightmap-samples N: N must be at least 1")
            if w * h * (a.lightmap_samples or LIGHTMAP_SAMPLES) > 2 ** 32:
                ap.error("--baked-lightmap: texels x samples must keep the stream index within 32 bits")
        if a.probe_visibility is not None:
            if a.baked_lightmap is not None:
                ap.error("--probe-visibility does not go together with --baked-lightmap: the lightmap pass takes no visibility maps")
            m = a.probe_visibility
            if not 1 <= m <= VISIBILITY_MAX_SIZE or grid[0] * grid[1] * grid[2] * m * m * VISIBILITY_SAMPLES > 2 ** 32:
                ap.error(f"--probe-visibility M: from 1 to {VISIBILITY_MAX_SIZE}; probes x M x M x {VISIBILITY_SAMPLES} samples must keep the stream index within 32 bits")
        if a.baked_reflections is not None:
            if a.baked_lightmap is not None or a.probe_visibility is not None:
                ap.error("--baked-reflections does not go together with --baked-lightmap or --probe-visibility: one look-up per call")
            if a.baked_reflection is not None:
                ap.error("--baked-reflections places its probes itself: not together with --baked-reflection X Y Z")
            cells = a.baked_reflections
            if min(cells) < 1 or cells[0] * cells[1] * cells[2] > REFLECTIONS_MAX_PROBES:
                ap.error(f"--baked-reflections NX NY NZ: three numbers >= 1 with at most {REFLECTIONS_MAX_PROBES} cells")
            if a.baked_reflection_fade is not None and not 0.0 <= a.baked_reflection_fade < float("inf"):
                ap.error("--baked-reflection-fade F: a finite number >= 0")
        if a.final_gather is not None:
            if a.baked_lightmap is not None or a.probe_visibility is not None or a.baked_reflections is not None:
                ap.error("--final-gather reads the plain grid and one chain: not together with --baked-lightmap, --probe-visibility or --baked-reflections")
            if not 1 <= a.final_gather <= gi.FINAL_GATHER_MAX_DIRS:
                ap.error(f"--final-gather DIRS: from 1 to {gi.FINAL_GATHER_MAX_DIRS}")
        if os.path.abspath(a.baked + ".ppm") == os.path.abspath(a.output):
            if explicit_output:
                ap.error(f"--baked {a.baked} writes {a.baked}.ppm, which is -o: name one of them differently")
            a.output = a.baked + "_frame.ppm"
    if a.denoise is None and (a.denoise_pfm or a.denoise_iterations is not None or a.denoise_sigmas is not None):
        ap.error("--denoise-pfm, --denoise-iterations and --denoise-sigmas need --denoise OUT.ppm")
    if a.progressive is None and (a.time_limit is not None or a.checkpoint is not None):
        ap.error("--time-limit and --checkpoint need --progressive N")
    if a.progressive is not None and a.progressive < 1:
        ap.error("--progressive N: N must be at least 1")
    if a.time_limit is not None and not a.time_limit >= 0:
        ap.error("--time-limit SECONDS: a number >= 0")
    if a.probes is None and a.reflection_probe is None and a.probe_samples is not None:
        ap.error("--probe-samples needs --probes NX NY NZ or --reflection-probe X Y Z")
    if a.reflection_probe is None and (a.probe_face is not None or a.probe_levels is not None):
        ap.error("--probe-face and --probe-levels need --reflection-probe X Y Z")
    if a.reflection_probe is not None:
        if a.probes is not None or a.lightmap is not None:
            ap.error("--reflection-probe does not go together with --probes or --lightmap")
        face = REFLECTION_FACE if a.probe_face is None else a.probe_face
        ns = REFLECTION_SAMPLES if a.probe_samples is None else a.probe_samples
        levels = 1 if a.probe_levels is None else a.probe_levels
        if not all(-float("inf") < v < float("inf") for v in a.reflection_probe):
            ap.error("--reflection-probe X Y Z: three finite numbers")
        if face < 1 or ns < 1 or not 1 <= levels <= gi.CUBEMAP_MAX_LEVELS:
            ap.error(f"--probe-face N and --probe-samples N must be at least 1, --probe-levels L from 1 to {gi.CUBEMAP_MAX_LEVELS}")
        if face % (1 << (levels - 1)):
            ap.error(f"--probe-levels {levels} needs a --probe-face divisible by {1 << (levels - 1)}")
        if 6 * face * face * ns > 2 ** 32:
            ap.error("--reflection-probe: texels x samples must keep the stream index within 32 bits")
        frame_flags = (a.pfm, a.samples, a.features, a.feature_samples, a.denoise, a.progressive, a.upsample, a.occlusion, a.aperture)
        if any(f is not None for f in frame_flags):
            ap.error("--reflection-probe renders no frame: only --probe-*, --photons, --device and -o go with it")
    if a.probes is not None:
        if min(a.probes) < 1 or a.probes[0] * a.probes[1] * a.probes[2] >= 2 ** 31:
            ap.error("--probes NX NY NZ: three numbers >= 1, fewer than 2^31 probes in all")
        if a.probe_samples is not None and a.probe_samples < 1:
            ap.error("--probe-samples N: N must be at least 1")
        if a.probes[0] * a.probes[1] * a.probes[2] * (a.probe_samples or PROBE_SAMPLES) > 2 ** 32:
            ap.error("--probes: probes x samples must keep the stream index within 32 bits")
        frame_flags = (a.pfm, a.samples, a.features, a.feature_samples, a.denoise, a.progressive, a.upsample, a.occlusion, a.aperture)
        if any(f is not None for f in frame_flags):
            ap.error("--probes renders no frame: only --photons, --probe-samples, --device and -o go with it")
    if a.lightmap is None and (a.lightmap_material is not None or (a.lightmap_samples is not None and a.baked_lightmap is None) or a.lightmap_dilate is not None):
        ap.error("--lightmap-material, --lightmap-samples and --lightmap-dilate need --lightmap W H (--lightmap-samples also goes with --baked-lightmap W H)")
    if a.lightmap is not None:
        w, h = a.lightmap
        if not (1 <= w <= 8192 and 1 <= h <= 8192):
            ap.error("--lightmap W H: two numbers from 1 to 8192")
        if a.lightmap_samples is not None and a.lightmap_samples < 1:
            ap.error("--lightmap-samples N: N must be at least 1")
        if a.lightmap_dilate is not None and not 0 <= a.lightmap_dilate <= 64:
            ap.error("--lightmap-dilate D: D from 0 to 64")
        if a.lightmap_material is not None and a.lightmap_material < 0:
            ap.error("--lightmap-material M: a material index >= 0")
        if w * h * (a.lightmap_samples or LIGHTMAP_SAMPLES) > 2 ** 32:
            ap.error("--lightmap: texels x samples must keep the stream index within 32 bits")
        frame_flags = (a.samples, a.features, a.feature_samples, a.denoise, a.progressive, a.upsample, a.occlusion, a.aperture, a.probes)
        if any(f is not None for f in frame_flags):
            ap.error("--lightmap renders no frame: only --lightmap-*, --photons, --device, -o and --pfm go with it")
    if a.upsample is None and a.upsample_pfm:
        ap.error("--upsample-pfm needs --upsample S")
    if a.occlusion is None and (a.occlusion_samples is not None or a.occlusion_dirs is not None or a.occlusion_radius is not None):
        ap.error("--occlusion-samples, --occlusion-dirs and --occlusion-radius need --occlusion PREFIX")
    if a.occlusion is not None:
        try:
            gi.occlusion_params(**occlusion_kwargs(a), width=a.width, height=a.height)
        except ValueError as e:
            ap.error(f"--occlusion: {e}")
    if a.aperture is None and (a.blades is not None or a.blade_rotation is not None or a.focus is not None or a.focus_pixel is not None):
        ap.error("--blades, --blade-rotation, --focus and --focus-pixel need --aperture R")
    if a.focus is not None and a.focus_pixel is not None:
        ap.error("--focus D and --focus-pixel X Y do not go together")
    if a.focus is not None and not 0 < a.focus < float("inf"):
        ap.error("--focus D: a finite distance > 0")
    if a.focus_pixel is not None and not (0 <= a.focus_pixel[0] < a.width and 0 <= a.focus_pixel[1] < a.height):
        ap.error(f"--focus-pixel X Y: a pixel of the {a.width} x {a.height} frame")
    try:
        lens_of(a)
    except ValueError as e:
        ap.error(f"--aperture: {e}")
    if a.upsample is not None:
        if a.progressive is not None:
            ap.error("--upsample and --progressive do not go together")
        try:
            gi.low_frame_size(a.width, a.height, a.upsample)
        except ValueError as e:
            ap.error(f"--upsample S: {e}")


def replace_file(path, write):
    """write(tmp) then rename over path: a reader sees the old file or the new one, never a part of one."""
    tmp = f"{path}.part"
    try:
        write(tmp)
    except BaseException:
        if os.path.exists(tmp):
            os.remove(tmp)
        raise
    os.replace(tmp, path)


def write_bytes(path, data):
    with open(path, "wb") as f:
        f.write(data)


def write_npz(path, arrays):
    import numpy as np
    with open(path, "wb") as f:      # (np.savez would add ".npz" to a name without it)
        np.savez(f, **arrays)


def write_npy(path, array):
    import numpy as np
    with open(path, "wb") as f:      # (np.save would add ".npy" to a name without it)
        np.save(f, array)


def render_progressive(a, rt):
    """The frame in steps of a.progressive samples; returns (frame, spp, a note for the summary line)."""
    resumed = a.checkpoint is not None and os.path.exists(a.checkpoint)
    if resumed:
        with open(a.checkpoint, "rb") as f:
            blob = f.read()
        h = gi.parse_checkpoint_header(blob)
        if (h["width"], h["height"]) != (a.width, a.height):
            raise SystemExit(f"{a.checkpoint}: a checkpoint of a {h['width']} x {h['height']} frame, not {a.width} x {a.height}")
        sess = rt.resume(blob)
        if (h["min_samples"], h["max_samples"], h["noise_thresh"]) != (rt.min_samples, rt.max_samples, rt.noise_thresh):
            print(f"{a.checkpoint}: resuming with the checkpoint's sample settings (min {h['min_samples']}, max {h['max_samples']}, noise threshold "
                  f"{h['noise_thresh']}), not those of this run (min {rt.min_samples}, max {rt.max_samples}, noise threshold {rt.noise_thresh})", file=sys.stderr)
        rt.min_samples, rt.max_samples, rt.noise_thresh = h["min_samples"], h["max_samples"], h["noise_thresh"]
    else:
        sess = rt.progressive(a.width, a.height)
    t0 = time.time()
    steps, first = 0, sess.sample_end
    with sess:
        while True:
            lin, spp = sess.step(a.progressive, f64=False, want_spp=True)
            steps += 1
            replace_file(a.output, lambda t: gi.save_ppm(t, lin))
            if a.pfm:
                replace_file(a.pfm, lambda t: gi.save_pfm(t, lin))
            if a.checkpoint:
                blob = sess.save()
                replace_file(a.checkpoint, lambda t: write_bytes(t, blob))
            done, end = sess.done, sess.sample_end
            if done or end >= rt.max_samples:
                why = "finished"
                break
            if a.time_limit is not None and time.time() - t0 >= a.time_limit:
                why = "time limit reached, frame unfinished"
                break
    note = f"; progressive: {steps} step(s) of {a.progressive}, samples {first} .. {end} of {rt.max_samples} offered per pixel ({why})"
    return lin, spp, note + (f", resumed from {a.checkpoint}" if resumed else "")


def denoise_kwargs(a):
    """The keyword arguments of RayTracer.denoise the --denoise-* flags set."""
    kw = {}
    if a.denoise_iterations is not None:
        kw["iterations"] = a.denoise_iterations
    if a.denoise_sigmas is not None:
        kw.update(zip(("sigma_color", "sigma_normal", "sigma_depth", "sigma_albedo"), a.denoise_sigmas))
    return kw


def occlusion_kwargs(a):
    """The keyword arguments of RayTracer.run_occlusion the --occlusion-* flags set."""
    kw = {"n": a.occlusion_samples, "dirs": a.occlusion_dirs, "radius": a.occlusion_radius}
    return {k: v for k, v in kw.items() if v is not None}


def render_baked(a, rt, scene):
    """--baked: the probe grid and the reflection probe baked with the defaults of --probes and --reflection-probe, then the baked-light pass;
    writes the four files and returns a note for the summary line."""
    box = scene.tables()["node_bbox"][0]
    nx, ny, nz = a.baked_probes or BAKED_PROBES
    points = gi.probe_grid(box, nx, ny, nz).reshape(-1, 3)
    sh = rt.bake_probes(points, PROBE_SAMPLES).reshape(nz, ny, nx, 9, 3)
    ns = BAKED_SAMPLES if a.baked_samples is None else a.baked_samples
    note, preview_ms = "", None                     # preview_ms: the time of the pass that made the preview where it is not the baked-light pass
    if a.baked_reflections is not None:
        cx, cy, cz = a.baked_reflections
        fade = a.baked_reflection_fade
        if fade is None:
            fade = REFLECTIONS_FADE * min((box[3 + k] - box[k]) / c for k, c in enumerate((cx, cy, cz)))
        table = gi.reflection_probe_cells(box, cx, cy, cz, fade)
        chains = rt.bake_reflection_probes(table[:, 0:3], REFLECTION_FACE, REFLECTION_SAMPLES, BAKED_LEVELS)
        print(f"{a.scene}: reflection probes {cx}x{cy}x{cz}, {len(table)} chains of face {REFLECTION_FACE} with {BAKED_LEVELS} levels, fade {fade:.4g}")
        lit = rt.run_baked_reflections(a.width, a.height, ns, table, chains, sh=sh, grid_box=box, f64=False, face=REFLECTION_FACE, levels=BAKED_LEVELS)
        gi.save_ppm(f"{a.baked}.ppm", lit["beauty"])
        for name in BAKED_FILES:
            gi.save_pfm(f"{a.baked}_{name}.pfm", lit[name])
        return (f"; baked light {nx} x {ny} x {nz} probes {rt.last_bake_ms():.2f} ms, reflection probes {cx}x{cy}x{cz}, {ns} spp preview {rt.last_baked_ms():.2f} ms "
                f"-> {a.baked}.ppm, {a.baked}_*.pfm")
    pos = a.baked_reflection if a.baked_reflection is not None else [0.5 * (box[k] + box[3 + k]) for k in range(3)]
    chain = rt.bake_reflection_probe(pos, REFLECTION_FACE, REFLECTION_SAMPLES, BAKED_LEVELS)
    if a.baked_lightmap is not None:
        w, h = a.baked_lightmap
        ent, uv = gi.chart_of_material(scene)
        atlas, _, n_cov = rt.bake_lightmap(ent, uv, w, h, a.lightmap_samples or LIGHTMAP_SAMPLES, want_owner=True)
        print(f"{a.scene}: baked lightmap {w}x{h}, {len(ent)} chart triangles, {n_cov} texels covered, {rt.last_lightmap_ms()[0]:.2f} ms")
        lit = rt.run_baked_lightmap(a.width, a.height, ns, atlas, ent, uv, sh=sh, grid_box=box, chain=chain, f64=False)
        note = f", lightmap {w}x{h}"
    elif a.probe_visibility is not None:
        m = a.probe_visibility
        vis = rt.bake_probe_visibility(points, m, VISIBILITY_SAMPLES).reshape(nz, ny, nx, m, m, 2)
        lit = rt.run_baked_visibility(a.width, a.height, ns, vis, sh=sh, grid_box=box, chain=chain, f64=False)
        note = f", visibility maps {m}x{m} {rt.last_probe_visibility_ms():.2f} ms"
    elif a.final_gather is not None:
        lit = rt.run_final_gather(a.width, a.height, ns, dirs=a.final_gather, sh=sh, grid_box=box, chain=chain, f64=False)
        note, preview_ms = f", final gather of {a.final_gather} rays", rt.last_final_gather_ms()
    else:
        lit = rt.run_baked(a.width, a.height, ns, sh=sh, grid_box=box, chain=chain, f64=False)      # (the chain's exponents are the library's defaults, in both calls)
    gi.save_ppm(f"{a.baked}.ppm", lit["beauty"])
    for name in BAKED_FILES:
        gi.save_pfm(f"{a.baked}_{name}.pfm", lit[name])
    return (f"; baked light {nx} x {ny} x {nz} probes {rt.last_bake_ms():.2f} ms, cube {rt.last_cubemap_ms()[0]:.2f} ms{note}, {ns} spp preview {rt.last_baked_ms() if preview_ms is None else preview_ms:.2f} ms "
            f"-> {a.baked}.ppm, {a.baked}_*.pfm")


def feature_samples(a, max_samples):
    """n of the feature pass: --feature-samples, else the frame's max_samples cut to the Halton cap of the frame size."""
    if a.feature_samples is not None:
        return a.feature_samples
    return max(1, min(int(max_samples), gi.halton_sample_cap(a.width, a.height)))


def main(argv=None):
    ap = parser()
    a = ap.parse_args(argv)
    check_args(ap, a)
    scene = gi.Scene.load(a.scene).rebuild()
    rt = gi.RayTracer(a.device).setScene(scene)          # raises without a GPU: there is no CPU path
    if a.samples:
        rt.min_samples = int(a.samples[0])
        rt.max_samples = int(a.samples[1]) if len(a.samples) > 1 else int(a.samples[0])
        if len(a.samples) > 2:
            rt.noise_thresh = float(a.samples[2])
    n_photons = rt.photons if a.photons is None else a.photons
    t0 = time.time()
    stored = 0
    if n_photons > 0 and scene.desc().n_light > 0:
        stored = len(rt.tracePhotons(n_photons)[0])
    t1 = time.time()
    if a.probes:
        import numpy as np
        nx, ny, nz = a.probes
        ns = a.probe_samples or PROBE_SAMPLES
        grid = gi.probe_grid(scene.tables()["node_bbox"][0], nx, ny, nz)
        sh = rt.bake_probes(grid.reshape(-1, 3), ns, f64=False).reshape(nz, ny, nx, 9, 3)
        replace_file(a.output, lambda t: write_npy(t, sh))
        print(f"{a.scene}: {nx} x {ny} x {nz} probes of {ns} samples, {stored} photons stored; photon pass {t1 - t0:.2f} s, "
              f"bake {rt.last_bake_ms():.2f} ms -> {a.output}")
        return 0
    if a.reflection_probe:
        face = REFLECTION_FACE if a.probe_face is None else a.probe_face
        ns = REFLECTION_SAMPLES if a.probe_samples is None else a.probe_samples
        levels = rt.bake_reflection_probe(a.reflection_probe, face, ns, 1 if a.probe_levels is None else a.probe_levels, f64=False)
        replace_file(a.output, lambda t: write_npz(t, {f"level{l}": v for l, v in enumerate(levels)}))
        ms, stages = rt.last_cubemap_ms()
        print(f"{a.scene}: reflection probe at {a.reflection_probe[0]:g} {a.reflection_probe[1]:g} {a.reflection_probe[2]:g}, face {face}, {ns} samples a texel, "
              f"{len(levels)} level(s), {stored} photons stored; photon pass {t1 - t0:.2f} s, probe {ms:.2f} ms (capture {stages['capture']:.2f}, "
              f"prefilter {stages['prefilter']:.2f}) -> {a.output}")
        return 0
    if a.lightmap:
        w, h = a.lightmap
        ns = a.lightmap_samples or LIGHTMAP_SAMPLES
        ent, uv = gi.chart_of_material(scene, a.lightmap_material)
        atlas, _, n_cov = rt.bake_lightmap(ent, uv, w, h, ns, dilate=2 if a.lightmap_dilate is None else a.lightmap_dilate, f64=False, want_owner=True)
        gi.save_ppm(a.output, atlas)
        if a.pfm:
            gi.save_pfm(a.pfm, atlas)
        ms, stages = rt.last_lightmap_ms()
        print(f"{a.scene}: lightmap {w}x{h}, {len(ent)} chart triangles, {n_cov} texels covered, {ns} samples each, {stored} photons stored; "
              f"photon pass {t1 - t0:.2f} s, lightmap {ms:.2f} ms (raster {stages['raster']:.2f}, bake {stages['bake']:.2f}, dilate {stages['dilate']:.2f}) -> {a.output}")
        return 0
    feat = lens_note = ""
    lens = lens_of(a)
    if lens is not None:
        if a.focus_pixel is not None:
            d = rt.focus_distance(a.width, a.height, *a.focus_pixel)
            if d is None or not d > 0:
                raise SystemExit(f"--focus-pixel {a.focus_pixel[0]} {a.focus_pixel[1]}: no surface behind that pixel")
            rt.focus_at(d)
        elif a.focus is not None:
            rt.focus_at(a.focus)
        rt.set_lens(lens=lens)
        lens_note = f"; lens radius {lens.radius:g}, {lens.blades} blades, sharp at {rt.focal_dist:g}"
    S = a.upsample
    if a.progressive:
        lin, spp, feat = render_progressive(a, rt)
        t2 = time.time()
    else:
        rw, rh = gi.low_frame_size(a.width, a.height, S) if S else (a.width, a.height)
        lin, spp = rt.run(rw, rh, f64=False, want_spp=True)
        t2 = time.time()
        if S:
            nf = feature_samples(a, rt.max_samples)
            low, fl = lin, rt.run_features(rw, rh, nf, f64=False, want_ids=False)
            fb = rt.run_features(a.width, a.height, nf, f64=False, want_ids=False)
            lin = rt.upsample(low, fl, fb, S)
            feat = f"; upsampled x{S} from {rw}x{rh} ({nf} spp features) {rt.last_upsample_ms():.2f} ms"
            if a.upsample_pfm:
                gi.save_pfm(a.upsample_pfm, low)
        gi.save_ppm(a.output, lin)
        if a.pfm:
            gi.save_pfm(a.pfm, lin)
    if a.features:
        nf = feature_samples(a, rt.max_samples)
        fb = fb if S else rt.run_features(a.width, a.height, nf, f64=False, want_ids=False)
        for name in FEATURE_FILES:
            gi.save_pfm(f"{a.features}_{name}.pfm", fb[name])
        feat = (feat if S else "") + f"; features {nf} spp {rt.last_features_ms():.2f} ms -> {a.features}_*.pfm"
    if a.denoise:
        nf = feature_samples(a, rt.max_samples)
        if S:
            den = rt.upsample(rt.denoise(low, fl, **denoise_kwargs(a)), fl, fb, S)
        else:
            fb = fb if a.features else rt.run_features(a.width, a.height, nf, f64=False, want_ids=False)
            den = rt.denoise(lin, fb["features"], **denoise_kwargs(a))
        gi.save_ppm(a.denoise, den)
        if a.denoise_pfm:
            gi.save_pfm(a.denoise_pfm, den)
        feat += f"; denoised ({nf} spp features) {rt.last_denoise_ms():.2f} ms -> {a.denoise}"
    if a.occlusion:
        ao = rt.run_occlusion(a.width, a.height, f64=False, **occlusion_kwargs(a))
        gi.save_pfm(f"{a.occlusion}.open.pfm", ao["open"])
        gi.save_pfm(f"{a.occlusion}.bent.pfm", ao["bent"])
        feat += f"; occlusion {rt.last_occlusion_ms():.2f} ms -> {a.occlusion}.open.pfm, {a.occlusion}.bent.pfm"
    if a.baked:
        feat += render_baked(a, rt, scene)
    n = int(spp.sum())
    print(f"{a.scene}: {a.width}x{a.height}, {n} samples (mean {n / spp.size:.1f} spp), {stored} photons stored; "
          f"photon pass {t1 - t0:.2f} s, frame {t2 - t1:.2f} s ({n / max(t2 - t1, 1e-9) / 1e6:.1f} Msamples/s incl. host copies) -> {a.output}{lens_note}{feat}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
