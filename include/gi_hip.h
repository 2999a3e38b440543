/* include/gi_hip.h -- C ABI of the MI355X (gfx950) render hot path of GI_Raytracer.
 *
 * This is the drop-in boundary (DESIGN.md "Boundary").  The reference has no FFI of its own: its
 * de-facto interface is the public C++ surface of include/raytracer.h, include/octree.h, include/photonMap.h and
 * include/entities.h.  The C++ headers under include/gi/ keep those spellings and are thin callers of the entry points
 * below; a maintainer of the reference swaps the bodies of the cited functions for these calls.
 *
 * Conventions: every entry returns 0 on success and a negative GI_E_* code on failure; gi_last_error() gives the text;
 * nothing throws, nothing prints.  All array arguments are caller-owned, read-only, plain host pointers and are copied
 * to the device by the call that receives them.  One context is used from one thread at a time (the reference calls
 * RayTracer::run from one worker thread, include/viewer.h:52-56).  There is NO CPU fallback: without a usable HIP
 * device gi_create fails with GI_E_NO_DEVICE.
 */
#ifndef GI_HIP_H
#define GI_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define GI_OK 0
#define GI_E_NO_DEVICE (-1)
#define GI_E_INVALID (-2)
#define GI_E_HIP (-3)
#define GI_E_STATE (-4)
#define GI_E_CANCELLED (-5)

typedef struct gi_ctx gi_ctx;

/* Flattened scene = what Octree holds after push_back()/rebuild() (include/octree.h:39-64, include/octree.cpp:25-119). */
typedef struct gi_scene_desc {
    int32_t n_tri;           /* number of entities (triangles, and spheres when ent_kind is given)                          */
    const double* tri_pos;   /* [n_tri][3][3] vertex positions          (triangle::vertices[k].pos, include/entities.h:331) */
    const double* tri_nrm;   /* [n_tri][3][3] vertex normals (all-zero row = flat shading, include/entities.h:478)          */
    const double* tri_uv;    /* [n_tri][3][2] texture coordinates                                                           */
    const int32_t* tri_mat;  /* [n_tri] index into mats                                                                     */
    int32_t n_mat;
    const double* mats;      /* [n_mat][9] roughness, opacity, IOR, diffuse rgb, emissive rgb (include/material.h:84-100)   */
    int32_t n_light;
    const double* lights;    /* [n_light][11] pos, col, rad, dir, angle (include/light.h:10-58; dir/angle from Octree::rebuild) */
    double ambient[3];       /* RayTracer::ambient (include/raytracer.h:726)                                                */
    /* linearised Octree: nodes in pre-order, children 0..7 as in Octree::Node::partition (include/octree.cpp:321-328)      */
    int32_t n_node;
    const double* node_bbox;     /* [n_node][6] min xyz, max xyz                                                            */
    const int32_t* node_child;   /* [n_node][8] node index or -1 (null child)                                               */
    const int32_t* node_ent_off; /* [n_node+1] range of node_ent_idx owned by the node (leaves only)                        */
    const int32_t* node_ent_idx; /* [node_ent_off[n_node]] triangle indices in Node::_entities order                        */
    /* entity kinds (include/entities.h): NULL = all triangles; else [n_tri] with 0 = triangle, 1 = analytic sphere
     * (include/entities.h:51-142) whose centre is tri_pos[i][0] and radius tri_pos[i][1].x (normals / uvs unused)          */
    const int32_t* ent_kind;
    /* atmosphere entities (Octree::at, include/octree.h:43): HeightFog (include/atmosphere.h:30-83).  fog [n_fog][12] = pos, size,
     * colour, density, scatter, noise scale; the noise grid of entity i is fog_grid[fog_grid_off[i] .. fog_grid_off[i+1])         */
    int32_t n_fog;
    const double* fog;
    const int32_t* fog_grid_off;
    const double* fog_grid;
    /* textures (include/material.h:10-81).  n_tex = 0: every material is the constant colour pair held in mats[] (colorTex).
     * Else mat_tex [n_mat][2] = diffuse and emissive texture of each material, and texture t is
     *   tex_kind[t] = 0  texture(col):            tex_param[t] = col rgb
     *   tex_kind[t] = 1  checkerboard(t, a, b):   tex_param[t] = a rgb, b rgb, tiles
     *   tex_kind[t] = 2  imageTexture(file, tile): tex_param[t] = tile u, tile v, width, height, has alpha channel (0/1), offset of
     *                    its first pixel in tex_pixels (pixels: RGBA8, rows top to bottom as QImage addresses them)           */
    int32_t n_tex;
    const int32_t* tex_kind;
    const double* tex_param;     /* [n_tex][8] */
    const int32_t* mat_tex;      /* [n_mat][2] */
    const uint8_t* tex_pixels;
    int64_t n_tex_pixel_bytes;
} gi_scene_desc;

/* Photon set + linearised PhotonMap (include/photonMap.h:13-49, include/photon.h:5-15). */
typedef struct gi_photon_map_desc {
    int32_t n_photon;
    const double* photons;       /* [n_photon][9] origin, dir, col                                                          */
    int32_t n_node;              /* 0 = no map (gather returns 0, as an empty PhotonMap does)                                */
    const double* node_bbox;     /* [n_node][6]                                                                             */
    const int32_t* node_child;   /* [n_node][8] node index, or -1 in every slot for a leaf (PhotonMap::Node::is_leaf)       */
    const int32_t* node_off;     /* [n_node+1] range of node_idx                                                            */
    const int32_t* node_idx;     /* photon indices in Node::_entities order                                                 */
} gi_photon_map_desc;

/* Camera (include/camera.h:7-31) + frame + sampling budget (include/raytracer.h:721-726). */
typedef struct gi_render_params {
    double cam_pos[3], cam_up[3], cam_forward[3];
    double sensor_diag, focal_dist;
    int32_t width, height;
    /* Row sharding for multi-GPU runs: the frame is cut into stripes of stripe_h rows; this context renders stripes
     * k with k % stripe_world == stripe_rank.  Single GPU: stripe_h = height, rank 0, world 1.                            */
    int32_t stripe_h, stripe_rank, stripe_world;
    int32_t min_samples, max_samples;
    double noise_thresh;
    uint64_t seed;           /* counter-RNG seed (replaces the reference's time-seeded drand(), DESIGN.md "RNG contract")  */
} gi_render_params;

int gi_create(gi_ctx** out, int device_ordinal);
void gi_destroy(gi_ctx*);
const char* gi_last_error(const gi_ctx*);
/* Launch kernels of this context on a caller-owned HIP stream (hipStream_t passed as void*; NULL = default stream). */
int gi_set_stream(gi_ctx*, void* hip_stream);

/* replaces: the scene half of RayTracer::setScene + the tree walk of Octree::intersect/intersectSorted (include/raytracer.h:35-39,
 * include/octree.cpp:150-211,256-313) -- uploads the tables every kernel reads.  It does NOT drop the photon map (ABI change of round 2,
 * INTEGRATION.md "ABI notes"): a caller that uploads a DIFFERENT scene calls gi_clear_photons as well -- RayTracer::setScene is the pair --
 * or the gather keeps answering from the previous scene's photons.                                                       */
int gi_upload_scene(gi_ctx*, const gi_scene_desc*);
/* replaces: PhotonMap::push_back/rebuild as the source of the gather (include/photonMap.cpp:24-47).  The map outlives gi_upload_scene
 * (the reference keeps a valid map when an edited scene is rebuilt, include/raytracer.h:56-72); gi_clear_photons drops it -- RayTracer::setScene,
 * which allocates a fresh PhotonMap (include/raytracer.h:38), is gi_upload_scene + gi_clear_photons.                                    */
int gi_upload_photons(gi_ctx*, const gi_photon_map_desc*);
int gi_clear_photons(gi_ctx*);

/* replaces: the pixel loop of RayTracer::run (include/raytracer.h:93-160) with radiance/trace/visible/secondaryRay/
 * samplePhotons inside (include/raytracer.h:167-579).
 * Number of rows this context renders for the given sharding: gi_local_rows().
 * d_out_lin: DEVICE pointer to [local_rows][width][3] linear (pre-gamma, unclamped) radiance, float (out_is_f64 = 0) or
 * double (1).  d_out_spp: optional DEVICE pointer to [local_rows][width] int32 samples taken (adaptive loop).
 * cancel: optional host flag polled between launches (RayTracer::stop, include/raytracer.h:98,718).                        */
int gi_local_rows(const gi_render_params*);
int gi_render_device(gi_ctx*, const gi_render_params*, void* d_out_lin, int out_is_f64, int32_t* d_out_spp, volatile const int* cancel);
/* Same, result copied to HOST memory (what a Qt-side caller wants). */
int gi_render_host(gi_ctx*, const gi_render_params*, void* h_out_lin, int out_is_f64, int32_t* h_out_spp, volatile const int* cancel);
/* Schedules of the same per-path arithmetic: 0 = wavefront pipeline (default: trace / shade / gather kernels over compacted
 * path queues in HBM; fixed-spp frames refill finished slots with new samples, adaptive frames run in synchronous rounds),
 * 1 = megakernel (one lane keeps one pixel, whole path in registers), 2 = synchronous rounds on the streaming passes, fixed
 * and adaptive frames alike (a second schedule of the fixed-spp frames).                                                     */
int gi_set_render_mode(gi_ctx*, int mode);
/* Octree walk: 1 (default) = wide records, the boxes of a node's children tested together from the five planes per axis that
 * Octree::Node::partition builds them from (include/octree.cpp:318-328); 0 = one box test per node record.  Same box
 * arithmetic (include/bbox.h:47-73), same visiting order, same results; a tree whose children are not those exact octants
 * always takes the per-node walk.  The photon octree has the same option (PhotonMap::Node::partition builds its children from
 * the same planes, include/photonMap.cpp:139-149): the descent of getBounds reads one record per level instead of two.
 * Exists so that the two can be compared.  Returns a bit set, negative on error: 1 = the wide walk is in use after the call
 * (a scene is uploaded and its tree qualifies), 2 = the uploaded photon octree is walked one record per level.               */
int gi_set_wide_nodes(gi_ctx*, int enable);
/* Content-box culling: 1 (default) = a child of the wide walk whose octant the ray enters is skipped when the ray misses the box of everything
 * referenced in that child's sub-tree (no entity there can report a hit, so the walk's results are the same by construction); 0 = every such
 * child is visited, as Octree::Node::intersectSorted does (include/octree.cpp:285-313).  Exists so that the two can be compared (frames are
 * identical bit for bit).  Returns 1 when culling is in use after the call (a scene is uploaded, its tree takes the wide walk), else 0.      */
int gi_set_content_culling(gi_ctx*, int enable);
/* Entity boxes: 1 (default) = the wide walk runs Entity::intersect only on the references of a leaf whose own (widened) box the ray touches; 0 = on
 * every reference, as RayTracer::trace / visible do (include/raytracer.h:290-305,446-472).  A ray that misses an entity's box cannot hit the entity:
 * same hits, same order, same frame bit for bit; exists so that the two can be compared.  Returns 1 when in use after the call.
 * The closest-hit walk's further cuts hang on the same switch (0 = off, the walks ask exactly what the reference asks): boxes cut to the part of an
 * opaque entity inside its leaf, content boxes made of those, no look behind the best hit -- and with them the re-walk of a ray that met two
 * entities at exactly the same distance, and the plain walk of rays along an axis plane (gi_walk.h: trace_wide_step).       */
int gi_set_entity_boxes(gi_ctx*, int enable);
/* Upper bound on paths in flight in the wavefront pipeline (232 B each, as field arrays).  Default: as many as 90 % of the free HBM holds
 * next to their queues, up to the whole frame (1080p x 256 spp = 531 M paths = 123 GB).                                                           */
int gi_set_pool_slots(gi_ctx*, int64_t slots);
/* Device time in ms of the render kernel(s) of the last gi_render_* call, measured with hipEvents on the launch stream. */
int gi_last_render_ms(gi_ctx*, float* ms, int32_t* n_launches);
/* Device time per pipeline stage of the last render, summed over its launches (HIP events around every launch):
 * [0] regenerate, [1] trace, [2] shade, [3] sorts (+ key kernels), [4] gather, [5] finish, [6] accumulate, [7] other.      */
int gi_last_stage_ms(gi_ctx*, float* out8);
/* The same per kernel family, out10: [0..7] as above except [2] = k_st_shade alone, [8] = k_st_shadow (the shadow walks the shade stage put off),
 * [9] reserved (0).                                                                                                         */
int gi_last_kernel_ms(gi_ctx*, float* out10);
/* Work counters of the last render.  gi_set_counters(ctx, 1): the REFERENCE's visits -- the frame is rendered by the megakernel with the
 * per-node walk and nothing culled, and gi_get_counters gives node visits in trace (BoundingBox::intersect calls of Octree::Node::intersectSorted,
 * include/octree.cpp:285-313), node visits in visible, triangle tests, shaded hits, photon candidates, trace calls, shadow rays, gathers.
 * gi_set_counters(ctx, 2): what the streaming kernels EXECUTE -- the frame is rendered by the pipeline that is benchmarked, its walks count per
 * lane, and gi_get_stream_counters gives out17 = k_st_trace: [0] walks begun (root box tests), [1] wide records visited, [2] child boxes tested
 * from them, [3] content boxes tested, [4] non-empty leaves met, [5] entity tests, [6] rays handed to the kernel; k_st_shadow: [7..12] the same
 * six, [13] shadow segments; [14] gather queries, [15] photon candidates they scanned, [16] shaded hits; [17] / [18] references sorted by their
 * entity box in k_st_trace / k_st_shadow (out must hold 19 values).  With content-box culling and entity boxes off, [5] is the reference's count of
 * entity tests in trace() exactly, and [0] the number of its trace() calls.  Covers fixed-sample-count frames of triangle scenes
 * without spheres, fog or textures (the BASELINE scenes); other scenes get GI_E_STATE.  0 = off (default).                                  */
int gi_set_counters(gi_ctx*, int mode);
int gi_get_counters(gi_ctx*, int64_t* out8);
int gi_get_stream_counters(gi_ctx*, int64_t* out19);

/* First-hit feature buffers -- an ADDITION: the reference renders radiance only.  Per sample s = 0 .. n_samples-1 of a pixel the values are what
 * RayTracer::radiance holds right after trace() of the primary ray (include/raytracer.h:112-129 the ray, 186-210 the hit): albedo =
 * current->material.diffuse->get(minUV) (include/raytracer.h:200), normal = minNorm as trace returns it (not flipped, not renormalised), depth =
 * glm::length(minHit - ray.origin) (include/raytracer.h:210), coverage = 1; all 0 on a miss.  The ray and the RNG keys of the alpha test are the
 * beauty pass's (params->seed, stream = Halton index of the sample, depth 0), so the first hits are the ones gi_render_* shades.  Per pixel: the
 * f64 sum over s in ascending order, divided once by n_samples.  Fog is ignored, specular chains are not followed (glass and mirrors report their
 * stored diffuse colour).  n_samples is the caller's and independent of min_samples / max_samples; it must be >= 1 and keep the Halton index
 * within 32 bits, as the beauty pass does (GI_E_INVALID otherwise).  Stripes as for the frame (gi_local_rows).
 * out [local_rows][width][8] = albedo rgb, normal xyz, depth, coverage, float (out_is_f64 = 0) or double (1);
 * ids (optional) [local_rows][width][2] = entity index, material index of sample 0's hit, -1 -1 on a miss.
 * gi_render_features_device: DEVICE pointers, asynchronous on the context's stream; gi_render_features_host: HOST pointers.
 * gi_last_features_ms: device time of the last feature pass (HIP events around it); gi_last_render_ms / gi_last_kernel_ms keep the last frame's. */
int gi_render_features_device(gi_ctx*, const gi_render_params*, int32_t n_samples, void* d_out, int out_is_f64, int32_t* d_ids);
int gi_render_features_host(gi_ctx*, const gi_render_params*, int32_t n_samples, void* h_out, int out_is_f64, int32_t* h_ids);
int gi_last_features_ms(gi_ctx*, float* ms);

/* Denoiser -- an ADDITION: the reference has none, so nothing of it is replaced.  A feature-guided, edge-avoiding a-trous wavelet filter
 * (Dammertz et al. 2010) over a whole frame, guided by the buffers of gi_render_features_*.  No scene is needed: the entries work on any context.
 * color [height][width][3] linear radiance as gi_render_* writes it; features [height][width][8] = albedo rgb, normal xyz, depth, coverage;
 * out [height][width][3].  Each of the three is float (flag 0) or double (1): floats are widened on load, the result is rounded once on store.
 * All arithmetic is f64 with IEEE operations only (+ - * /, compares, selects; no exp / pow / sqrt) in the order written here, so the result
 * can be restated exactly (the tests' numpy statement is bit-equal); the edge-stopping function is therefore Tukey's biweight, not a Gaussian.
 *   1. iterations = 0: out = color (converted), nothing else runs.
 *   2. m = demodulate ? (albedo > 1e-3 ? albedo : 1e-3) : 1 per channel;  c = color / m.
 *   3. for level i = 0 .. iterations-1, step = 1 << i, h = [1/16, 1/4, 3/8, 1/4, 1/16]: for pixel p the taps q = p + step (dx, dy), dy = -2 .. 2
 *      outer, dx = -2 .. 2 inner; taps outside the frame are skipped.  With |v|^2 = (x^2 + y^2) + z^2:
 *        dc = |c_p - c_q|^2 / (|c_p|^2 + (|c_q|^2 + 1e-12))          dn = |n_p - n_q|^2
 *        da = |a_p - a_q|^2 + (cov_p - cov_q)^2                        dz = r^2, r = (z_p - z_q) / (z_p + z_q) if z_p + z_q > 0, else 0
 *        d  = ((dc inv_c + dn inv_n) + dz inv_z) + da inv_a,  inv_c = 4^i / sigma_color^2 (the colour sigma halves per level), the others
 *             1 / sigma^2, computed once on the host in double; a sigma of 0 switches its term off (inv = 0)
 *        t  = 1 - min(d, 1) (a NaN d counts as 1);   w = (h[dy] h[dx]) (t t);   num += w c_q per channel, den += w, in tap order
 *      c'_p = num / den.  The centre tap has d = 0 and weight 9/64, so den > 0.
 *   4. out = c m.
 *   5. A tap whose (demodulated) colour has a non-finite channel is skipped; a centre pixel with a non-finite channel uses dc = 0 for all
 *      its taps; if every tap was skipped the pixel becomes 0 0 0.  The output of a level is always finite (finite features given).
 * Whole frames only: the filter reads neighbours across rows, so callers that render in stripes denoise the gathered frame.
 * GI_E_INVALID: width or height < 1, iterations outside 0 .. 8, a negative or NaN sigma, a null pointer; the output is not touched.
 * gi_denoise_default_params: 5 iterations, demodulate 1, sigmas 1.0, 0.5, 0.1, 0.25 (width and height 0: the caller sets them).  A colour sigma of
 * 2.0 smooths an untextured frame a little more but blurs the lighting of a frame that has little noise to begin with.
 * gi_denoise_device: DEVICE pointers, asynchronous on the context's stream; out may be the same pointer as color.  The context owns the scratch
 * (two f64 colour buffers and one f64 guide record per pixel: 112 bytes per pixel), sized on first use and kept.
 * gi_denoise_host: HOST pointers.  gi_last_denoise_ms: device time of the last pass (HIP events around it); the frame's and the feature
 * pass's times are left alone. */
typedef struct gi_denoise_params {
    int32_t width, height;
    int32_t iterations;      /* 0 .. 8 levels */
    int32_t demodulate;      /* 1: filter colour / albedo and multiply back (keeps texture detail) */
    double sigma_color, sigma_normal, sigma_depth, sigma_albedo;
} gi_denoise_params;
void gi_denoise_default_params(gi_denoise_params*);
int gi_denoise_device(gi_ctx*, const gi_denoise_params*, const void* d_color, int color_is_f64, const void* d_features, int features_is_f64, void* d_out, int out_is_f64);
int gi_denoise_host(gi_ctx*, const gi_denoise_params*, const void* h_color, int color_is_f64, const void* h_features, int features_is_f64, void* h_out, int out_is_f64);
int gi_last_denoise_ms(gi_ctx*, float* ms);

/* Guided upsampling -- an ADDITION: a full-size frame from a reduced-size render.  A joint-bilateral upsampler (Kopf et al. 2007) guided by the
 * buffers of gi_render_features_* at both sizes: the colour is interpolated between low pixels where the full-size normal and depth agree with
 * theirs, and the full-size albedo multiplied back in restores the texture detail that was never rendered.  gi_layout.h derives the sensor from
 * the aspect ratio alone, so a (width / factor) x (height / factor) frame with factor | width and factor | height sees the view of the
 * width x height frame, and low pixel (X, Y) covers the full pixels [factor X, factor X + factor) x [factor Y, factor Y + factor).  No scene is needed.
 * low_color [low_height][low_width][3] linear radiance; low_features [low_height][low_width][8] and features [height][width][8] = albedo rgb,
 * normal xyz, depth, coverage; out [height][width][3].  Each of the four is float (flag 0) or double (1): floats are widened on load, the result
 * is rounded once on store.  All arithmetic is f64 with IEEE operations only, in the order written here (the tests' numpy statement,
 * tests/upsample_expect.py, is bit-equal).  With S = factor, wl = low_width, hl = low_height, |v|^2 = (x^2 + y^2) + z^2, and the modulation m of
 * the denoiser (demodulate ? (albedo > 1e-3 ? albedo : 1e-3) : 1 per channel), ml of the low features and mf of the full ones:
 *   1. c = low_color / ml.
 *   2. for full pixel (x, y), in integers: Nx = 2 x + 1 - S, X0 = floor(Nx / 2S) (floor division: Nx may be negative); Ny, Y0 likewise.  2S X - Nx is
 *      twice the distance, in full pixels, between the centre of low pixel X and the centre of x.
 *   3. the 16 taps (X, Y): Y = Y0-1 .. Y0+2 outer, X = X0-1 .. X0+2 inner; taps outside the low frame are skipped.
 *   4. the spatial weight is a tent of radius two low pixels: nx = |2S X - Nx|, tx = (double)(4S - nx) / (double)(4S) if nx < 4S, else 0; ty likewise.
 *   5. between the full pixel's guide p = features[y][x] and the tap's guide q = low_features[Y][X], the denoiser's terms
 *        dn = |n_p - n_q|^2      da = |a_p - a_q|^2 + (cov_p - cov_q)^2      dz = r^2, r = (z_p - z_q) / (z_p + z_q) if z_p + z_q > 0, else 0
 *        d  = (dn inv_n + dz inv_z) + da inv_a, inv = 1 / sigma^2 computed once on the host in double; a sigma of 0 switches its term off (inv = 0)
 *        e  = 1 - min(d, 1) (a NaN d counts as 1).  There is no colour term: the full-size colour is what is being made.
 *   6. w = (ty tx) (e e); a tap whose c has a non-finite channel is skipped; num += w c per channel, den += w, in tap order.
 *   7. den > 0: out = (num / den) mf.  Otherwise the nearest low pixel (min(x / S, wl - 1), min(y / S, hl - 1)): out = c mf, or 0 0 0 if that
 *      pixel has a non-finite channel.  The output is finite for finite features.
 * GI_E_INVALID: width or height < 1, factor outside 2 .. 8, low_width != ceil(width / factor) or low_height != ceil(height / factor), a negative or
 * NaN sigma, a null pointer; the output is not touched.
 * gi_upsample_default_params: demodulate 1, sigmas 0.5, 0.1, 0.0 (sizes and factor 0: the caller sets them).  The albedo term is off by default: a
 * low-size albedo is the mean of an S x S block of texture, and comparing it with the full-size albedo would reject every tap on a textured surface.
 * gi_upsample_device: DEVICE pointers, asynchronous on the context's stream; out must not overlap an input.  The low frame is widened and
 * demodulated into the denoiser's scratch (the context's, sized on first use and kept).  gi_upsample_host: HOST pointers.
 * gi_last_upsample_ms: device time of the last pass (HIP events around it); the frame's, the feature pass's and the denoiser's times are left
 * alone, and so is a progressive session. */
typedef struct gi_upsample_params {
    int32_t width, height;            /* of the output and of features */
    int32_t low_width, low_height;    /* of low_color and low_features: ceil(width / factor), ceil(height / factor) */
    int32_t factor;                   /* 2 .. 8 */
    int32_t demodulate;               /* 1: interpolate colour / albedo and multiply by the full-size albedo */
    double sigma_normal, sigma_depth, sigma_albedo;
} gi_upsample_params;
void gi_upsample_default_params(gi_upsample_params*);
int gi_upsample_device(gi_ctx*, const gi_upsample_params*, const void* d_low_color, int low_color_is_f64, const void* d_low_features, int low_features_is_f64,
                       const void* d_features, int features_is_f64, void* d_out, int out_is_f64);
int gi_upsample_host(gi_ctx*, const gi_upsample_params*, const void* h_low_color, int low_color_is_f64, const void* h_low_features, int low_features_is_f64,
                     const void* h_features, int features_is_f64, void* h_out, int out_is_f64);
int gi_last_upsample_ms(gi_ctx*, float* ms);

/* Ambient occlusion and bent normals -- an ADDITION: the reference renders radiance only.  A buffer beside the first-hit features: how much of the
 * hemisphere above the first surface is free of geometry within `radius`, and the mean free direction.  Per pixel and per sample
 * s = 0 .. n_samples-1:
 *   1. the primary ray and its first hit are those of gi_render_features_* and of the beauty pass: Halton index idx of sample s, RNG stream
 *      (params->seed, idx), depth 0, the alpha test of RayTracer::trace (include/raytracer.h:382-478).
 *   2. a miss: the sample's openness is 1, its bent vector 0 0 0.
 *   3. a hit at P with shading normal N (minNorm of trace, include/raytracer.h:461): n = N * (1 / sqrt(dot(N, N))), Nf = -n if dot(n, ray.dir) > 0
 *      else n (the side the ray came from), O = P + 0.0001 Nf (SHADOW_BIAS, the offset of the reference's shadow rays, include/raytracer.h:241).
 *   4. for j = 0 .. n_dirs-1: u = (float) draw(purpose 32, a = j), v = (float) draw(purpose 33, a = j) of that stream (DESIGN.md "RNG contract";
 *      gi_kat 8), d_j = hemisphereSample_cos(Nf, u, v, 1) (include/util.cpp:35-58), T_j = O + radius d_j.
 *   5. segment j is open when RayTracer::visible (include/raytracer.h:280-319) finds no occluder between O and T_j: the ray (O, d_j), maxt = the
 *      squared length of T_j - O as gi_visible forms it (x x + y y + z z), so gi_visible on the rows (O, T_j) states it.  The alpha test of a
 *      translucent occluder draws with the light index 65536 + j, which no light has.  The medium is not asked: fog does not occlude.
 *   6. open_s = (open segments) / n_dirs;  bent_s = (sum of d_j over the open j, ascending) / n_dirs per component.
 * Per pixel: the f64 sums of open_s and bent_s over s in ascending order, divided once by n_samples.  bent is not renormalised: its length is a
 * cosine-weighted openness, its direction the mean free direction.  The result does not depend on stripes, the octree walk in use or the launch.
 * out [local_rows][width][4] = openness, bent x y z, float (out_is_f64 = 0) or double (1), rounded once on store.  Stripes as for the frame.
 * radius = 0 stands for a tenth of the diagonal of the scene's root box: 0.1 sqrt((dx dx + dy dy) + dz dz).
 * GI_E_INVALID: n_samples < 1 or taking the Halton index beyond 32 bits (as the feature pass), n_dirs outside 1 .. 64, a negative, NaN or infinite
 * radius, a null pointer; GI_E_STATE: no scene.  The output is not touched then.
 * gi_occlusion_default_params: 16 samples, 16 directions, radius 0.
 * gi_render_occlusion_device: DEVICE pointer, asynchronous on the context's stream; gi_render_occlusion_host: HOST pointer.
 * gi_last_occlusion_ms: device time of the last pass (HIP events around it); the frame's, the feature pass's, the denoiser's and the upsampler's
 * times are left alone, and so is a progressive session. */
typedef struct gi_occlusion_params {
    int32_t n_samples;       /* >= 1 */
    int32_t n_dirs;          /* 1 .. 64 segments per sample */
    double radius;           /* length of a segment; 0 = a tenth of the scene box's diagonal */
} gi_occlusion_params;
void gi_occlusion_default_params(gi_occlusion_params*);
int gi_render_occlusion_device(gi_ctx*, const gi_render_params*, const gi_occlusion_params*, void* d_out, int out_is_f64);
int gi_render_occlusion_host(gi_ctx*, const gi_render_params*, const gi_occlusion_params*, void* h_out, int out_is_f64);
int gi_last_occlusion_ms(gi_ctx*, float* ms);

/* Function-level entry points (parity tests and the C++ API's public methods).  Host pointers.
 * replaces RayTracer::trace (include/raytracer.h:382-478): rays [n][6] origin + unit dir -> hit, entity, res [n][8]        */
int gi_trace(gi_ctx*, int32_t n, const double* rays, int32_t* hit, int32_t* ent, double* res);
/* replaces RayTracer::visible (include/raytracer.h:280-319): q [n][6] = shadow-ray origin, target point                    */
int gi_visible(gi_ctx*, int32_t n, const double* q, int32_t* vis);
/* the same with the reference's own arguments: rays [n][6] = shadow-ray origin + unit direction, mt [n] = squared distance to the light point */
int gi_visible_rays(gi_ctx*, int32_t n, const double* rays, const double* mt, int32_t* vis);
/* replaces RayTracer::samplePhotons(pos, dir, 32) (include/raytracer.h:532-579): q [n][6] = pos, dir                       */
int gi_gather(gi_ctx*, int32_t n, const double* q, double* res3, int32_t* n_cand);
/* replaces RayTracer::radiance(ray, 0, ...) (include/raytracer.h:167-276): rays [n][6], stream [n] = Halton sample index  */
int gi_radiance(gi_ctx*, int32_t n, const double* rays, const uint32_t* stream, uint64_t seed, double* out3);
/* replaces RayTracer::tracePhotons (include/raytracer.h:582-715): emits `count` photon indices per light on the device;
 * photons_out [cap][9]; returns the number stored (<= count * n_light) or a negative error; tries_out = emission tries.    */
int gi_emit_photons(gi_ctx*, int32_t count, int32_t max_depth, uint64_t seed, double* photons_out, int32_t cap, int64_t* tries_out);

/* Halton_sampler::sample / Halton_enum::get_index on the device tables (include/halton_sampler.h:626-888,
 * include/halton_enum.h:106-114) -- known-answer access for tests                                                          */
int gi_halton_sample(gi_ctx*, int32_t n, const uint32_t* dim, const uint32_t* index, float* out);
int gi_halton_index(gi_ctx*, int32_t width, int32_t height, int32_t n, const uint32_t* sxy /*[n][3]*/, uint32_t* out);

/* The photon map built on the device.  replaces: PhotonMap::push_back x n + PhotonMap::rebuild / PhotonMap::Node::partition
 * (include/photonMap.cpp:24-47,137-192) and the upload, for photons handed in (gi_build_photon_map: photons [n][9] on the host) or emitted
 * by the device itself (gi_trace_photons = RayTracer::tracePhotons(max_depth, count) + rebuild, include/raytracer.h:61-72,582-715: the
 * photons never leave the device; returns the number stored, tries_out = emission tries).  box6 = the box of the map (PhotonMap(min, max));
 * NULL = the root box of the uploaded scene (RayTracer::setScene, include/raytracer.h:38).  The tables are, byte for byte, the ones
 * gi_upload_photons derives from the host builder's tree.  gi_debug_photon_tables copies the installed tables back (NULL pointers: sizes only):
 * nodes128 [n_node][128 bytes], ranges2 [n_range][2], pos3 [n_photon][3], dircol6 [n_photon][6].                                      */
int gi_build_photon_map(gi_ctx*, int32_t n, const double* photons, const double* box6);
int gi_trace_photons(gi_ctx*, int32_t count, int32_t max_depth, uint64_t seed, const double* box6, int64_t* tries_out);
int gi_debug_photon_tables(gi_ctx*, int32_t* n_node, int32_t* n_range, int32_t* n_photon, void* nodes128, int32_t* ranges2, double* pos3, double* dircol6);

/* Several GPUs from one process.  Replaces the OpenMP row loop of RayTracer::run (include/raytracer.h:93: `#pragma omp parallel for
 * schedule(dynamic, 10)` over image rows) for a caller that is one process -- the Qt application: a group holds one context per device, the
 * scene and photon tables are replicated, the frame's stripes of stripe_h rows are dealt round-robin to the devices, each rendered on its own
 * host thread, and gathered into one frame.
 * gi_group_create: n_devices = 0 takes every visible device; device_ordinals may repeat an ordinal (several contexts on one device: how the
 * one-GPU tests exercise this path).  gi_group_ctx gives a member context, e.g. for gi_emit_photons on device 0.
 * gi_group_render_host: stripes [first_stripe, first_stripe + n_stripes) of the frame, stripe s on device (s - first_stripe) % n; every device
 * copies its rows into the caller's whole-frame host buffer h_frame [height][width][3] (float or double) and h_spp [height][width] (optional);
 * other rows are not touched -- RayTracer::run's progressive display calls this with a window of n stripes per step.
 * gi_group_render_device: the whole frame, gathered into d_frame_on_device0 (DEVICE pointer on the first context's device) with peer copies
 * over xGMI.  Both return after every device has finished; errors name the device (gi_group_last_error).                              */
typedef struct gi_group gi_group;
int gi_device_count(void);   /* usable HIP devices (0 without a GPU or a driver) */
int gi_group_create(gi_group** out, int32_t n_devices, const int32_t* device_ordinals);
void gi_group_destroy(gi_group*);
int gi_group_size(const gi_group*);
gi_ctx* gi_group_ctx(gi_group*, int32_t i);
const char* gi_group_last_error(const gi_group*);
int gi_group_upload_scene(gi_group*, const gi_scene_desc*);
int gi_group_upload_photons(gi_group*, const gi_photon_map_desc*);
int gi_group_clear_photons(gi_group*);
int gi_group_render_host(gi_group*, const gi_render_params*, int32_t stripe_h, int32_t first_stripe, int32_t n_stripes, void* h_frame, int out_is_f64, int32_t* h_spp, volatile const int* cancel);
int gi_group_render_device(gi_group*, const gi_render_params*, int32_t stripe_h, void* d_frame_on_device0, int out_is_f64, volatile const int* cancel);

/* Diagnostics for parity tests (not needed to render).
 * gi_debug_leaf_order: what Octree::intersectSorted(ray, 0, inf) returns (include/octree.cpp:188-211,285-313) as the device walk produces
 * it: for ray i, the non-empty leaves in visiting order as pre-order node indices in leaf_out[i*cap ..], their number in n_out[i]
 * (may exceed cap; only cap are stored).  Uses the walk the kernels use (wide records or per-node links, gi_set_wide_nodes).
 * gi_kat: known answers of the scalar building blocks as the device computes them.  what: 0 fastPow(a,b), 1 fastPrecisePow(a,b)
 * (include/util.h:100-136), 2 hemisphereSample_cos(n,u,v,power), 3 sample_phong(outdir,power,sx,sy), 4 sphereCapSample_cos(n,u,v,power,frac)
 * (include/util.cpp:35-107), 5 randomUnitVec(x,y), 6 refr(inc,n,eta) (include/util.h:173-188), 7 glm::reflect(inc,n); 16..22 the libm
 * calls of the path: sin, cos, acos, asin, atan2(a,b), pow(a,b), sqrt.  8 = the counter RNG that stands in for drand() (include/util.h:52-80;
 * DESIGN.md "RNG contract"): in = seed high 32 bits, seed low 32 bits, stream, depth, purpose, a, b (integers carried in doubles),
 * out = the draw, the stream key's high and low 32 bits.  in [n][in_stride] (arguments in the order given), out3 [n][3].  */
int gi_debug_leaf_order(gi_ctx*, int32_t n, const double* rays, int32_t cap, int32_t* leaf_out, int32_t* n_out);
/* gi_debug_sort_pairs: the pipeline's own radix sort (gi_sort.inc: the gather queries by photon-map leaf, the continuing rays by coherence key) on
 * caller data -- n (key, value) pairs sorted by bits [begin_bit, end_bit) of the key, stable.  Host pointers.                                */
int gi_debug_sort_pairs(gi_ctx*, int32_t n, const uint32_t* keys, const uint32_t* vals, int32_t begin_bit, int32_t end_bit, uint32_t* keys_out, uint32_t* vals_out);
/* gi_debug_find_leaves: the photon-map leaf around each position (PhotonMap::Node::getBounds, include/photonMap.cpp:115-134) as the two descents of the
 * pipeline find it: full_out the one that asks every box on the way (-1: no leaf contains the position), fast_out the one the gather keys of a pass
 * take (split records only, the first five levels through a jump table), -2 where that one declines (a position within 1e-12 of a split plane).
 * (gi_gather.h: gather_find_leaf, gather_find_leaf_fast; gather_leaf_of is the two together.) */
int gi_debug_find_leaves(gi_ctx*, int32_t n, const double* pos, int32_t* fast_out, int32_t* full_out);
/* gi_debug_gather_pass: one gather pass of the streaming pipeline on caller queries q6 [n][6] = position, direction.  Query i takes slot i of a
 * path pool (gather factor 1, radiance 0) and the sort key k_st_compact gives it; sort = 1 puts the queries in leaf order with the pipeline's
 * radix sort, sort = 0 keeps the caller's order.  kernel: 0 k_st_gather, 1 its counting instance, 2 k_st_gather_wave, 3 its counting instance,
 * launched as the pass loop launches them (GI_E_STATE: the wave kernel without written-out candidate lists, GI_FLAT_CANDIDATES=0).
 * res3 [n][3] = the caustic term of query i (RayTracer::samplePhotons(pos, dir, 32)); keys_out / order_out [n] (optional) = the keys and slots
 * in the order the kernel read them; counters2 (optional) = gather queries and candidates a counting instance counted (0 otherwise).
 * The kernels are in gi_gather.inc, the selection they share with gi_gather (k_gather) in gi_gather.h.                                  */
int gi_debug_gather_pass(gi_ctx*, int32_t n, const double* q6, int32_t kernel, int32_t sort, double* res3, uint32_t* keys_out, uint32_t* order_out, int64_t* counters2);
/* gi_debug_walk: caller rays [n][6] (origin, unit direction) through the octree walk in the forms the passes run it, with gi_trace's /
 * gi_visible_rays' keys (stream = ray index, seed 0, light 0): the same answers, ray by ray.  mt NULL: closest hit, hit_or_vis / ent / res8 as gi_trace
 * writes them; mt [n] (squared length): any hit below it, hit_or_vis = visible, ent / res8 are not touched.  form: 0 a ray per lane (the loop of the
 * trace and shadow kernels), 1 a ray per wave, 2 a ray per group of 16 lanes (the finisher's last stages: ray i = group i).  lds: 1 the wide records
 * and content boxes staged in LDS as those kernels stage them (form 0, closest hit: the closest-hit walk's boxes; else the whole entities'), 0 the
 * same tables read from global memory.  GI_E_STATE: the scene has no wide records.                                                          */
int gi_debug_walk(gi_ctx*, int32_t n, const double* rays, const double* mt, int32_t form, int32_t lds, int32_t* hit_or_vis, int32_t* ent, double* res8);
int gi_kat(gi_ctx*, int32_t what, int32_t n, const double* in, int32_t in_stride, double* out3);

/* Progressive render sessions -- an ADDITION: the reference renders a frame in one piece (its GUI repaints rows as they finish).  A session keeps
 * the per-pixel state of RayTracer::run's loop (running mean, last colour, variance, samps, s; include/raytracer.h:102-148) on the device between
 * calls, in a buffer of its own, and takes further samples when asked.  The contract: A FRAME BUILT IN STEPS HAS THE BITS OF THE FRAME gi_render_*
 * BUILDS IN ONE CALL with the same parameters, scene, photon map and render mode.  One session per context; a caller with several devices opens
 * one per context with its stripe fields (the gi_group_* entries have no progressive form).
 * gi_progressive_begin: validates the parameters as gi_render_* does, picks the schedule gi_render_device would pick (render mode 0 with
 *   min_samples == max_samples: the refill pipeline; otherwise synchronous rounds), puts every pixel in its initial state and sets the sample
 *   counter E to 0.  GI_E_STATE without a scene and in render mode 1 (the megakernel keeps a pixel in registers).  A second begin replaces the session.
 * gi_progressive_step_*: E' = min(E + n_samples, max_samples); every pixel takes samples while s < E' and the reference's rule still wants one
 *   (fixed sample count: exactly samples [E, E') of every pixel), then E = E'.  out / spp get what gi_render_* writes -- the running mean, linear and
 *   unclamped, and the samples taken, [local_rows][width] of this rank; DEVICE pointers (asynchronous on the context's stream) or HOST pointers.
 *   n_samples = 0 runs no path kernel and writes the current state (right after begin: 0.5 everywhere, spp 0, as a 0-sample frame).  GI_E_INVALID:
 *   n_samples < 0 or a null out; GI_E_STATE: no session.  A step times itself as a frame does: gi_last_render_ms / _stage_ms / _kernel_ms report it.
 *   cancel is polled where a frame polls it; a cancelled step returns GI_E_CANCELLED, keeps what it folded (E advances by the sample chunks a
 *   fixed-count step completed, not at all in rounds, where pixels may nevertheless be ahead of E) and leaves the session valid: stepping on ends
 *   on the same bits.
 * gi_progressive_status: sample_end = E; pixels_wanting = pixels of this rank that would take another sample under the session's max_samples
 *   (0: the frame is finished).  Either pointer may be null.
 * gi_upload_scene, gi_upload_photons, gi_clear_photons, gi_build_photon_map and gi_trace_photons END the session (the next step: GI_E_STATE),
 *   also when the call itself fails: they end it before they look at their arguments, so a failed upload never leaves a session on a half-set scene.
 *   Every other entry may be called between steps -- gi_render_* of any size, the feature pass, the denoiser, the upsampler, the function-level and debug
 *   entries, the result-neutral switches (wide nodes, culling, entity boxes, pool slots): the path pool, the queues and the per-sample buffer
 *   are shared scratch, only the pixel state is the session's.
 * gi_progressive_save / _restore: a checkpoint is one little-endian blob of gi_progressive_state_bytes bytes:
 *     0 char[8] magic "GIPROGR\0"   8 u32 version (1)   12 u32 header bytes (192)
 *    16 gi_render_params, its fields in declaration order: 11 f64 (cam_pos, cam_up, cam_forward, sensor_diag, focal_dist), 7 i32 (width, height,
 *       stripe_h, stripe_rank, stripe_world, min_samples, max_samples), 4 bytes 0, f64 noise_thresh, u64 seed
 *   152 i32 schedule (0 refill pipeline: records in 8x8-tile order without padding; 1 rounds: whole 8x8 tiles, padding records included)
 *   156 i32 E   160 u64 record count   168 u32 record bytes (72)   172 u32 0
 *   176 i32 entities, i32 octree nodes, i32 stored photons of the scene it was taken on (a weak fingerprint), u32 lens tag (0: pinhole; gi_set_lens)
 *   192 the records as they lie on the device: f64 colour[3], lastCol[3], var, i32 samps, s, n (scratch of a round), 0
 *   restore opens a session from a blob, on the blob's schedule.  GI_E_INVALID: bad magic, version, sizes, truncation; GI_E_STATE: no scene, or
 *   the fingerprint differs.  THE CALLER uploads the same scene and the same photons first (same photon seed and count): the fingerprint only
 *   catches a different scene, it does not prove an equal one.  restore does not look at the context's render mode (the blob's schedule holds, so
 *   a checkpoint of either schedule resumes in mode 0, 1 or 2), but like begin it returns GI_E_STATE while the megakernel's work counters are on
 *   (gi_set_counters 1).  A restore that fails leaves no session open, as a begin that fails does.
 * gi_progressive_end: closes the session and frees its records (a context's destruction does so too). */
int gi_progressive_begin(gi_ctx*, const gi_render_params*);
int gi_progressive_step_device(gi_ctx*, int32_t n_samples, void* d_out_lin, int out_is_f64, int32_t* d_out_spp, volatile const int* cancel);
int gi_progressive_step_host  (gi_ctx*, int32_t n_samples, void* h_out_lin, int out_is_f64, int32_t* h_out_spp, volatile const int* cancel);
int gi_progressive_status(gi_ctx*, int32_t* sample_end, int64_t* pixels_wanting);
int gi_progressive_state_bytes(gi_ctx*, int64_t* n_bytes);
int gi_progressive_save(gi_ctx*, void* h_blob, int64_t cap_bytes);
int gi_progressive_restore(gi_ctx*, const void* h_blob, int64_t n_bytes);
int gi_progressive_end(gi_ctx*);

/* Thin-lens camera: depth of field with a bladed aperture -- an ADDITION.  The reference's camera is a pinhole (FOCAL_BLUR == 0 at compile time,
 * include/raytracer.h:112-129); its formula for a non-zero FOCAL_BLUR moves the eye by the two Halton numbers that also place the sample in the pixel,
 * which shears the projection instead of blurring it, and is not mirrored.  Here the eye of every primary ray is drawn from an aperture in the plane
 * of `right` = normalize(cross(cam_forward, cam_up)) and cam_up -- the vectors the sensor plane is spanned by -- and the sensor plane, focal_dist in
 * front of cam_pos, is the plane that stays sharp.  The lens is state of the context, not a field of gi_render_params: every pass that makes primary
 * rays (gi_render_* in all render modes, gi_progressive_*, gi_render_features_*, gi_render_occlusion_*, gi_group_render_*) runs under it, and it
 * outlives scene and photon uploads.
 * The aperture is a regular polygon of `blades` vertices, v_k = (cos(rotation + 2 pi k / blades), sin(rotation + 2 pi k / blades)), k = 0 .. blades,
 * v_blades a copy of v_0, computed ONCE on the host with the host's libm (gi_lens_vertices; theta_k = rotation + (2 pi k) / blades in double) and
 * read by the kernels from a table: the device side is IEEE operations only (+ - * /, sqrt, compares) and can be restated bit for bit
 * (tests/lens_expect.py).  Per sample with Halton index idx, in this order, B = blades:
 *   u0 = draw(seed, stream idx, depth 0, purpose 34, a = 0),  u1 = the same with purpose 35   (f64 draws; DESIGN.md "RNG contract", gi_kat 8)
 *   k = min((int)(u0 B), B - 1),  f = u0 B - k,  r = sqrt(f)
 *   l = r ((1 - u1) v_k + u1 v_k+1)                     per component; uniform by area over the polygon
 *   eyePos = (cam_pos + (radius l.x) right) + (radius l.y) cam_up
 *   pixelPos as for the pinhole;  dir = normalize(pixelPos - eyePos)
 * radius == 0 is the pinhole: no draw is made and nothing is added to the eye, so a context that was never given a lens and one that was given
 * {0, any valid blades and rotation} produce the same bits everywhere.  The depth of gi_render_features_* stays length(hit - ray.origin), from the
 * eye on the lens.
 * gi_lens_default: radius 0, rotation 0, 6 blades.
 * gi_set_lens: radius in scene units, finite and >= 0; blades 3 .. 16; rotation finite, in radians; reserved 0 -- anything else (or a null
 *   pointer): GI_E_INVALID, and the lens stays as it was.  GI_E_STATE while a progressive session is open (its samples so far were taken under the
 *   lens it began with).  gi_get_lens returns what was set (the default on a fresh context).
 * gi_lens_vertices: host only, no device: xy [blades + 1][2]; GI_E_INVALID for a lens gi_set_lens would refuse.
 * gi_group_set_lens: the lens of every member context.
 * Checkpoints: the header word at offset 188 (reserved1 so far) is the lens tag: 0 for a pinhole -- pinhole checkpoints keep their bytes -- else
 *   the low 32 bits of 64-bit FNV-1a over the 24 bytes of gi_lens, 0 replaced by 1.  gi_progressive_restore returns GI_E_INVALID when the blob's tag is not
 *   that of the context's lens: as with scene and photons, the caller sets the lens first.
 * gi_debug_primary_rays: rays [n][6] = origin, unit direction of the samples with the given Halton indices of the frame `params`, under the
 *   context's lens -- what every pass above traces.  No scene is needed.
 * gi_focus_distance: autofocus.  The PINHOLE ray through the centre of pixel (x, y) of the frame (dx = x + .5, dy = y + .5) is traced as a primary
 *   ray is (RayTracer::trace; alpha test with seed params->seed, stream 0, depth 0); *dist = length(hit - cam_pos) dot(dir, cam_forward), the distance
 *   of the plane through the hit that is parallel to the sensor.  Returns 1 and leaves *dist alone on a miss.  GI_E_INVALID: a pixel outside the
 *   frame, bad parameters, a null pointer; GI_E_STATE: no scene.  A caller makes that plane the sharp one by scaling sensor_diag and focal_dist by
 *   dist / focal_dist: the field of view stays. */
typedef struct gi_lens { double radius; double rotation; int32_t blades; int32_t reserved; } gi_lens;
void gi_lens_default(gi_lens*);
int gi_set_lens(gi_ctx*, const gi_lens*);
int gi_get_lens(gi_ctx*, gi_lens*);
int gi_lens_vertices(const gi_lens*, double* xy /*[blades + 1][2]*/);
int gi_group_set_lens(gi_group*, const gi_lens*);
int gi_debug_primary_rays(gi_ctx*, const gi_render_params*, int32_t n, const uint32_t* idx, double* rays /*[n][6]*/);
int gi_focus_distance(gi_ctx*, const gi_render_params*, int32_t x, int32_t y, double* dist);

/* Light baking -- an ADDITION: the reference's paths all start at the camera.  A bake gathers incident light at caller-given points: light probes
 * (nine spherical-harmonic coefficients per colour channel) and lightmap texels (the diffuse indirect factor), with the renderer's own samplers and
 * the whole path tracer behind every ray -- the streaming passes gi_render_* runs, fed by a generator of their own instead of a frame.
 * A bake takes n_points points with n_samples directions each.  Sample k of point i carries the 32-bit Halton / RNG stream index
 *     stream = stream_base + i * n_samples + k
 * which plays the part a pixel sample's Halton index plays in the frame: Halton dimensions 0 and 1 at that index, as floats, are the direction's
 * (u, v) (the frame places the sample in the pixel with them, emission the point on the light); dimensions 2 + 2d and 3 + 2d and the counter RNG
 * keyed by (seed, stream) drive the path exactly as for a primary ray of that index (DESIGN.md "RNG contract").  A caller that splits a point list
 * over several calls or devices gives part [a, b) the base stream_base + a * n_samples and gets the rows [a, b) of the whole bake, bit for bit.
 *   GI_BAKE_TEXEL (lightmap texel): points [n][6] = position P, normal N.
 *     Nn = N / sqrt((Nx Nx + Ny Ny) + Nz Nz) per component;  O = P + 0.0001 Nn (SHADOW_BIAS);  d = hemisphereSample_cos(Nn, u, v, 2)
 *     (include/util.cpp:35-58), the lobe of the reference's diffuse bounce (include/raytracer.h:321-379);  the ray is Ray(O, d) (include/ray.h:7-17:
 *     d is normalised once more).  out [n][3] = the sum over k of L_k, accumulated in ascending k from +0.0, divided by (double) n_samples.
 *     This is the factor the albedo of a roughness-1 surface is multiplied by for its indirect term in RayTracer::radiance; times pi it is the
 *     irradiance, up to what fastPrecisePow does to the cosine lobe (include/util.h:113-136).
 *   GI_BAKE_SH9 (light probe): points [n][3] = position P.
 *     O = P;  d = randomUnitVec((double) u, (double) v) (include/util.h:183-188), uniform over the sphere.
 *     out [n][9][3]: acc[j][c] += L_k[c] Y_j(d_k) in ascending k from +0.0, then (acc * 12.566370614359172) / (double) n_samples.
 *     Y_j is the real SH basis of bands 0 to 2 at the unit direction (x, y, z) the path's record holds, in this order and with these literals:
 *       Y0 = 0.28209479177387814              Y1 = 0.4886025119029199 y              Y2 = 0.4886025119029199 z
 *       Y3 = 0.4886025119029199 x             Y4 = 1.0925484305920792 (x y)          Y5 = 1.0925484305920792 (y z)
 *       Y6 = 0.31539156525252005 (3.0 (z z) - 1.0)    Y7 = 1.0925484305920792 (x z)  Y8 = 0.5462742152960396 (x x - y y)
 * L_k = RayTracer::radiance(ray, depth 0) (include/raytracer.h:167-276) of that ray under the counter RNG with the call's seed -- gi_radiance on the
 * rows of gi_bake_rays states it: the first hit's emission, its direct light, its caustic gather, the rest of the path, fog on the way, the ambient
 * term on a miss.  The fold is IEEE operations only (+ * /) in the order written, compiled without contraction: given the same L_k and d_k it can be
 * restated bit for bit (tests/bake_expect.py); gi_bake_fold runs it on caller data.
 * What a bake does NOT hold: the analytic lights are not geometry, so no ray ever hits one -- direct light of the lights at the point itself is not in
 * the result.  This is the usual indirect-only bake; the consumer adds direct light itself: gi_render_baked_* does, and gi_visible answers the shadow segment for any other.  The context's
 * lens plays no part (there is no primary ray), nor does the render mode: a bake always runs the streaming passes.  Points inside geometry are
 * baked like any other.  There is no gi_group_* form: split the point list.
 * out is float (out_is_f64 = 0) or double (1), rounded once on store.  Points that do not fit the path pool (gi_set_pool_slots, free memory) run in
 * chunks, samples that do not fit in ranges of k; the sums stay f64 in ascending k, so the result does not depend on either, nor on the launch.
 * The path pool, the queues and the per-sample buffer are the shared scratch a frame uses: an open progressive session is left as it is.
 * GI_E_INVALID: a null pointer (points and out may be null when n_points is 0), a mode other than the two, n_samples < 1, n_points < 0,
 * stream_base + n_points * n_samples - 1 beyond 32 bits, and -- gi_bake_host and gi_bake_rays, which look at the points -- a position or normal that
 * is not finite, or a normal 0 0 0.  gi_bake_device does NOT look at its points: they are the caller's device memory.  GI_E_STATE: no scene.
 * n_points = 0 is GI_OK and writes nothing.  A refused call does not touch the output, and leaves the frame's and the other passes' times alone.
 * gi_bake_default_params: GI_BAKE_SH9, 256 samples, stream_base 0, seed 0x9E3779B97F4A7C15.
 * gi_bake_device: DEVICE pointers, asynchronous on the context's stream between its own read-backs; gi_bake_host: HOST pointers.
 * gi_last_bake_ms: device time of the last bake (HIP events around it); the frame's and the other passes' times are left alone.
 * Check entries (host pointers): gi_bake_rays gives the rays the generator makes, rays6_out [n_points * n_samples][6] = origin, unit direction
 * and stream_out [n_points * n_samples], sample k of point i in row i * n_samples + k; no scene is needed.  gi_bake_fold runs the fold kernel on
 * caller data: dirs3 and L3 [n_points][n_samples][3] (dirs3 may be null for GI_BAKE_TEXEL), out [n_points][3] or [n_points][9][3] double; the samples go
 * through it in ranges of 16, as those of a bake that does not fit the pool. */
#define GI_BAKE_TEXEL 0
#define GI_BAKE_SH9 1
typedef struct gi_bake_params {
    int32_t mode;            /* GI_BAKE_TEXEL or GI_BAKE_SH9 */
    int32_t n_samples;       /* >= 1 directions per point */
    uint32_t stream_base;    /* stream index of sample 0 of point 0 */
    uint64_t seed;           /* counter-RNG seed, as gi_render_params::seed */
} gi_bake_params;
void gi_bake_default_params(gi_bake_params*);
int gi_bake_device(gi_ctx*, const double* d_points, int32_t n_points, const gi_bake_params*, void* d_out, int out_is_f64);
int gi_bake_host(gi_ctx*, const double* points, int32_t n_points, const gi_bake_params*, void* h_out, int out_is_f64);
int gi_last_bake_ms(gi_ctx*, float* ms);
int gi_bake_rays(gi_ctx*, const double* points, int32_t n_points, const gi_bake_params*, double* rays6_out, uint32_t* stream_out);
int gi_bake_fold(gi_ctx*, int32_t mode, int32_t n_points, int32_t n_samples, const double* dirs3, const double* L3, double* out);

/* Lightmap atlases -- an ADDITION around the bake: the UV chart of a mesh rasterised into texels, the covered texels baked as GI_BAKE_TEXEL points,
 * the rows scattered back into an image and the gutters filled, in one device-side pass.  An atlas image comes back, not a point list.
 * A lightmap is baked for a CHART of n_chart rows.  Row j holds ent[j], an entity index that must be a triangle (0 <= ent < n_tri, not an analytic
 * sphere), and uv[j][3][2], three finite f64 chart coordinates for the triangle's vertices 0, 1 and 2.  The chart is the caller's, a second UV set:
 * the scene's texture coordinates play no part on the device.  The same entity may appear in several rows.
 * The atlas is width x height texels.  Texel (x, y) is in row y from the top and has index t = y * width + x; its centre is
 *     pu = ((double) x + 0.5) / (double) width,  pv = ((double) y + 0.5) / (double) height
 * v grows with the row index; there is no wrap and no flip.  All arithmetic below is f64, IEEE + - * / only, in the order written, compiled without
 * contraction, so that it can be restated bit for bit (tests/lightmap_expect.py).
 * Coverage.  E(a, b, p) = (b.x - a.x) * (p.y - a.y) - (b.y - a.y) * (p.x - a.x).  For row j with chart vertices a, b, c: area = E(a, b, c),
 *   e0 = E(b, c, p), e1 = E(c, a, p), e2 = E(a, b, p).  A row with area == 0 or a non-finite area covers nothing.  Otherwise the row covers p iff
 *   p lies in the row's chart box -- min(a.x, b.x, c.x) <= p.x <= max(a.x, b.x, c.x) and the same in y, plain comparisons, both ends included --
 *   AND the edge test passes: e0 >= 0 && e1 >= 0 && e2 >= 0 if area > 0, all three <= 0 if area < 0.  Edges are inclusive: a texel centre on an
 *   edge shared by two rows is claimed by both.  The box is part of the definition, not a short cut: where the three vertices are collinear up to
 *   rounding the area is a tiny non-zero number and the edge values round to 0 or to its sign all along the line EXTENDED; the box ends such a
 *   sliver at its vertices.  The OWNER of a texel is the lowest row index that covers it.  Nothing of the result depends on the launch, nor on
 *   the size of the coordinates: which texels the rasteriser visits for a row is its own business, it applies this test to each.
 * Point of an owned texel.  b1 = e1 / area, b2 = e2 / area.  With the entity's vertex 0 and edges p0, e1v = p1 - p0, e2v = p2 - p0: per component
 *   P = (p0 + b1 * e1v) + b2 * e2v.  If the entity interpolates normals (all three vertex normals non-zero), N = ((1 - b1 - b2) * n0 + b1 * n1) + b2 * n2,
 *   else N = the face normal normalize(cross(p1 - p0, p2 - p0)).  params.flip != 0 negates N.  A texel whose N is 0 0 0 or not finite is NOT COVERED:
 *   its owner is reported as -1, and no other row inherits it.
 * Rank.  Covered texels are numbered i = 0 .. n_cov - 1 in ascending t.  points[n_cov][6] = P, N with texel[n_cov] = t is a GI_BAKE_TEXEL point list,
 *   and the bake is exactly gi_bake_* on it: sample k of covered texel i runs on stream_base + i * n_samples + k, with the same fold, the same
 *   chunking freedom and the same seed meaning.  Direct light of the analytic lights is not in it, as in every bake.
 * Scatter and dilation.  The atlas value of a covered texel is its bake row, f64.  Then `dilate` passes run.  In each pass, every texel that is not
 *   filled at the start of the pass and has at least one filled 8-neighbour takes the sum of its filled neighbours' values, from +0.0 in the order
 *   (x-1,y-1) (x,y-1) (x+1,y-1) (x-1,y) (x+1,y) (x-1,y+1) (x,y+1) (x+1,y+1), divided by (double) count; neighbours outside the atlas do not exist.
 *   The texel is filled from the next pass on (a pass reads only the state before it).  Texels still unfilled at the end are 0 0 0.
 * Outputs: atlas [height][width][3], float (out_is_f64 = 0) or double (1), rounded once on store; optionally owner [height][width] int32, the chart
 * row of a covered texel and -1 otherwise (dilated texels stay -1); optionally *n_covered.
 * GI_E_INVALID: a null pointer where one is needed (ent and uv may be null when n_chart is 0, which is GI_OK and gives an all-zero atlas with owner
 * -1), width or height outside 1 .. 8192, n_samples < 1, dilate outside 0 .. 64, flip other than 0 / 1, n_chart < 0,
 * stream_base + width * height * n_samples beyond 2^32 (every texel may be covered), and -- the host entries, which look at the chart -- an entity
 * index out of range, an entity that is a sphere, a non-finite coordinate.  gi_lightmap_device does NOT look at its chart, apart from clamping ent
 * to the entity tables.  GI_E_STATE: no scene.  A refused call touches no output and no timer.
 * gi_lightmap_default_params: 256 x 256, 256 samples, dilate 2, flip 0, stream_base 0, seed 0x9E3779B97F4A7C15.
 * gi_lightmap_device: DEVICE pointers for ent, uv, atlas and owner (n_covered is a host pointer); it waits for the stream once, to size the bake.
 * Scratch: 58 bytes per texel and 76 per covered texel of device memory, kept by the context for the next call; the host entries give it back when
 * they return if the atlas has more than 2^22 texels, gi_lightmap_device keeps it until a host entry or gi_destroy frees it.
 * gi_last_lightmap_ms: device time of the last lightmap, and per stage in stages3 (may be null): raster + rank, bake, scatter + dilate.
 * gi_last_bake_ms, the frame's and the other passes' times keep their values across a lightmap; an open progressive session is left as it is.
 * Check entries (host pointers): gi_lightmap_texels gives the texel table -- owner [height][width], *n_covered, points6 [cap][6], texel [cap];
 * cap < n_covered is GI_E_INVALID, but *n_covered and owner are still written.  gi_lightmap_dilate runs `passes` dilation passes on caller data:
 * values3 [height][width][3], filled [height][width] (0 / non-zero; the values of unfilled texels are not read), out3 [height][width][3]; no scene needed.
 * There is no gi_group_* form: split the atlas by rows of covered texels with stream_base, as the bake documents. */
typedef struct gi_lightmap_params {
    int32_t width, height;   /* 1 .. 8192 each */
    int32_t n_samples;       /* >= 1 directions per covered texel */
    int32_t dilate;          /* 0 .. 64 passes */
    int32_t flip;            /* 0 / 1: negate the normals */
    uint32_t stream_base;    /* stream index of sample 0 of covered texel 0 */
    uint64_t seed;           /* counter-RNG seed, as gi_bake_params::seed */
} gi_lightmap_params;
void gi_lightmap_default_params(gi_lightmap_params*);
int gi_lightmap_host(gi_ctx*, const gi_lightmap_params*, int32_t n_chart, const int32_t* ent, const double* uv, void* h_atlas, int out_is_f64, int32_t* h_owner, int32_t* n_covered);
int gi_lightmap_device(gi_ctx*, const gi_lightmap_params*, int32_t n_chart, const int32_t* d_ent, const double* d_uv, void* d_atlas, int out_is_f64, int32_t* d_owner, int32_t* n_covered);
int gi_last_lightmap_ms(gi_ctx*, float* ms, float* stages3);
int gi_lightmap_texels(gi_ctx*, const gi_lightmap_params*, int32_t n_chart, const int32_t* ent, const double* uv, int32_t* owner, int32_t* n_covered, double* points6, int32_t* texel, int32_t cap);
int gi_lightmap_dilate(gi_ctx*, int32_t width, int32_t height, int32_t passes, const double* values3, const int32_t* filled, double* out3);

/* Reflection probes -- an ADDITION beside the bakes: the specular product.  A probe is a cube map of the radiance seen from a point, captured with
 * the path tracer behind every ray as a bake's rays are, and the roughness mip chain filtered from it, in one device-side pass.
 * Texels and faces.  A cube of face N has 6 N^2 texels.  Faces run in the order +X, -X, +Y, -Y, +Z, -Z; texel (x, y) of face f has index
 *     t = (f * N + y) * N + x
 * and row y grows downward.  With a = (2.0 * ((double) x + ju)) / (double) N - 1.0 and b the same from y and jv, the unnormalised direction is
 *     f0 ( 1, -b, -a)   f1 (-1, -b,  a)   f2 ( a,  1,  b)   f3 ( a, -1, -b)   f4 ( a, -b,  1)   f5 (-a, -b, -1)
 * the layout of the usual cube-map texture.  The texel centre is ju = jv = 0.5.  All arithmetic below is f64, IEEE + - * / and sqrt only, in the
 * order written, compiled without contraction, so that it can be restated bit for bit (tests/cubemap_expect.py).
 * Capture.  Sample k of texel t runs on stream = stream_base + t * n_samples + k: ju = (double) halton(0, stream), jv = (double) halton(1, stream),
 *   the two dimensions a bake's ray takes for its direction; the ray is Ray(P, d) from the probe position P itself, with no bias (include/ray.h:7-17:
 *   d is normalised there); the rest of the index drives the path as it does for a bake.  No device trigonometry is involved: the rays are the
 *   statement's bit for bit, not within 4 ulp as a bake's are.  The texel's value is the texel fold of the bake: the sum over k of L_k in ascending k
 *   from +0.0, divided by (double) n_samples, L_k as gi_bake_* defines it.  Chunks of texels and ranges of samples (gi_set_pool_slots, free memory)
 *   do not show in the result.  As in a bake and in a frame, the analytic lights are not geometry: no ray hits one, so a probe holds no image of the
 *   lights themselves -- what they light, it holds.  The lens and the render mode play no part.
 * Box levels.  B_0 is the capture.  B_l has face N >> l, and each of its texels is ((p00 + p01) + (p10 + p11)) * 0.25 of B_(l-1), row-major in
 *   the 2 x 2 block, per channel.  levels > 1 requires N to be divisible by 2^(levels - 1).
 * Filtered levels.  F_0 = B_0, bit for bit.  For l >= 1, F_l has face n = N >> l and is filtered from B_(l-1), whose face is 2 n.  Per source
 *   texel s with centre (a, b) and unnormalised centre direction u:  d_s = u * (1.0 / sqrt((ux ux + uy uy) + uz uz));  m_s = 1.0 / (r * sqrt(r))
 *   with r = (1.0 + a a) + b b, the texel's solid angle up to a factor common to the level.  Per output texel with normalised centre direction R:
 *   c = (Rx dx + Ry dy) + Rz dz;  w = c > 0 ? c : 0, squared log2_exponent[l] times (the Phong lobe of exponent 2^log2_exponent[l]), then multiplied
 *   by m_s.  For each source face g, W_g += w and A_g[ch] += w * L_s[ch] over the face's texels in ascending s from +0.0.  Then
 *   W = ((((W_0 + W_1) + W_2) + W_3) + W_4) + W_5, A likewise, and F_l = A / W per channel.  Every sum is per face first, then the faces in order,
 *   whatever the launch.  A lobe so narrow that every weight underflows leaves W = 0 and the texel NaN (0 / 0): exponents are the caller's to suit to
 *   the face of the source level; the defaults are safe for every cube of face 4 or more.
 * Output.  The levels lie one after another, level l as [6][N >> l][N >> l][3], float (out_is_f64 = 0) or double (1); a float is the double rounded
 * once.  gi_cubemap_chain_texels(face, levels) is the number of texels of the chain, or -1 for a pair a call would refuse.
 * A consumer looks up level l at the direction d by the face of d's largest component and (a, b) of the table above divided by that component's size:
 * gi_render_baked_* is that consumer, and step 5 of its definition states the texel exactly.
 * GI_E_INVALID, before any pointer is used: a null pointer, face < 1, n_samples < 1, levels outside 1 .. GI_CUBEMAP_MAX_LEVELS, a face not
 * divisible by 2^(levels - 1), log2_exponent[l] outside 0 .. 16 for a level 1 <= l < levels (entry 0 and the entries from `levels` on are ignored),
 * stream_base + 6 N^2 n_samples beyond 2^32, and -- gi_cubemap_host and gi_cubemap_rays -- a position that is not finite.  GI_E_STATE: no scene.
 * A refused call touches no output and no timer.
 * gi_cubemap_default_params: face 32, 64 samples, 1 level (the capture alone), stream_base 0, seed 0x9E3779B97F4A7C15,
 *   log2_exponent[l] = max(0, 16 - 3 l).
 * gi_cubemap_host: pos3 and h_out are HOST pointers.  gi_cubemap_device: d_out is a DEVICE pointer, pos3 a HOST pointer read before the call returns
 *   and taken as it is; asynchronous on the context's stream.  Scratch: 24 bytes per texel of the chain and 32 bytes per texel of level 1 and source
 *   face (192 per texel of level 1) of device memory, kept by the context for the next call, beside the shared scratch of the stream passes.
 * gi_last_cubemap_ms: device time of the last probe, and per stage in stages2 (may be null): capture, prefilter.  gi_last_bake_ms, the frame's and
 *   the other passes' times keep their values across a probe; an open progressive session is left as it is.
 * Check entries (host pointers): gi_cubemap_rays gives the capture's rays as gi_bake_rays does, rays6_out [6 N^2 n_samples][6] and stream_out
 *   [6 N^2 n_samples], sample k of texel t in row t * n_samples + k; no scene is needed.  gi_cubemap_prefilter runs the box levels and the filter on
 *   the caller's cube: cube_in [6][N][N][3] double, chain_out the whole chain, double, level 0 the input's bits; params as for a capture; no scene
 *   is needed and no timer is touched.
 * There is no gi_group_* form and one probe per call: a caller with many probes loops. */
#define GI_CUBEMAP_MAX_LEVELS 12
typedef struct gi_cubemap_params {
    int32_t face;            /* N >= 1: texels per face edge */
    int32_t n_samples;       /* >= 1 rays per texel */
    int32_t levels;          /* 1 .. GI_CUBEMAP_MAX_LEVELS; 1: the capture alone */
    uint32_t stream_base;    /* stream index of sample 0 of texel 0 */
    uint64_t seed;           /* counter-RNG seed, as gi_bake_params::seed */
    int32_t log2_exponent[GI_CUBEMAP_MAX_LEVELS];   /* 0 .. 16 each: level l is filtered with the lobe cos^(2^log2_exponent[l]); entry 0 is ignored */
} gi_cubemap_params;
void gi_cubemap_default_params(gi_cubemap_params*);
int64_t gi_cubemap_chain_texels(int32_t face, int32_t levels);
int gi_cubemap_host(gi_ctx*, const double* pos3, const gi_cubemap_params*, void* h_out, int out_is_f64);
int gi_cubemap_device(gi_ctx*, const double* pos3, const gi_cubemap_params*, void* d_out, int out_is_f64);
int gi_last_cubemap_ms(gi_ctx*, float* ms, float* stages2);
int gi_cubemap_rays(gi_ctx*, const double* pos3, const gi_cubemap_params*, double* rays6_out, uint32_t* stream_out);
int gi_cubemap_prefilter(gi_ctx*, const gi_cubemap_params*, const double* cube_in, double* chain_out);

/* The baked-light pass -- an ADDITION: the consumer of the bakes.  A per-pixel pass beside the first-hit features and the occlusion: it shades the
 * frame's first hit from a grid of SH9 light probes (gi_bake_*, GI_BAKE_SH9), a reflection probe's chain (gi_cubemap_*) and the analytic lights -- a
 * preview of the scene at about the cost of a feature pass, with no path pool, no sorts and no gather.  Every operation of steps 3 to 7 is f64, IEEE
 * + - * / and sqrt only, in the order written, compiled without contraction, so that it can be restated bit for bit (tests/baked_expect.py).
 * Inputs beside the parameters: sh [nz][ny][nx][9][3] f64, the rows gi_bake_* gives for the nx x ny x nz probes at the CELL CENTRES of the box
 * grid_min .. grid_max, x fastest; chain, the whole chain as gi_cubemap_host writes it with out_is_f64 = 1, gi_cubemap_chain_texels(face, levels)
 * texels of 3.  A pointer may be null when its term's bit is clear.
 * Per pixel and per sample s = 0 .. n_samples-1 (Halton index, frame parameters, stripes and seed as for gi_render_occlusion_*; the context's lens applies):
 *   1. First hit: that of gi_render_features_* (same ray, same RNG keys).  From it: color, the feature pass's albedo (texture included); emissive,
 *      with its texture; N, minNorm of trace; P, the ray direction d, the material m.  norm = -N if dot(N, d) > 0 else N (secondaryRay's turn,
 *      include/raytracer.h:321-379: not renormalised); Nf as step 3 of the occlusion pass.  A miss adds the scene's ambient colour to beauty and
 *      nothing to the three terms.
 *   2. Direct: by definition what the frame's depth-0 shade adds for the analytic lights (include/raytracer.h:230-256), as the streaming passes
 *      compute it: per light li the draws P_LIGHT_Y | li << 8 and P_LIGHT_X | li << 8 of the stream at depth 0, the shadow ray from
 *      P + 0.0001 norm towards the point drawn on the light, asked of RayTracer::visible with light index li (the medium included, as in the
 *      frame), i_li = col * pow(max(0, dot(norm, normalize(lpos - P))), 1 / roughness) * (1 / (pi |lpos - P|^2)).  The reference keeps the share
 *      of the LAST visible light, so i = i_li of the highest li that is visible, or 0.  direct = color * i.  A one-sample frame of a scene whose
 *      paths all leave after the first hit, with no ambient light and no photons, is this term bit for bit.
 *   3. Lobe, by the roughness alone (rayType and secondaryRay without their draws): roughness < .001, a mirror: specular only, from level 0;
 *      .001 <= roughness < .9, glossy: specular only, from the material's level; otherwise diffuse only.  Opacity is ignored.
 *      The material's level: with levels == 1, level 0; else the l of 1 .. levels-1 whose log2_exponent[l] is nearest to
 *      log2(1 / roughness + 1) (host libm; the Phong exponent of the glossy bounce), ties to the lower l.  The table is made on the host per call.
 *   4. Diffuse = color * D.  Per axis with n probes: g = ((P - gmin) / (gmax - gmin)) * (double) n - 0.5, clamped to [0, n - 1]; i0 = floor(g),
 *      i1 = min(i0 + 1, n - 1), t = g - i0.  F_j = k_j * Y_j(Nf) with Y_j of GI_BAKE_SH9 (same order, same literals, each product as written
 *      there) and k_j = 1.0 (band 0), 0.6666666666666666 (band 1), 0.25 (band 2): the cosine lobe's factors over pi, so D is on the scale of a
 *      GI_BAKE_TEXEL result.  At each of the eight probes around P: D_c[ch] = sum over j, ascending from +0.0, of F_j * c_j[ch].  Then
 *      a + t * (b - a) along x, then y, then z; then each channel < 0 becomes 0.
 *   5. Specular = color * C_l(R), R = d - (Nf * dot(Nf, d)) * 2.0 with dot = (Nf.x d.x + Nf.y d.y) + Nf.z d.z.  The texel of R in level l of face
 *      n = face >> l: the face of the largest |component|, the first of equals; x, y, z = R / that size; (a, b) = (-z, -y) on +X, (z, -y) on -X,
 *      (x, z) on +Y, (x, -z) on -Y, (x, -y) on +Z, (-x, -y) on -Z; column = min(n - 1, max(0, (int) floor(((a + 1.0) * 0.5) * n))), row the same
 *      from b.  The nearest texel, read at R as if the surface stood at the probe; no blending between levels.  A NaN texel of an over-narrow lobe passes through.
 *   6. Emissive: the first hit's emissive.
 *   7. beauty = ((direct + diffuse) + specular) + emissive, a term whose bit is clear being +0.0.
 * Per pixel: the f64 sums over s in ascending order from +0.0 of the twelve channels, each divided once by (double) n_samples.  No reduction
 * across lanes: the result does not depend on stripes, the octree walk in use or the launch.
 * out [local_rows][width][12] = beauty rgb, direct rgb, diffuse rgb, specular rgb, float (out_is_f64 = 0) or double (1), rounded once on store.
 * What the preview is not: a transparent surface is shaded as opaque; the camera segment is not marched through the medium (the first hit is the
 * surface's, as in the feature pass); probes are looked up without visibility (gi_render_baked_visibility_* below looks them up with it), one cube is read for the whole scene at R itself
 * (gi_render_baked_reflections_* below reads a set of probes, each at the direction projected onto its box); a lightmap atlas (gi_lightmap_*) is read by gi_render_baked_lightmap_*
 * below, not by these two entries.
 * GI_E_INVALID: null parameters or output; n_samples < 1 or taking the Halton index beyond 32 bits; terms 0 or with unknown bits; a grid dimension
 * < 1 or more than 2^31 probes; with GI_BAKED_DIFFUSE: a null sh, non-finite bounds or grid_max <= grid_min on an axis; with GI_BAKED_SPECULAR: a
 * null chain, face, levels and log2_exponent not as gi_cubemap_params allows.  GI_E_STATE: no scene.  A refused call touches no output and no
 * timer; an open progressive session is left as it is.
 * gi_baked_default_params: 4 samples, terms DIRECT | EMISSIVE, a 1 x 1 x 1 grid in the unit box, face 32, 1 level, log2_exponent as gi_cubemap's.
 * gi_render_baked_device: DEVICE pointers (sh, chain, out), asynchronous on the context's stream, except that with GI_BAKED_SPECULAR it first waits
 * for the stream's earlier work, to replace the level table.  gi_render_baked_host: HOST pointers.
 * gi_last_baked_ms: device time of the last pass (HIP events around the kernel); the frame's and the other passes' times are left alone. */
#define GI_BAKED_DIRECT 1
#define GI_BAKED_DIFFUSE 2
#define GI_BAKED_SPECULAR 4
#define GI_BAKED_EMISSIVE 8
typedef struct gi_baked_params {
    int32_t n_samples;       /* >= 1 */
    int32_t terms;           /* GI_BAKED_* bits, at least one */
    double grid_min[3], grid_max[3];   /* the probe grid's box */
    int32_t nx, ny, nz;      /* >= 1 each: probes per axis, at the cell centres */
    int32_t face;            /* of the chain, as gi_cubemap_params::face */
    int32_t levels;          /* 1 .. GI_CUBEMAP_MAX_LEVELS */
    int32_t log2_exponent[GI_CUBEMAP_MAX_LEVELS];   /* as gi_cubemap_params::log2_exponent: what the levels were filtered with */
} gi_baked_params;
void gi_baked_default_params(gi_baked_params*);
int gi_render_baked_device(gi_ctx*, const gi_render_params*, const gi_baked_params*, const double* d_sh, const double* d_chain, void* d_out, int out_is_f64);
int gi_render_baked_host(gi_ctx*, const gi_render_params*, const gi_baked_params*, const double* sh, const double* chain, void* h_out, int out_is_f64);
int gi_last_baked_ms(gi_ctx*, float* ms);

/* The baked-light pass with a lightmap -- an ADDITION: the reader of the atlas gi_lightmap_* bakes.  The pass above, except that a first hit on a
 * diffuse surface that has a chart row takes its irradiance from a lightmap atlas at the hit's chart coordinate instead of the probe grid: the
 * per-texel detail an atlas is baked for -- contact shadows, colour bleeding -- shows in the preview.  Steps 1 to 3 and 5 to 7, the sums, the output
 * layout, the Halton index, the stripes and the lens are gi_render_baked_*'s.  Everything in the look-up is f64, IEEE + - * / only, in the order
 * written, compiled without contraction, so that it can be restated bit for bit (tests/baked_lightmap_expect.py).
 * Inputs beside those of gi_render_baked_*: a chart of n_chart rows, ent [n_chart] and uv [n_chart][3][2] in the form gi_lightmap_* takes, and
 * the atlas [height][width][3] baked for it (or any other image of that shape).  On the device the atlas is f64; the host entry takes float
 * (atlas_is_f64 = 0) or double (1) and widens a float exactly.
 *   Row of an entity.  row_of_ent[e] = the lowest chart row j with ent[j] == e, or none.  A row that names a sphere or no entity of the scene
 *     serves nothing.
 *   Which hits read the atlas.  A sample's first hit reads the atlas iff GI_BAKED_DIFFUSE is set, the material is on the diffuse lobe (step 3:
 *     roughness >= .9) and the hit entity has a row.  A diffuse-lobe hit on an entity without a row reads the probe grid as in step 4 if sh is
 *     given; if sh is null its diffuse term is +0.0.  The side the surface is seen from plays no part: a texel baked for the front is read from
 *     the back too.
 *   Chart coordinate.  A function of the entity and the hit position P alone (the P of step 1).  With the entity's vertex 0 and edges p0,
 *     e1v = p1 - p0, e2v = p2 - p0 as the library lays them out, and every dot written (x x' + y y') + z z':
 *       d = P - p0;  d00 = e1v.e1v, d01 = e1v.e2v, d11 = e2v.e2v, d20 = d.e1v, d21 = d.e2v;  den = d00 * d11 - d01 * d01;
 *       b1 = (d11 * d20 - d01 * d21) / den;  b2 = (d00 * d21 - d01 * d20) / den;
 *       u = ((1 - b1 - b2) * uv0.x + b1 * uv1.x) + b2 * uv2.x, and v the same from the .y components, uv0 uv1 uv2 the row's three coordinates.
 *     This inverts the point a lightmap puts under a texel, P = (p0 + b1 * e1v) + b2 * e2v.  A degenerate triangle has den = 0 and gives NaN or
 *     infinite coordinates, which the clamps below send to a border texel (a NaN to texel 0 of its axis).
 *   GI_LM_BILINEAR.  Per axis with n texels, centres at (x + 0.5) / n as in a lightmap: g = ((a - 0.0) / (1.0 - 0.0)) * (double) n - 0.5 clamped to
 *     [0, n - 1] (a NaN to 0), i0 = floor(g), i1 = min(i0 + 1, n - 1), t = g - i0 -- the cell of step 4 for the box 0 .. 1: coordinates beyond the
 *     outermost centres read the border texels.  Then a + t * (b - a) along x on rows y0 and y1, then along y; then each channel < 0 becomes 0.
 *   GI_LM_NEAREST.  Texel min(n - 1, max(0, (int) floor(a * (double) n))) per axis, a NaN going to 0; the texel's value as it is.
 *   Diffuse = color * E, E the filtered value: the atlas is on the scale of a GI_BAKE_TEXEL result, as a lightmap's is.
 * Texels no row of the chart covers are read as they are -- the filter knows nothing of owners: the caller dilates (gi_lightmap_params::dilate).
 * With n_chart = 0, or without GI_BAKED_DIFFUSE, the result is gi_render_baked_*'s on the same arguments, bit for bit (with a null sh, that of
 * the terms without GI_BAKED_DIFFUSE), and atlas, ent and uv may be null.
 * GI_E_INVALID, with a message that names render_baked_lightmap: everything gi_render_baked_* refuses, except that sh may be null with
 * GI_BAKED_DIFFUSE; null lightmap parameters; width or height outside 1 .. 8192; a filter other than the two; n_chart < 0; a null atlas, ent or uv
 * with n_chart > 0 and GI_BAKED_DIFFUSE; and -- gi_render_baked_lightmap_host, which looks at the chart as gi_lightmap_host does -- an entity
 * index out of range, an entity that is a sphere, a non-finite coordinate.  GI_E_STATE: no scene.  A refused call touches no output and no timer;
 * an open progressive session is left as it is.
 * gi_baked_lightmap_default_params: 256 x 256, GI_LM_BILINEAR, 0 rows.
 * gi_render_baked_lightmap_device: DEVICE pointers (sh, chain, atlas f64, ent, uv, out); it does not look at its chart; asynchronous on the
 * context's stream as gi_render_baked_device is.  The table row_of_ent [n_tri] is the context's, rebuilt by every call.
 * gi_last_baked_ms is this pass's timer too.  There is one atlas per call and no gi_group_* form. */
#define GI_LM_NEAREST 0
#define GI_LM_BILINEAR 1
typedef struct gi_baked_lightmap_params {
    int32_t width, height;   /* of the atlas, 1 .. 8192 each */
    int32_t filter;          /* GI_LM_NEAREST or GI_LM_BILINEAR */
    int32_t n_chart;         /* >= 0 rows of the chart */
} gi_baked_lightmap_params;
void gi_baked_lightmap_default_params(gi_baked_lightmap_params*);
int gi_render_baked_lightmap_host(gi_ctx*, const gi_render_params*, const gi_baked_params*, const gi_baked_lightmap_params*, const double* sh, const double* chain,
                                  const void* atlas, int atlas_is_f64, const int32_t* ent, const double* uv, void* h_out, int out_is_f64);
int gi_render_baked_lightmap_device(gi_ctx*, const gi_render_params*, const gi_baked_params*, const gi_baked_lightmap_params*, const double* d_sh, const double* d_chain,
                                    const double* d_atlas, const int32_t* d_ent, const double* d_uv, void* d_out, int out_is_f64);

/* Probe visibility, capture -- an ADDITION beside the bakes: what keeps a probe grid from leaking light through walls.  Beside its SH9 coefficients a
 * probe gets a small octahedral map of the mean and the mean squared distance to the nearest surface per direction, as the probe volumes of dynamic
 * diffuse GI keep; gi_render_baked_visibility_* below weights the probes around a hit by a Chebyshev test against these maps.  All arithmetic named
 * here is f64, IEEE + - * / and sqrt only, in the order written, compiled without contraction, so that it can be restated bit for bit
 * (tests/visibility_expect.py).
 * Octahedral map.  A map has M x M texels; texel (x, y) of probe i has index t = (i * M + y) * M + x.  sgn(q) = q >= 0 ? 1.0 : -1.0.
 *   Decode of (a, b) in [0, 1]^2:  px = 2.0 * a - 1.0;  py = 2.0 * b - 1.0;  vz = (1.0 - |px|) - |py|;  if vz < 0:
 *     (vx, vy) = ((1.0 - |py|) * sgn(px), (1.0 - |px|) * sgn(py)), otherwise (vx, vy) = (px, py).  The direction is (vx, vy, vz), not normalised.
 *   Encode of a vector v that is not 0 0 0:  s = (|vx| + |vy|) + |vz|;  px = vx / s;  py = vy / s;  the same fold when vz < 0;
 *     a = (px + 1.0) * 0.5;  b = (py + 1.0) * 0.5.
 * Rays.  Sample k of texel t runs on stream = stream_base + t * n_samples + k: ju = (double) halton(0, stream), jv = (double) halton(1, stream),
 *   a = ((double) x + ju) / (double) M, b the same from y and jv; the ray is Ray(P_i, decode(a, b)): the direction is normalised there, and the ray
 *   leaves the probe's position itself, with no bias, as a reflection probe's.
 * Distance.  The closest hit is RayTracer::trace of that ray, as the frame's primary ray gets it, alpha draws keyed by (seed, stream) at depth 0;
 *   on a scene whose alpha tests cannot depend on the draw this is gi_trace's answer.  On a hit at H, r = sqrt(((Hx-Px)^2 + (Hy-Py)^2) + (Hz-Pz)^2);
 *   on a miss r = max_dist; then r = r < max_dist ? r : max_dist.  The lens and the render mode play no part; no analytic light is hit.
 * Fold.  Per texel, in ascending k from +0.0:  m = sum(r_k) / (double) n_samples,  m2 = sum(r_k * r_k) / (double) n_samples.
 * out [n_points][M][M][2] = (m, m2), float (out_is_f64 = 0) or double (1), rounded once on store.  One lane owns a texel and nothing is reduced across
 * lanes: the result does not depend on the launch, the octree walk in use or gi_set_pool_slots, and a point list split over calls gives the same
 * maps when call a, starting at point a, passes stream_base + a * M * M * n_samples.
 * GI_E_INVALID, before any pointer is used: null parameters, size outside 1 .. 64, n_samples < 1, n_points < 0, a max_dist that is not finite or not
 * positive, stream_base + n_points * M * M * n_samples beyond 2^32, null points or output with n_points > 0, and -- gi_probe_visibility_host and
 * gi_probe_visibility_rays -- a position that is not finite.  GI_E_STATE: no scene.  n_points = 0 is GI_OK and writes nothing.  A refused call
 * touches no output and no timer; an open progressive session is left as it is.
 * gi_probe_visibility_default_params: size 8, 16 samples, stream_base 0, seed 0x9E3779B97F4A7C15, max_dist 1e30 (callers pass the scene's diagonal).
 * gi_probe_visibility_device: DEVICE pointers (points [n][3] f64, out), asynchronous on the context's stream; the points are not looked at.
 * gi_probe_visibility_host: HOST pointers.  gi_last_probe_visibility_ms: device time of the last capture (HIP events around the kernel); the
 * frame's and the other passes' times are left alone.
 * Check entries (host pointers): gi_probe_visibility_rays gives the capture's rays as gi_cubemap_rays does, rays6_out [n M M n_samples][6] and
 *   stream_out [n M M n_samples], sample k of texel t in row t * n_samples + k; no scene is needed.  gi_probe_visibility_fold runs the fold on
 *   caller distances dist [n_texels][n_samples] and writes out2 [n_texels][2], double; no scene is needed and no timer is touched.
 * There is no gi_group_* form: split the point list. */
typedef struct gi_probe_visibility_params {
    int32_t size;            /* M, 1 .. 64: the map is M x M texels */
    int32_t n_samples;       /* >= 1 rays per texel */
    uint32_t stream_base;    /* stream index of sample 0 of texel 0 of point 0 */
    uint64_t seed;           /* counter-RNG seed, as gi_bake_params::seed */
    double max_dist;         /* finite, > 0: a miss, and any hit farther away, counts as this distance */
} gi_probe_visibility_params;
void gi_probe_visibility_default_params(gi_probe_visibility_params*);
int gi_probe_visibility_device(gi_ctx*, const double* d_points, int32_t n_points, const gi_probe_visibility_params*, void* d_out, int out_is_f64);
int gi_probe_visibility_host(gi_ctx*, const double* points, int32_t n_points, const gi_probe_visibility_params*, void* h_out, int out_is_f64);
int gi_last_probe_visibility_ms(gi_ctx*, float* ms);
int gi_probe_visibility_rays(gi_ctx*, const double* points, int32_t n_points, const gi_probe_visibility_params*, double* rays6_out, uint32_t* stream_out);
int gi_probe_visibility_fold(gi_ctx*, int32_t n_texels, int32_t n_samples, const double* dist, double* out2);

/* The baked-light pass with probe visibility -- an ADDITION: gi_render_baked_* with the probes looked up WITH visibility, so that a probe behind a
 * wall does not light the hit.  Steps 1 to 3 and 5 to 7, the sums, the output layout, the Halton index, the stripes, the lens and the timer
 * (gi_last_baked_ms) are gi_render_baked_*'s.  Input beside theirs: vis [nz][ny][nx][M][M][2] f64, the maps gi_probe_visibility_* gives for the
 * grid's probes in the grid's order (M = size); the host entry takes float (vis_is_f64 = 0) or double (1) and widens a float exactly.  Everything
 * below is f64, IEEE + - * / and sqrt only, in the order written (tests/visibility_expect.py).
 *   4. Diffuse = color * D.  The cell per axis (i0, i1, t), F_j and D_c at a probe are step 4's of gi_render_baked_*.  For the eight corners
 *      c = cx + 2 cy + 4 cz in ascending c, with c_a the corner's bit of axis a:
 *      probe      j_a = c_a ? i1_a : i0_a;  q = (jz * ny + jy) * nx + jx.
 *      trilinear  w_a = c_a ? t_a : 1.0 - t_a;  tw = (wx * wy) * wz;  tw = tw > 0.001 ? tw : 0.001.
 *      position   Q_a = gmin_a + (((double) j_a + 0.5) / (double) n_a) * (gmax_a - gmin_a).
 *      back face  e = Q - P;  le = sqrt((ex ex + ey ey) + ez ez);  cb = le > 0 ? ((ex Nfx + ey Nfy) + ez Nfz) / le : 1.0;  h = (cb + 1.0) * 0.5;
 *                 wb = h * h + 0.2.
 *      visibility v = (P + Nf * normal_bias) - Q per component;  r = sqrt((vx vx + vy vy) + vz vz).  If r == 0, vis = 1.0.  Otherwise (a, b) =
 *                 encode(v), and (m, m2) = the bilinear value of map q at (a, b): per axis the cell of step 4 for the box 0 .. 1 with n = M (texel
 *                 centres at (x + 0.5) / M, clamped at the map's border, a NaN going to texel 0), then a + t * (b - a) along x on both rows, then
 *                 along y -- GI_LM_BILINEAR's rule without its clamp at 0, and with no wrap across the octahedral map's edges.  A texel value that
 *                 is NaN or not finite is the caller's: it passes through.  If r > m: var = |m * m - m2|;  dd = r - m;  ch = var / (var + dd * dd);
 *                 ch = (ch * ch) * ch;  vis = ch > vis_floor ? ch : vis_floor.  Otherwise vis = 1.0.
 *      weight     w = (tw * wb) * vis;  num[ch] += w * D_c[ch];  den += w, both from +0.0.
 *      Then D = num / den per channel, and each channel < 0 becomes 0.  den > 0: every factor has a positive floor.
 * With a null vis, or without GI_BAKED_DIFFUSE, the result is gi_render_baked_*'s on the same arguments, bit for bit, through the same kernel
 * instances.  gi_render_baked_lightmap_* takes no maps: combining a lightmap and probe visibility in one call is out of scope.
 * GI_E_INVALID, with a message that names render_baked_visibility: everything gi_render_baked_* refuses (a null sh with GI_BAKED_DIFFUSE among it,
 * with a map or without); null visibility parameters; size outside 1 .. 64; a normal_bias that is not finite or negative; a vis_floor outside
 * (0, 1].  GI_E_STATE: no scene.  A refused call touches no output and no timer; an open progressive session is left as it is.
 * gi_baked_visibility_default_params: size 8, normal_bias 0.0, vis_floor 0.05.
 * gi_render_baked_visibility_device: DEVICE pointers (sh, chain, vis f64, out), asynchronous on the context's stream as gi_render_baked_device is.
 * gi_render_baked_visibility_host: HOST pointers.  There is no gi_group_* form. */
typedef struct gi_baked_visibility_params {
    int32_t size;            /* M of the maps, 1 .. 64 */
    double normal_bias;      /* finite, >= 0: the hit is moved this far along Nf before it is tested against the maps */
    double vis_floor;        /* 0 < vis_floor <= 1: the least visibility weight of a probe */
} gi_baked_visibility_params;
void gi_baked_visibility_default_params(gi_baked_visibility_params*);
int gi_render_baked_visibility_device(gi_ctx*, const gi_render_params*, const gi_baked_params*, const gi_baked_visibility_params*, const double* d_sh, const double* d_chain,
                                      const double* d_vis, void* d_out, int out_is_f64);
int gi_render_baked_visibility_host(gi_ctx*, const gi_render_params*, const gi_baked_params*, const gi_baked_visibility_params*, const double* sh, const double* chain,
                                    const void* vis, int vis_is_f64, void* h_out, int out_is_f64);

/* The baked-light pass with a reflection probe set -- an ADDITION: gi_render_baked_* with the specular term read from a SET of reflection probes,
 * box-projected and blended, so that a mirror floor shows the room as seen from the floor and every room shows its own reflections.  Each probe
 * has an influence box that also serves as proxy geometry: the reflection ray is cut with the box, the probe's cube is read in the direction
 * from the probe to that point, and probes whose boxes overlap are blended by the distance of the hit to their boxes' faces.  Steps 1 to 4, 6 and
 * 7, the sums, the output layout, the Halton index, the stripes, the lens and the timer (gi_last_baked_ms) are gi_render_baked_*'s.  Inputs beside
 * theirs: probes [K][10] f64, one row per probe: pos[3], box_min[3], box_max[3], fade; chains [K][texels][3] f64, K chains as gi_cubemap_* makes
 * them, all of the face, levels and log2_exponent of gi_baked_params, texels = gi_cubemap_chain_texels(face, levels); K = n_probes, 1 ..
 * GI_REFLECTIONS_MAX_PROBES.  Everything below is f64, IEEE + - * / and comparisons only, in the order written (tests/reflections_expect.py).
 *   5. Specular = color * S, for a first hit on the mirror or glossy lobe.  P, d, Nf, the level l and R = d - (Nf * dot(Nf, d)) * 2.0 are step
 *      5's of gi_render_baked_*; n = face >> l, off_l the texels before level l.  For k = 0 .. K-1 in ascending order, acc and W from +0.0:
 *      containment  box_min[a] <= P[a] <= box_max[a] on all three axes (a NaN fails); a probe that does not contain P adds nothing.
 *      edge         the least of P.x - min.x, max.x - P.x, P.y - min.y, max.y - P.y, P.z - min.z, max.z - P.z: the first, then each later one
 *                   where it is smaller.
 *      weight       w = fade > 0 ? (edge / fade < 1 ? edge / fade : 1.0) : 1.0.
 *      exit         per axis a with R[a] != 0: v_a = ((R[a] > 0 ? box_max[a] : box_min[a]) - P[a]) / R[a]; t = v of the first such axis in the
 *                   order x, y, z, then each later v where it is smaller; with no such axis t = 0.
 *      direction    Q = P + t * R;  D = Q - pos.  If a component of D is not finite, or all three are 0, D = R.
 *      accumulate   v = chains[k][off_l + texel(D, n)] with step 5's texel rule;  acc[ch] += w * v[ch];  W += w.
 *      If W > 0: S = acc / W per channel.  Otherwise -- the hit is in no box, or only on faces of boxes with a fade -- k* = the probe with the
 *      least ((dx dx + dy dy) + dz dz), d = P - pos, the first of equals, a NaN never less (k* = 0 when none is less than infinity), and
 *      S = chains[k*][off_l + texel(R, n)]: step 5 of gi_render_baked_* on that probe's chain.
 * The texel rule clamps rows and columns and sends a NaN to texel 0, so whatever the table holds no read leaves chains[k].
 * With n_probes = 0, or without GI_BAKED_SPECULAR, the result is gi_render_baked_*'s on (sh, chain), bit for bit, through the same kernel
 * instances; probes and chains may then be null.  With n_probes > 0 chain is not read and may be null.  Combining a probe set with a lightmap or
 * with visibility maps in one call is out of scope.
 * GI_E_INVALID, with a message that names render_baked_reflections: everything gi_render_baked_* refuses, except a null chain when n_probes > 0;
 * null reflections parameters; n_probes outside 0 .. 64; null probes or chains with n_probes > 0 and GI_BAKED_SPECULAR; and --
 * gi_render_baked_reflections_host, which looks at the table -- a pos, box or fade that is not finite, box_max <= box_min on an axis, fade < 0.
 * GI_E_STATE: no scene.  A refused call touches no output and no timer; an open progressive session is left as it is.
 * gi_baked_reflections_default_params: 0 probes.
 * gi_render_baked_reflections_device: DEVICE pointers (sh, chain, probes, chains, out); it does not look at its table; asynchronous on the
 * context's stream as gi_render_baked_device is.  gi_render_baked_reflections_host: HOST pointers.  There is no gi_group_* form. */
#define GI_REFLECTIONS_MAX_PROBES 64
typedef struct gi_baked_reflections_params {
    int32_t n_probes;        /* K, 0 .. GI_REFLECTIONS_MAX_PROBES; 0: gi_render_baked_* on (sh, chain) */
} gi_baked_reflections_params;
void gi_baked_reflections_default_params(gi_baked_reflections_params*);
int gi_render_baked_reflections_device(gi_ctx*, const gi_render_params*, const gi_baked_params*, const gi_baked_reflections_params*, const double* d_sh, const double* d_chain,
                                       const double* d_probes, const double* d_chains, void* d_out, int out_is_f64);
int gi_render_baked_reflections_host(gi_ctx*, const gi_render_params*, const gi_baked_params*, const gi_baked_reflections_params*, const double* sh, const double* chain,
                                     const double* probes, const double* chains, void* h_out, int out_is_f64);

/* The final-gather pass -- an ADDITION: one bounce from the first hits into the baked light, the step between gi_render_baked_* (which reads the
 * probe grid at the first hit itself, so the picture has the grid's resolution) and the path tracer.  From a diffuse first hit it shoots n_dirs
 * cosine-distributed rays, shades what they hit from the baked data -- the analytic lights, the probe grid, one cube chain, emission -- and
 * averages: the grid is read one bounce away, where its coarseness is averaged over the hemisphere, at the cost of n_dirs closest-hit walks per
 * sample, with no path pool, no sorts and no gather.  Inputs: sh and chain as gi_render_baked_* takes them.  sh is needed with GI_BAKED_DIFFUSE
 * (pass a grid of zeros for a frame without baked irradiance); chain is needed with GI_BAKED_SPECULAR and otherwise optional: when given,
 * secondary hits on mirror and glossy surfaces read it, when null that read is +0.0 -- face, levels and log2_exponent are checked whenever a
 * chain is given.  Per pixel and per sample s = 0 .. n_samples-1 with Halton index idx:
 *   1. First hit: step 1 of gi_render_baked_* (same ray, same RNG keys: seed, stream idx, depth 0; the context's lens applies).  A miss adds the
 *      ambient colour to beauty and nothing to the three terms.
 *   2. Direct, specular and emissive of the first hit: steps 2, 3, 5 and 6 of gi_render_baked_*, unchanged.  Without GI_BAKED_DIFFUSE the pass is
 *      gi_render_baked_* bit for bit.
 *   3. Diffuse, for a first hit on the diffuse lobe (roughness >= .9) with GI_BAKED_DIFFUSE: O = P + 0.0001 Nf.  For j = 0 .. n_dirs-1:
 *      u = (float) draw(purpose 36, a = j), v = (float) draw(purpose 37, a = j) of the stream at depth 0; d_j = hemisphereSample_cos(Nf, u, v, 2)
 *      (include/util.cpp:35-58), the lobe of the path tracer's diffuse bounce and of GI_BAKE_TEXEL.  The closest hit of the ray (O, d_j) -- d_j as
 *      the sampler gave it, not renormalised: gi_trace on the row (O, d_j) states it -- is RayTracer::trace's, its alpha draws those of the
 *      stream's RNG with depth = 1 + j.  The medium is not marched along the ray.
 *        a miss:  L_j = ambient.
 *        a hit at Q on entity e with material m: color_Q, emissive_Q (textures applied) and roughness_Q are m's; N = minNorm of trace;
 *                 normQ = -N if dot(N, d_j) > 0 else N (not renormalised); NfQ = normQ * (1 / sqrt(dot(normQ, normQ)));
 *                 i_Q = step 2's i at (Q, normQ, roughness_Q) with the RNG at depth 1 + j (light draws and shadow-ray alpha draws alike; the
 *                 medium included, as in step 2);  base_Q = emissive_Q + color_Q * i_Q.
 *                 roughness_Q >= .9:            L_j = base_Q + color_Q * D(Q, NfQ), D step 4's of gi_render_baked_* (the plain grid).
 *                 roughness_Q < .9, a chain:    L_j = base_Q + color_Q * chain[l][texel(R)], R = d_j - (NfQ * dot(NfQ, d_j)) * 2.0, step 5's
 *                                               texel rule, l = 0 for roughness_Q < .001 else m's level (step 3's table).
 *                 roughness_Q < .9, no chain:   L_j = base_Q.
 *      The terms bits do not gate what a secondary hit adds.  E = (((+0.0 + L_0) + L_1) + ... + L_{n_dirs-1}) / (double) n_dirs per channel;
 *      diffuse = color * E.  Each product and sum above is one IEEE operation per channel, in the order written.
 *   4. beauty = ((direct + diffuse) + specular) + emissive, a term whose bit is clear being +0.0.
 * Per pixel: the f64 sums over s in ascending order from +0.0 of the twelve channels, each divided once by (double) n_samples; no reduction
 * across lanes, so the result does not depend on stripes, the octree walk in use or the launch.
 * out [local_rows][width][12] = beauty rgb, direct rgb, diffuse rgb, specular rgb, as gi_render_baked_* lays them out, float or double, rounded
 * once on store.  ids (optional) [local_rows][width][n_samples][n_dirs] int32: the entity gather ray j of sample s hit; -1: it left the scene;
 * -2: no gather for that sample (the first hit missed or is not on the diffuse lobe, or GI_BAKED_DIFFUSE is clear).
 * What is exact and what is not: d_j comes from sin, cos and sqrt of the device's math library, a few ulp from the host's, so Q and what is read
 * there carry that, and a ray that grazes an edge may hit another entity; everything else is stated bit for bit (tests/finalgather_expect.py).
 * Out of scope: lightmap atlases, probe visibility and probe sets at the secondary hits (only the plain grid and one chain are read there);
 * gathering from mirror and glossy first hits; the medium along the gather rays.
 * GI_E_INVALID, with a message that names render_final_gather: everything gi_render_baked_* refuses on the baked block (a null sh with
 * GI_BAKED_DIFFUSE, a null chain with GI_BAKED_SPECULAR, face / levels / log2_exponent not as gi_cubemap_params allows when there is a chain),
 * n_dirs outside 1 .. 64, reserved != 0, null parameters or output.  GI_E_STATE: no scene.  A refused call touches no output and no timer; an
 * open progressive session is left as it is.
 * gi_final_gather_default_params: gi_baked_default_params with terms DIRECT | DIFFUSE | EMISSIVE, 16 directions.
 * gi_render_final_gather_device: DEVICE pointers (sh, chain, out, ids), asynchronous on the context's stream, except that with a chain it first
 * waits for the stream's earlier work, to replace its level table.  gi_render_final_gather_host: HOST pointers.
 * gi_last_final_gather_ms: device time of the last pass (HIP events around the kernel); the frame's and every other pass's times are left alone.
 * There is no gi_group_* form. */
typedef struct gi_final_gather_params {
    gi_baked_params baked;   /* n_samples, terms, the grid, face, levels, log2_exponent: as gi_render_baked_* */
    int32_t n_dirs;          /* 1 .. 64 gather rays per sample */
    int32_t reserved;        /* must be 0 */
} gi_final_gather_params;
void gi_final_gather_default_params(gi_final_gather_params*);
int gi_render_final_gather_device(gi_ctx*, const gi_render_params*, const gi_final_gather_params*, const double* d_sh, const double* d_chain, void* d_out, int out_is_f64,
                                  int32_t* d_ids);
int gi_render_final_gather_host(gi_ctx*, const gi_render_params*, const gi_final_gather_params*, const double* sh, const double* chain, void* h_out, int out_is_f64,
                                int32_t* h_ids);
int gi_last_final_gather_ms(gi_ctx*, float* ms);

#ifdef __cplusplus
}
#endif
#endif
