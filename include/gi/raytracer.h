// include/gi/raytracer.h -- drop-in for the reference's RayTracer (include/raytracer.h:23-735) on the MI355X path.
// Same public data (photons, photon_depth, min_samples, max_samples, noise_thresh, ambient, _camera, width, height, p), same life cycle
// (RayTracer(camera); setScene(octree); start(); run(w, h) on a worker thread while the GUI thread polls getImage() every 32 ms; stop()),
// copyable with shared scene / photon map / image exactly as gui.h:19 / viewer.h:16 need, and the per-ray methods with the reference's
// signatures (trace, visible, samplePhotons, radiance, tracePhotons, secondaryRay, rayType, raymarch).
//
// run() flattens + uploads when the scene is not valid, emits photons on the GPU when the photon map is not valid, then renders the
// frame in stripes (`progressive_rows` = 16 rows first, doubling while a step is shorter than `progressive_ms`) through gi_render_host: after every stripe its pixels go through gamma 2.2 / clamp / the
// truncating 8-bit store into the shared Image (the display frame fills top to bottom as the reference's does row by row,
// include/raytracer.h:93-160), and `_running` is polled (include/raytracer.h:98) -- stop() ends run() within one stripe.
// trace / visible / samplePhotons / radiance / tracePhotons run on the GPU through the C ABI (one-element batches); there is no CPU
// renderer behind this class: without a usable HIP device run() leaves the image black and last_error() says why.
// secondaryRay / rayType / raymarch are the kernels' per-lane functions evaluated on the host for a single vertex (detail.h) -- the
// reference draws drand() inside them; here the draws come from the counter RNG keyed by (seed, rng_stream, rng_depth).
#pragma once
#include <chrono>
#include <cmath>
#include <cstdio>
#include <memory>
#include <string>
#include <vector>
#include "../gi_hip.h"
#include "camera.h"
#include "entities.h"
#include "halton_enum.h"
#include "halton_sampler.h"
#include "image.h"
#include "octree.h"
#include "photonMap.h"

class RayTracer {
  public:
    int p = 0;
    int width = 0, height = 0;

    RayTracer() = delete;
    RayTracer(const Camera& camera) : _camera(camera), _st(std::make_shared<State>()), _image(std::make_shared<Image>(0, 0)) {}

    void setScene(Octree* scene)   // include/raytracer.h:35-39: the photon map lives in the scene's root box
    {
        _scene = scene;
        _st->photon_map = std::make_shared<PhotonMap>(scene->_root._bbox.min, scene->_root._bbox.max);
        _st->uploaded = false;
        _st->photons_uploaded = false;
        _st->fresh_map = true;
    }

    // RayTracer::run(w, h), include/raytracer.h:41-165
    void run(int w, int h)
    {
        _image = std::make_shared<Image>(w, h);
        width = w; height = h;
        if (!prepare()) return;
        _linear.assign((size_t)w * h * 3, 0.f);
        if (_st->group) { run_on_group(w, h); return; }
        int rows = progressive_rows > 0 ? std::min(progressive_rows, h) : h;
        std::vector<double> lin;
        std::vector<uint8_t> rgb;
        for (int y0 = 0; y0 < h;) {
            if (!_running) return;                                   // RayTracer::stop(), polled per row in the reference (include/raytracer.h:98)
            gi_render_params rp = params(w, h);
            rp.stripe_h = rows; rp.stripe_rank = y0 / rows; rp.stripe_world = (h + rows - 1) / rows;   // this call renders one stripe only (y0 is a multiple of rows)
            const int nr = std::min(rows, h - y0);
            rows_in_flight = nr;
            lin.resize((size_t)nr * w * 3);
            _cancel = _running ? 0 : 1;
            const auto t0 = std::chrono::steady_clock::now();
            if (check(gi_render_host(_st->ctx, &rp, lin.data(), 1, nullptr, &_cancel)) != 0) return;
            const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            show_rows(lin.data(), rgb, y0, nr, w);
            y0 += nr;
            rows = next_rows(rows, y0, ms);
        }
    }

  private:
    // Stripes grow while a step is shorter than `progressive_ms`: a render call has a floor of some 20 ms whatever its size (the chain of up to 64
    // dependent bounces of its deepest path), so a frame in 16-row steps would spend nearly all its time there -- the first stripe appears at once,
    // the following ones double (16, 16, 32, 64, ...; the next start row stays a multiple of the stripe height, which is what the stripe
    // parameters of the C ABI address) until a step takes long enough for the viewer's 32 ms repaint to show progress.
    int next_rows(int rows, int y0, double ms) const
    {
        return progressive_ms > 0 && progressive_rows > 0 && ms < progressive_ms && y0 % (2 * rows) == 0 ? 2 * rows : rows;
    }
    // the same frame over every visible GPU (gi_group_*, include/gi_hip.h): each progressive step renders one stripe per device
    void run_on_group(int w, int h)
    {
        const int n = gi_group_size(_st->group);
        int rows = progressive_rows > 0 ? std::min(progressive_rows, h) : (h + n - 1) / n;
        std::vector<double> frame((size_t)w * h * 3, 0.0);
        std::vector<uint8_t> rgb;
        for (int y0 = 0; y0 < h;) {
            if (!_running) return;
            gi_render_params rp = params(w, h);
            const int total = (h + rows - 1) / rows, k = y0 / rows;
            const int ns = std::min(n, total - k), nr = std::min(ns * rows, h - y0);
            rows_in_flight = nr;
            _cancel = _running ? 0 : 1;
            const auto t0 = std::chrono::steady_clock::now();
            const int rc = gi_group_render_host(_st->group, &rp, rows, k, ns, frame.data(), 1, nullptr, &_cancel);
            if (rc != 0) { if (rc != GI_E_CANCELLED) { _st->err = gi_group_last_error(_st->group); fprintf(stderr, "gi: %s\n", _st->err.c_str()); } return; }
            const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            show_rows(frame.data() + (size_t)y0 * w * 3, rgb, y0, nr, w);
            y0 += nr;
            rows = next_rows(rows, y0, ms);
        }
    }
    // gamma(color, 2.2), glm::clamp, (int)(255 c) of rows [y0, y0 + nr) into the shared image: include/raytracer.h:150-157
    void show_rows(const double* lin, std::vector<uint8_t>& rgb, int y0, int nr, int w)
    {
        const size_t n = (size_t)nr * w * 3;
        rgb.resize(n);
        gih_to_rgb8(lin, 1, (int64_t)n, rgb.data());
        for (int y = 0; y < nr; y++)
            for (int x = 0; x < w; x++) _image->setPixel8(x, y0 + y, &rgb[((size_t)y * w + x) * 3]);
        for (size_t i = 0; i < n; i++) _linear[(size_t)y0 * w * 3 + i] = (float)lin[i];
        rows_done = y0 + nr;
    }

  public:

    // ---- per-ray methods, signatures of include/raytracer.h:167,280,382,532,582 -- each is a one-element batch on the GPU
    bool trace(const Ray& ray, gi::dvec3& minHit, gi::dvec3& minNorm, gi::dvec2& minUV, Entity*& obj)
    {
        if (!ready()) return false;
        const double r[6] = {ray.origin.x, ray.origin.y, ray.origin.z, ray.dir.x, ray.dir.y, ray.dir.z};
        int32_t hit = 0, ent = -1;
        double res[8];
        if (check(gi_trace(_st->ctx, 1, r, &hit, &ent, res)) != 0 || !hit) return false;
        minHit = gi::get3(res); minNorm = gi::get3(res + 3);
        obj = _scene->entities()[(size_t)ent];
        // `uv` as Entity::intersect leaves it: interpolated texCoords of a smooth triangle, asin / atan2 of a sphere, untouched for a flat triangle
        gi::dvec3 h2(0, 0, 0), n2(0, 0, 0);
        gi::dvec2 uv = minUV;
        if (obj->intersect(ray, h2, n2, uv)) minUV = uv;
        return true;
    }
    bool visible(const Ray& ray, double mt)
    {
        if (!ready()) return false;
        const double r[6] = {ray.origin.x, ray.origin.y, ray.origin.z, ray.dir.x, ray.dir.y, ray.dir.z};
        int32_t vis = 0;
        return check(gi_visible_rays(_st->ctx, 1, r, &mt, &vis)) == 0 && vis != 0;
    }
    gi::dvec3 samplePhotons(gi::dvec3 pos, gi::dvec3 dir, int count)
    {
        if (count != GI_GATHER_K) { _st->err = "samplePhotons: the gather kernel selects 32 photons (the only count the reference uses)"; return gi::dvec3(0, 0, 0); }
        if (!ready() || !photons_ready()) return gi::dvec3(0, 0, 0);
        const double q[6] = {pos.x, pos.y, pos.z, dir.x, dir.y, dir.z};
        double res[3] = {0, 0, 0};
        check(gi_gather(_st->ctx, 1, q, res, nullptr));
        return gi::get3(res);
    }
    // radiance(ray, 0, sampler, enumerator, sample, (1,1,1)): `sample` is the Halton index = the stream of the counter RNG
    gi::dvec3 radiance(const Ray& ray, int depth, const Halton_sampler&, const Halton_enum&, int sample, gi::dvec3 contrib)
    {
        if (depth != 0 || contrib.x != 1 || contrib.y != 1 || contrib.z != 1) { _st->err = "radiance: paths start at depth 0 with contrib 1 (the recursion is a loop inside the kernel)"; return gi::dvec3(0, 0, 0); }
        if (!ready() || !photons_ready()) return gi::dvec3(0, 0, 0);
        const double r[6] = {ray.origin.x, ray.origin.y, ray.origin.z, ray.dir.x, ray.dir.y, ray.dir.z};
        const uint32_t stream = (uint32_t)sample;
        double out[3] = {0, 0, 0};
        check(gi_radiance(_st->ctx, 1, r, &stream, seed, out));
        return gi::get3(out);
    }
    // photon emission on the GPU; the stored photons are appended to the map (include/raytracer.h:582-715)
    void tracePhotons(int maxDepth, int count, Halton_sampler&, Halton_enum&) { tracePhotons(maxDepth, count); }
    void tracePhotons(int maxDepth, int count)
    {
        if (!ready() || count <= 0 || _scene->lights.empty()) return;
        std::vector<double> out((size_t)count * _scene->lights.size() * 9);
        int64_t tries = 0;
        const int n = gi_emit_photons(_st->ctx, count, maxDepth, seed, out.data(), (int32_t)(out.size() / 9), &tries);
        if (n < 0) { check(n); return; }
        _st->photon_map->reserve(_st->photon_map->size() + n);
        for (int i = 0; i < n; i++) _st->photon_map->push_back(new Photon(gi::get3(&out[(size_t)i * 9]), gi::get3(&out[(size_t)i * 9 + 3]), gi::get3(&out[(size_t)i * 9 + 6])));
    }

    // ---- ADDITION (the reference has no such member): the first-hit feature buffers of the w x h frame run() renders -- per pixel the mean over
    // samples 0 .. n-1 of what radiance() holds after trace() of the primary ray (diffuse->get(minUV), minNorm, |minHit - origin|, 1 on a hit), and the
    // entity / material index of sample 0's hit (-1 on a miss; entity = index into Octree::entities()).  gi_render_features_host on the context of
    // the per-ray methods (device 0 of a group); false with last_error() set when it cannot run.
    struct Features {
        int width = 0, height = 0, samples = 0;
        std::vector<double> albedo, normal;      // [height][width][3]
        std::vector<double> depth, coverage;     // [height][width]
        std::vector<int32_t> entity, material;   // [height][width]
    };
    bool renderFeatures(int w, int h, int n, Features& out)
    {
        if (!ready()) return false;
        const gi_render_params rp = params(w, h);
        const size_t npix = (size_t)(w > 0 ? w : 0) * (size_t)(h > 0 ? h : 0);
        std::vector<double> buf(npix * 8 + 8);
        std::vector<int32_t> ids(npix * 2 + 2);
        if (check(gi_render_features_host(_st->ctx, &rp, n, buf.data(), 1, ids.data())) != 0) return false;
        out.width = w; out.height = h; out.samples = n;
        out.albedo.resize(npix * 3); out.normal.resize(npix * 3); out.depth.resize(npix); out.coverage.resize(npix);
        out.entity.resize(npix); out.material.resize(npix);
        for (size_t i = 0; i < npix; i++) {
            for (int k = 0; k < 3; k++) { out.albedo[i * 3 + k] = buf[i * 8 + k]; out.normal[i * 3 + k] = buf[i * 8 + 3 + k]; }
            out.depth[i] = buf[i * 8 + 6]; out.coverage[i] = buf[i * 8 + 7];
            out.entity[i] = ids[i * 2]; out.material[i] = ids[i * 2 + 1];
        }
        return true;
    }

    // ---- ADDITION (the reference's camera is a pinhole: FOCAL_BLUR == 0): a thin lens for every frame and pass of this RayTracer -- run(),
    // renderFeatures, renderOcclusion -- on every device it renders on (gi_set_lens / gi_group_set_lens; include/gi_hip.h states the definition).
    // radius in scene units (0: the pinhole again), blades 3 .. 16, rotation in radians.  The plane that stays sharp is the camera's sensor plane,
    // focalDist in front of it.  false with last_error() set when the lens is refused (the lens then stays as it was) or no device is usable.
    bool setLens(double radius, int blades = 6, double rotation = 0)
    {
        if (!ensure_context()) return false;
        gi_lens l;
        l.radius = radius; l.rotation = rotation; l.blades = blades; l.reserved = 0;
        return check(_st->group ? gi_group_set_lens(_st->group, &l) : gi_set_lens(_st->ctx, &l)) == 0;
    }
    // ---- ADDITION: move the sharp plane to `dist` in front of the camera.  sensorDiag and focalDist are both multiplied by dist / focalDist, so the
    // field of view is kept.  false for a distance that is not finite and > 0 (the camera is then left alone).
    bool focusAt(double dist)
    {
        if (!(dist > 0) || !(dist < INFINITY)) return false;
        const double k = dist / _camera.focalDist;
        _camera.sensorDiag = _camera.sensorDiag * k; _camera.focalDist = _camera.focalDist * k;
        return true;
    }

    // ---- ADDITION (the reference has no such member): ambient occlusion and bent normals of the w x h frame run() renders (include/gi_hip.h states
    // the definition): per pixel the share of the segments above the first hit that meet nothing within the radius, and their mean direction.
    // op = nullptr: gi_occlusion_default_params (16 samples, 16 directions, a tenth of the scene box's diagonal).  gi_render_occlusion_host on the
    // context of the per-ray methods; false with last_error() set when it cannot run (out is then left alone).
    struct Occlusion {
        int width = 0, height = 0, samples = 0, dirs = 0;
        std::vector<double> open;                // [height][width]
        std::vector<double> bent;                // [height][width][3]
    };
    bool renderOcclusion(int w, int h, Occlusion& out, const gi_occlusion_params* op = nullptr)
    {
        if (!ready()) return false;
        const gi_render_params rp = params(w, h);
        gi_occlusion_params p;
        if (op) p = *op; else gi_occlusion_default_params(&p);
        const size_t npix = (size_t)(w > 0 ? w : 0) * (size_t)(h > 0 ? h : 0);
        std::vector<double> buf(npix * 4 + 4);
        if (check(gi_render_occlusion_host(_st->ctx, &rp, &p, buf.data(), 1)) != 0) return false;
        out.width = w; out.height = h; out.samples = p.n_samples; out.dirs = p.n_dirs;
        out.open.resize(npix); out.bent.resize(npix * 3);
        for (size_t i = 0; i < npix; i++) {
            out.open[i] = buf[i * 4];
            for (int k = 0; k < 3; k++) out.bent[i * 3 + k] = buf[i * 4 + 1 + k];
        }
        return true;
    }

    // ---- ADDITION (the reference's paths all start at the camera): light baking on the context of the per-ray methods (gi_bake_host; include/gi_hip.h
    // states the definition, and what a bake does not hold: direct light of the lights at the point itself).  Sample k of point i runs on stream
    // streamBase + i * samples + k under this RayTracer's seed.  false with last_error() set when it cannot run (out is then left alone).
    // bakeProbes: points [n][3] -> out [n][9][3], the SH coefficients of bands 0 to 2 of the incident radiance, per colour channel.
    bool bakeProbes(const std::vector<double>& points, int samples, std::vector<double>& out, uint32_t streamBase = 0)
    {
        return bake(GI_BAKE_SH9, points, 3, 27, samples, streamBase, out);
    }
    // bakeTexels: pointsAndNormals [n][6] = position, normal -> out [n][3], the factor a roughness-1 albedo is multiplied by for its indirect term.
    bool bakeTexels(const std::vector<double>& pointsAndNormals, int samples, std::vector<double>& out, uint32_t streamBase = 0)
    {
        return bake(GI_BAKE_TEXEL, pointsAndNormals, 6, 3, samples, streamBase, out);
    }
    // bakeReflectionProbe (gi_cubemap_host): the cube map of the radiance seen from pos, `face` texels per face edge and `samples` jittered rays per
    // texel, and `levels` levels of the roughness chain filtered from it (1: the capture alone; face must be divisible by 2^(levels - 1)).  out gets
    // one vector per level, [6][face >> l][face >> l][3]: faces +X, -X, +Y, -Y, +Z, -Z, rows growing downward.  log2Exponents (optional, indexed by
    // level, entry 0 ignored) replaces the default lobe exponents 2^(16 - 3 l).  The lights themselves are not in it: no ray hits an analytic light.
    bool bakeReflectionProbe(const gi::dvec3& pos, int face, int samples, std::vector<std::vector<double>>& out, int levels = 1,
                             const std::vector<int>* log2Exponents = nullptr, uint32_t streamBase = 0)
    {
        if (!ready()) return false;
        gi_cubemap_params p;
        gi_cubemap_default_params(&p);
        p.face = face; p.n_samples = samples; p.levels = levels; p.stream_base = streamBase; p.seed = seed;
        for (size_t l = 0; log2Exponents && l < log2Exponents->size() && l < (size_t)GI_CUBEMAP_MAX_LEVELS; l++) p.log2_exponent[l] = (*log2Exponents)[l];
        const int64_t texels = gi_cubemap_chain_texels(face, levels);
        const double P[3] = {pos.x, pos.y, pos.z};
        std::vector<double> buf((size_t)(texels > 0 ? texels : 0) * 3 + 1);
        if (check(gi_cubemap_host(_st->ctx, P, &p, buf.data(), 1)) != 0) return false;
        out.clear();
        size_t at = 0;
        for (int l = 0; l < levels; l++) {
            const size_t n = (size_t)(face >> l), count = 6 * n * n * 3;
            out.emplace_back(buf.begin() + at, buf.begin() + at + count);
            at += count;
        }
        return true;
    }
    // bakeLightmap (gi_lightmap_host): the chart -- ent [n] triangle entities of the uploaded scene, uv [n][3][2] their chart coordinates, v growing
    // with the row -- rasterised into width x height texels, the covered ones baked as bakeTexels does, put back into the image and dilated `dilate`
    // times.  atlas gets [height][width][3]; owner (optional) [height][width], the chart row of a covered texel or -1; nCovered (optional) their number.
    bool bakeLightmap(const std::vector<int32_t>& ent, const std::vector<double>& uv, int width, int height, int samples, std::vector<double>& atlas,
                      int dilate = 2, bool flip = false, uint32_t streamBase = 0, std::vector<int32_t>* owner = nullptr, int* nCovered = nullptr)
    {
        if (!ready()) return false;
        if (uv.size() != ent.size() * 6 || ent.size() > 0x7fffffffu) { _st->err = "bakeLightmap: uv must hold three coordinate pairs per chart row"; return false; }
        gi_lightmap_params p;
        gi_lightmap_default_params(&p);
        p.width = width; p.height = height; p.n_samples = samples; p.dilate = dilate; p.flip = flip ? 1 : 0; p.stream_base = streamBase; p.seed = seed;
        const size_t T = width > 0 && height > 0 && width <= 8192 && height <= 8192 ? (size_t)width * (size_t)height : 0;
        std::vector<double> buf(T * 3 + 1);
        std::vector<int32_t> own(T + 1);
        int32_t n = 0;
        if (check(gi_lightmap_host(_st->ctx, &p, (int32_t)ent.size(), ent.data(), uv.data(), buf.data(), 1, owner ? own.data() : nullptr, &n)) != 0) return false;
        atlas.assign(buf.begin(), buf.begin() + T * 3);
        if (owner) owner->assign(own.begin(), own.begin() + T);
        if (nCovered) *nCovered = n;
        return true;
    }

    // ---- ADDITION (the reference has no denoiser): the edge-avoiding a-trous filter of gi_denoise_host (include/gi_hip.h states the formula) on a
    // whole frame.  color = [height][width][3] linear radiance of a feat.width x feat.height frame, feat = what renderFeatures filled; out gets
    // [height][width][3].  dp = nullptr: gi_denoise_default_params; else its width / height are overwritten with feat's.  Needs a device, not a
    // scene.  false with last_error() set when it cannot run (out is then left alone).
    bool denoise(const std::vector<double>& color, const Features& feat, std::vector<double>& out, const gi_denoise_params* dp = nullptr)
    {
        if (!ensure_context()) return false;
        gi_denoise_params p;
        if (dp) p = *dp; else gi_denoise_default_params(&p);
        p.width = feat.width; p.height = feat.height;
        const size_t npix = (size_t)(feat.width > 0 ? feat.width : 0) * (size_t)(feat.height > 0 ? feat.height : 0);
        if (color.size() != npix * 3 || feat.albedo.size() != npix * 3 || feat.normal.size() != npix * 3 || feat.depth.size() != npix || feat.coverage.size() != npix) {
            _st->err = "denoise: colour and feature buffers do not have the size of a " + std::to_string(feat.width) + " x " + std::to_string(feat.height) + " frame";
            return false;
        }
        std::vector<double> buf(npix * 8 + 8), res(npix * 3 + 3);
        for (size_t i = 0; i < npix; i++) {
            for (int k = 0; k < 3; k++) { buf[i * 8 + k] = feat.albedo[i * 3 + k]; buf[i * 8 + 3 + k] = feat.normal[i * 3 + k]; }
            buf[i * 8 + 6] = feat.depth[i]; buf[i * 8 + 7] = feat.coverage[i];
        }
        if (check(gi_denoise_host(_st->ctx, &p, color.data(), 1, buf.data(), 1, res.data(), 1)) != 0) return false;
        res.resize(npix * 3);
        out.swap(res);
        return true;
    }

    // ---- ADDITION (the reference has no upsampler): the guided upsampler of gi_upsample_host (include/gi_hip.h states the formula).  low_color =
    // [low.height][low.width][3] linear radiance of the reduced-size frame, low and full = what renderFeatures filled at the two sizes, with
    // low.width = ceil(full.width / factor) and low.height likewise; out gets [full.height][full.width][3].  up = nullptr:
    // gi_upsample_default_params; else its sizes and factor are overwritten.  Needs a device, not a scene.  false with last_error() set when it
    // cannot run (out is then left alone).
    bool upsample(const std::vector<double>& low_color, const Features& low, const Features& full, int factor, std::vector<double>& out, const gi_upsample_params* up = nullptr)
    {
        if (!ensure_context()) return false;
        gi_upsample_params p;
        if (up) p = *up; else gi_upsample_default_params(&p);
        p.width = full.width; p.height = full.height; p.low_width = low.width; p.low_height = low.height; p.factor = factor;
        const size_t nlow = feature_pixels(low), npix = feature_pixels(full);
        std::vector<double> lbuf, fbuf;
        if (low_color.size() != nlow * 3 || !pack_features(low, lbuf) || !pack_features(full, fbuf)) {
            _st->err = "upsample: colour and feature buffers do not have the sizes of a " + std::to_string(low.width) + " x " + std::to_string(low.height) + " and a " +
                       std::to_string(full.width) + " x " + std::to_string(full.height) + " frame";
            return false;
        }
        std::vector<double> res(npix * 3 + 3);
        if (check(gi_upsample_host(_st->ctx, &p, low_color.data(), 1, lbuf.data(), 1, fbuf.data(), 1, res.data(), 1)) != 0) return false;
        res.resize(npix * 3);
        out.swap(res);
        return true;
    }
    static size_t feature_pixels(const Features& f) { return (size_t)(f.width > 0 ? f.width : 0) * (size_t)(f.height > 0 ? f.height : 0); }
    // the [height][width][8] records of gi_hip.h from the separate buffers (8 more, so that an empty frame still has an address to refuse);
    // false when a buffer does not have the frame's size
    static bool pack_features(const Features& f, std::vector<double>& buf)
    {
        const size_t npix = feature_pixels(f);
        if (f.albedo.size() != npix * 3 || f.normal.size() != npix * 3 || f.depth.size() != npix || f.coverage.size() != npix) return false;
        buf.assign(npix * 8 + 8, 0.0);
        for (size_t i = 0; i < npix; i++) {
            for (int k = 0; k < 3; k++) { buf[i * 8 + k] = f.albedo[i * 3 + k]; buf[i * 8 + 3 + k] = f.normal[i * 3 + k]; }
            buf[i * 8 + 6] = f.depth[i]; buf[i * 8 + 7] = f.coverage[i];
        }
        return true;
    }

    // ---- single-vertex pieces of radiance(), include/raytracer.h:321-379,481-506,509-529: the kernels' per-lane functions on the host
    uint32_t rng_stream = 0, rng_depth = 0;   // key of the counter RNG for the draws these three make (the reference calls drand())
    int rayType(const Entity* entity, const Ray& ray, gi::dvec3& norm, gi::dvec2& minUV)
    {
        const gi::Mat m = mat_of(entity);
        gi::dvec2 uv = minUV;
        return gi::ray_type(m, entity->material.diffuse->getAlpha(uv), gi::to_lane_ray(ray), gi::to_v3(norm), lane_rng());
    }
    void secondaryRay(const Ray& ray, const Entity* current, gi::dvec3& norm, gi::dvec2& UV, double sx, double sy, gi::dvec3& refDir, gi::dvec3& f, double& roughness,
                      gi::dvec3& contrib, double& offset)
    {
        const gi::Mat m = mat_of(current);
        gi::V3 n = gi::to_v3(norm), rd, ff, cb = gi::to_v3(contrib);
        gi::secondary_ray(gi::to_lane_ray(ray), m, gi::to_v3(current->material.diffuse->get(UV)), current->material.diffuse->getAlpha(UV), n, sx, sy, rd, ff, roughness, cb, offset, lane_rng());
        norm = gi::from_v3(n); refDir = gi::from_v3(rd); f = gi::from_v3(ff); contrib = gi::from_v3(cb);
    }
    bool raymarch(const Ray& r, gi::dvec3& hit, gi::dvec3& col, double mint, double maxt)
    {
        if (!_scene) return false;
        std::vector<gi::FogD> fogs;
        std::vector<double> grid;
        for (AtmosphereEntity* a : _scene->at)
            if (HeightFog* hf = dynamic_cast<HeightFog*>(a)) {
                gi::FogD fd;
                memset(&fd, 0, sizeof fd);
                gi::put3(fd.pos, hf->pos); gi::put3(fd.size, hf->s); gi::put3(fd.col, hf->col);
                fd.d = hf->d; fd.sc = hf->sc;
                gi::put3(fd.bmin, hf->bbox.min); gi::put3(fd.bmax, hf->bbox.max);
                fd.grid_off = (int32_t)grid.size(); fd.grid_n = (int32_t)hf->noiseGrid.size();
                grid.insert(grid.end(), hf->noiseGrid.begin(), hf->noiseGrid.end());
                fogs.push_back(fd);
            }
        gi::Scene S{};
        S.fogs = fogs.data(); S.fog_grid = grid.data(); S.n_fog = (int32_t)fogs.size();
        gi::V3 h, c;
        if (!gi::raymarch(S, gi::to_lane_ray(r), h, c, mint, maxt, lane_rng(), gi::P_FOG_CAMERA)) return false;
        hit = gi::from_v3(h); col = gi::from_v3(c);
        return true;
    }

    bool running() const { return _running; }
    void stop() { _running = false; _cancel = 1; }
    void start() { _running = true; _cancel = 0; }

    int photons = 75000;
    int photon_depth = 5;
    int min_samples = 8;
    int max_samples = 32;
    double noise_thresh = 0.0015;
    gi::dvec3 ambient = gi::dvec3(0, 0, 0);
    uint64_t seed = 0x9E3779B97F4A7C15ull;   // counter-RNG seed (the reference seeds drand() with time(0))
    int progressive_rows = 16;                // rows of the first displayed stripe of run(); 0 = the whole frame in one call
    double progressive_ms = 50;               // stripes double while a step takes less than this many ms; 0 = every stripe progressive_rows high
    volatile int rows_in_flight = 0;          // rows of the step being rendered (they are painted when it ends)
    std::vector<int32_t> devices;             // HIP device ordinals to render on; empty = every visible GPU (the frame's stripes are dealt round-robin)
    volatile int rows_done = 0;               // rows of the current frame already in the Image
    int photons_on_device = 0;                // photons stored by the last on-device emission of run()

    std::shared_ptr<Image> getImage() const { return _image; }
    const std::vector<float>& linear() const { return _linear; }   // float tap of the frame (pre-gamma)
    const std::string& last_error() const { return _st->err; }
    PhotonMap* photonMap() const { return _st->photon_map.get(); }
    Camera _camera;

  private:
    struct State {
        gi_ctx* ctx = nullptr;        // the context of the per-ray methods and of photon emission; member 0 of the group when there is one
        gi_group* group = nullptr;    // every visible GPU, when there is more than one (or `devices` says so)
        std::shared_ptr<PhotonMap> photon_map;
        bool uploaded = false, photons_uploaded = false, fresh_map = true;
        std::string err;
        ~State() { if (group) gi_group_destroy(group); else if (ctx) gi_destroy(ctx); }
    };
    bool ensure_context()
    {
        if (_st->ctx) return true;
        const int want = devices.empty() ? gi_device_count() : (int)devices.size();
        int rc;
        if (want > 1) {
            rc = gi_group_create(&_st->group, (int32_t)devices.size(), devices.empty() ? nullptr : devices.data());
            if (rc == 0) _st->ctx = gi_group_ctx(_st->group, 0);
        } else
            rc = gi_create(&_st->ctx, devices.empty() ? 0 : devices[0]);
        if (rc != 0) { _st->err = "gi_create failed: no usable HIP device (this renderer has no CPU fallback)"; fprintf(stderr, "%s\n", _st->err.c_str()); return false; }
        return true;
    }
    bool ready()
    {
        if (!ensure_context() || !_scene) return false;
        if (!_scene->valid) { _scene->rebuild(); _st->uploaded = false; }
        return upload_scene();
    }
    // scene tables and photon map on the device; photons are emitted once per scene (the reference keeps a valid map across frames)
    bool prepare()
    {
        if (!ready()) return false;
        return photons_ready();
    }
    bool photons_ready()
    {
        PhotonMap* pm = _st->photon_map.get();
        if (!pm) return true;
        if (!pm->valid) {
            if (pm->size() == 0) {
                // nothing pushed by a caller: RayTracer::run's tracePhotons + rebuild (include/raytracer.h:61-72) entirely on the device(s) --
                // emission, octree, candidate ranges; the photons never visit the host (every device emits the same keyed set)
                const double box[6] = {pm->_root._bbox.min.x, pm->_root._bbox.min.y, pm->_root._bbox.min.z, pm->_root._bbox.max.x, pm->_root._bbox.max.y, pm->_root._bbox.max.z};
                const int members = _st->group ? gi_group_size(_st->group) : 1;
                for (int i = 0; i < members; i++) {
                    gi_ctx* cx = _st->group ? gi_group_ctx(_st->group, i) : _st->ctx;
                    const int n = gi_trace_photons(cx, _scene->lights.empty() ? 0 : photons, 5, seed, box, nullptr);
                    if (n < 0) { _st->err = gi_last_error(cx); fprintf(stderr, "gi: %s\n", _st->err.c_str()); return false; }
                    photons_on_device = n;
                }
                pm->valid = true;
                _st->photons_uploaded = true;
                return true;
            }
            pm->rebuild();
            _st->photons_uploaded = false;
        }
        if (!_st->photons_uploaded) {
            gi_photon_map_desc pd;
            gih_get_photon_desc(pm->handle(), &pd);
            if (check(_st->group ? gi_group_upload_photons(_st->group, &pd) : gi_upload_photons(_st->ctx, &pd)) != 0) return false;
            _st->photons_uploaded = true;
        }
        return true;
    }
    bool upload_scene()
    {
        if (_st->uploaded) return true;
        const double amb[3] = {ambient.x, ambient.y, ambient.z};
        gih_set_ambient(_scene->handle(), amb);
        gi_scene_desc d;
        if (gih_get_scene_desc(_scene->handle(), &d) != 0) { _st->err = "scene octree not built"; return false; }
        if (check(_st->group ? gi_group_upload_scene(_st->group, &d) : gi_upload_scene(_st->ctx, &d)) != 0) return false;
        _st->uploaded = true;
        if (_st->fresh_map) { if (_st->group) gi_group_clear_photons(_st->group); else gi_clear_photons(_st->ctx); _st->fresh_map = false; }   // setScene: a fresh PhotonMap; an edited scene keeps its map
        return true;
    }
    int check(int rc)
    {
        if (rc < 0 && rc != GI_E_CANCELLED) {
            _st->err = gi_last_error(_st->ctx);
            if (_st->err.empty() && _st->group) _st->err = gi_group_last_error(_st->group);
            fprintf(stderr, "gi: %s\n", _st->err.c_str());
        }
        return rc < 0 ? rc : 0;
    }
    gi_render_params params(int w, int h) const
    {
        gi_render_params rp;
        const gi::dvec3 *v[3] = {&_camera.pos, &_camera.up, &_camera.forward};
        double* dst[3] = {rp.cam_pos, rp.cam_up, rp.cam_forward};
        for (int k = 0; k < 3; k++) { dst[k][0] = v[k]->x; dst[k][1] = v[k]->y; dst[k][2] = v[k]->z; }
        rp.sensor_diag = _camera.sensorDiag; rp.focal_dist = _camera.focalDist;
        rp.width = w; rp.height = h;
        rp.stripe_h = h; rp.stripe_rank = 0; rp.stripe_world = 1;
        rp.min_samples = min_samples; rp.max_samples = max_samples; rp.noise_thresh = noise_thresh;
        rp.seed = seed;
        return rp;
    }
    bool bake(int mode, const std::vector<double>& rows, size_t row, size_t terms, int samples, uint32_t streamBase, std::vector<double>& out)
    {
        if (!ready()) return false;
        if (rows.size() % row != 0 || rows.size() / row > 0x7fffffffu) { _st->err = "bake: the points are not rows of " + std::to_string(row) + " numbers"; return false; }
        gi_bake_params p;
        gi_bake_default_params(&p);
        p.mode = mode; p.n_samples = samples; p.stream_base = streamBase; p.seed = seed;
        const size_t n = rows.size() / row;
        std::vector<double> buf(n * terms + 1);
        if (check(gi_bake_host(_st->ctx, rows.data(), (int32_t)n, &p, buf.data(), 1)) != 0) return false;
        out.assign(buf.begin(), buf.begin() + n * terms);
        return true;
    }
    static gi::Mat mat_of(const Entity* e)
    {
        gi::Mat m;
        memset(&m, 0, sizeof m);
        m.roughness = e->material.roughness; m.opacity = e->material.opacity; m.ior = e->material.IOR;
        m.dtex = -1; m.etex = -1;
        return m;
    }
    gi::Rng lane_rng() const { gi::Rng r = gi::rng_make(seed, rng_stream); r.depth = rng_depth; return r; }

    volatile bool _running = false;
    volatile int _cancel = 0;
    Octree* _scene = nullptr;
    std::shared_ptr<State> _st;
    std::shared_ptr<Image> _image;
    std::vector<float> _linear;
};
