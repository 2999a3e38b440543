"""The thin lens (gi_set_lens; include/gi_hip.h states the definition) restated in numpy, bit for bit: the primary ray of the sample with Halton
index idx under a lens, from the oracle's Halton sampler and counter RNG (gio_halton_sample, gio_halton_scale, gio_counter_rand) and the vertices
gi_lens_vertices computes on the host.  Shared by the CPU tests, the stand-alone host program's test and the GPU tests.

Everything here is IEEE double arithmetic in the order the header gives (numpy never contracts a multiply and an add), so `rays` must equal the
device's and the host build's primary_ray_at in every bit."""
import ctypes as C

import numpy as np

import oracle_lib as ol

P_LENS_U, P_LENS_V = 34, 35
DEFAULT_SEED = ol.DEFAULT_SEED


def camera(rt_or_dict):
    """cam_pos, cam_up, cam_forward, sensor_diag, focal_dist of a RayTracer (or a dict with those keys) as a dict of float64 values."""
    g = (lambda k: rt_or_dict[k]) if isinstance(rt_or_dict, dict) else (lambda k: getattr(rt_or_dict, k))
    return {"cam_pos": np.array(g("cam_pos"), np.float64), "cam_up": np.array(g("cam_up"), np.float64), "cam_forward": np.array(g("cam_forward"), np.float64),
            "sensor_diag": float(g("sensor_diag")), "focal_dist": float(g("focal_dist"))}


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def normalize(v):
    """glm::normalize as gi_math.h writes it: v * (1 / sqrt(dot(v, v)))."""
    return v * (1.0 / np.sqrt(dot(v, v)))[..., None]


def cross(x, y):
    return np.stack([x[..., 1] * y[..., 2] - y[..., 1] * x[..., 2], x[..., 2] * y[..., 0] - y[..., 2] * x[..., 0], x[..., 0] * y[..., 1] - y[..., 0] * x[..., 1]], -1)


def frame(cam, w, h):
    """make_frame (gi_layout.h): the sensor's size, centre and `right`."""
    sw = (cam["sensor_diag"] * w) / np.sqrt(float(w) * w + h * h)
    sh = sw * (float(h) / w)
    return {"sw": sw, "sh": sh, "center": cam["cam_pos"] + cam["focal_dist"] * cam["cam_forward"], "right": normalize(cross(cam["cam_forward"], cam["cam_up"])),
            "w": w, "h": h}


def halton_index(w, h, s, x, y):
    return int(ol.lib().gio_halton_index(w, h, int(s), int(x), int(y)))


def frame_indices(w, h, s):
    """Halton indices of sample s of every pixel, row-major [h * w]."""
    return np.array([halton_index(w, h, s, x, y) for y in range(h) for x in range(w)], np.uint32)


def pixel_offsets(w, h, idx):
    """(dx, dy) [n] of primary_ray_at: the two Halton numbers scaled to pixels in float, widened."""
    L = ol.lib()
    dx = np.array([L.gio_halton_scale(w, h, 0, L.gio_halton_sample(0, int(i))) for i in idx], np.float64)
    dy = np.array([L.gio_halton_scale(w, h, 1, L.gio_halton_sample(1, int(i))) for i in idx], np.float64)
    return dx, dy


def pixel_pos(cam, w, h, dx, dy):
    """pixelPos [n][3] for pixel offsets dx, dy [n]: the point of the sensor plane the ray goes through (pinhole and lens alike)."""
    F = frame(cam, w, h)
    a = (F["sw"] * (dx / w - .5))[:, None] * F["right"][None, :]
    b = (F["sh"] * (dy / h - .5))[:, None] * cam["cam_up"][None, :]
    return (F["center"][None, :] + a) - b


def draws(idx, seed=DEFAULT_SEED):
    """u0, u1 [n]: the f64 draws (seed, stream idx, depth 0, purpose 34 / 35, a = 0, b = 0)."""
    L = ol.lib()
    u0 = np.array([L.gio_counter_rand(C.c_uint64(seed), int(i), 0, P_LENS_U, 0, 0) for i in idx], np.float64)
    u1 = np.array([L.gio_counter_rand(C.c_uint64(seed), int(i), 0, P_LENS_V, 0, 0) for i in idx], np.float64)
    return u0, u1


def lens_points(verts, u0, u1):
    """(l [n][2], k [n]) on the unit polygon `verts` [B + 1][2]: k = min((int)(u0 B), B - 1), f = u0 B - k, r = sqrt(f), l = r ((1 - u1) v_k + u1 v_k+1)."""
    B = len(verts) - 1
    ub = u0 * float(B)
    k = np.minimum(ub.astype(np.int64), B - 1)
    r = np.sqrt(ub - k.astype(np.float64))
    l = r[:, None] * ((1.0 - u1)[:, None] * verts[k] + u1[:, None] * verts[k + 1])
    return l, k


def eyes(cam, w, h, verts, radius, idx, seed=DEFAULT_SEED):
    """eyePos [n][3] = (cam_pos + (radius l.x) right) + (radius l.y) cam_up, and (l, k)."""
    F = frame(cam, w, h)
    l, k = lens_points(verts, *draws(idx, seed))
    e = (cam["cam_pos"][None, :] + (radius * l[:, 0])[:, None] * F["right"][None, :]) + (radius * l[:, 1])[:, None] * cam["cam_up"][None, :]
    return e, l, k


def rays(cam, w, h, idx, radius=0.0, verts=None, seed=DEFAULT_SEED):
    """primary_ray_at for Halton indices idx of a w x h frame: [n][6] = origin, direction.  radius 0: the pinhole (no draw, the eye is cam_pos);
    else verts = gi_lens_vertices' table.  The direction is normalised twice, as make_ray(eye, normalize(pixelPos - eye)) does."""
    idx = np.asarray(idx, np.uint32).reshape(-1)
    pp = pixel_pos(cam, w, h, *pixel_offsets(w, h, idx))
    if radius > 0:
        eye = eyes(cam, w, h, verts, radius, idx, seed)[0]
    else:
        eye = np.repeat(cam["cam_pos"][None, :], len(idx), 0)
    d = normalize(normalize(pp - eye))
    return np.concatenate([eye, d], 1)


def pinhole_centre_ray(cam, w, h, x, y):
    """The pinhole ray through the centre of pixel (x, y): gi_focus_distance's."""
    pp = pixel_pos(cam, w, h, np.array([x + .5]), np.array([y + .5]))
    eye = cam["cam_pos"][None, :]
    return np.concatenate([eye, normalize(normalize(pp - eye))], 1)


def fold(samples):
    """pixel_add_sample's running mean over samples [n][npix][3] in order: colour = L for s = 0, else (s colour + L) (1 / (s + 1))."""
    c = None
    for s, L in enumerate(samples):
        c = L.copy() if s == 0 else (1.0 * s * c + L) * (1.0 / (s + 1))
    return c


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
