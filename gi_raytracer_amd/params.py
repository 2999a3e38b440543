"""Parameter blocks built and validated before the library is called: the Halton cap, the upsampler's sizes and arrays, gi_occlusion_params, gi_lens."""
import ctypes as C

import numpy as np

from ._abi import GI_OK, Lens, OcclusionParams, _f64, _floats, _p, lib


def halton_sample_cap(w, h):
    """Samples per pixel a w x h frame can take before the Halton index leaves 32 bits: index = offset + s * inc with offset < inc = 2^a 3^b,
    the smallest such powers >= w and >= h (Halton_enum, include/halton_enum.h:69-114)."""
    pw, ph = 1, 1
    while pw < w:
        pw *= 2
    while ph < h:
        ph *= 3
    return (1 << 32) // (pw * ph)


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
    return _floats(a["features"] if isinstance(a, dict) else a)


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


def _number(name, v):
    try:
        return float(v)
    except (TypeError, ValueError):
        raise ValueError(f"lens: {name} must be a number, got {v!r}") from None


def lens_params(radius=None, blades=None, rotation=None):
    """gi_lens_default (radius 0 = the pinhole, 6 blades, rotation 0) with any of radius (scene units), blades, rotation (radians) set.  No device
    needed.  ValueError for what gi_set_lens would refuse: a negative, NaN or infinite radius, blades outside 3 .. 16, a rotation that is not finite."""
    l = Lens()
    lib().gi_lens_default(C.byref(l))
    if radius is not None:
        radius = _number("radius", radius)
        if not (0.0 <= radius < float("inf")):
            raise ValueError(f"lens: radius must be finite and >= 0 (0: the pinhole), got {radius}")
        l.radius = radius
    if blades is not None:
        l.blades = _whole("blades", blades, "lens")
    if rotation is not None:
        rotation = _number("rotation", rotation)
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


def _bake_points(points, normals=None):
    pts = _f64(points).reshape(-1, 3)
    if normals is None:
        return pts
    nrm = _f64(normals).reshape(-1, 3)
    if len(nrm) != len(pts):
        raise ValueError(f"bake: {len(pts)} points and {len(nrm)} normals")
    return np.ascontiguousarray(np.concatenate([pts, nrm], 1))


def _chart(ent, uv):
    e = np.ascontiguousarray(ent, np.int32).reshape(-1)
    c = _f64(uv).reshape(-1, 3, 2)
    if len(c) != len(e):
        raise ValueError(f"lightmap: {len(e)} entities and {len(c)} chart triangles")
    return e, c
