"""Parameter blocks built and validated before the library is called: the Halton cap, the upsampler's sizes and arrays, gi_occlusion_params, gi_lens, gi_baked_params, gi_baked_lightmap_params, gi_baked_visibility_params, gi_baked_reflections_params, gi_final_gather_params."""
import ctypes as C

import numpy as np

from ._abi import (BAKED_DIFFUSE, BAKED_DIRECT, BAKED_EMISSIVE, BAKED_SPECULAR, CUBEMAP_MAX_LEVELS, GI_OK, LM_FILTERS, PROBE_VISIBILITY_MAX_SIZE, REFLECTIONS_MAX_PROBES, BakedLightmapParams,
                   BakedParams, BakedReflectionsParams, BakedVisibilityParams, FinalGatherParams, Lens, OcclusionParams, _f64, _floats, _p, lib)


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


BAKED_TERMS = BAKED_DIRECT | BAKED_DIFFUSE | BAKED_SPECULAR | BAKED_EMISSIVE


def baked_params(n=None, sh=None, grid_box=None, chain=None, exponents=None, terms=None, width=None, height=None, lightmap=False):
    """(gi_baked_params, sh, chain) of RayTracer.run_baked: the library's defaults with n samples; sh [nz][ny][nx][9][3] the probe grid (bake_probes
    on probe_grid(grid_box, nx, ny, nz), reshaped) with its box grid_box = (min xyz, max xyz); chain a reflection probe's levels
    [6][face >> l][face >> l][3] (the list bake_reflection_probe returns, or one array for a single level) filtered with `exponents` (indexed by level,
    entry 0 ignored; default: the library's); terms a set of BAKED_* bits, default: DIRECT | EMISSIVE plus DIFFUSE with sh and SPECULAR with chain.
    The arrays come back contiguous float64, the chain concatenated [texels][3]; None where not given.  No device needed.  ValueError for what the
    library would refuse and for shapes that do not fit.  lightmap: the block of run_baked_lightmap, whose atlas serves the diffuse term -- DIFFUSE
    is a default term and needs no sh."""
    p = BakedParams()
    lib().gi_baked_default_params(C.byref(p))
    if n is not None:
        p.n_samples = _whole("n", n, "baked")
    if p.n_samples < 1:
        raise ValueError(f"baked: n must be at least 1, got {p.n_samples}")
    if width is not None and height is not None and p.n_samples > halton_sample_cap(width, height):
        raise ValueError(f"baked: n = {p.n_samples} takes the Halton index of a {width} x {height} frame beyond 32 bits (at most {halton_sample_cap(width, height)})")
    if sh is not None:
        sh = _f64(sh)
        if sh.ndim != 5 or sh.shape[3:] != (9, 3) or min(sh.shape[:3]) < 1:
            raise ValueError(f"baked: sh [nz][ny][nx][9][3] expected, got {sh.shape}")
        if grid_box is None:
            raise ValueError("baked: a probe grid needs its box, grid_box = (min xyz, max xyz)")
        box = _f64(grid_box).reshape(-1)
        if box.shape != (6,) or not np.isfinite(box).all() or not (box[3:] > box[:3]).all():
            raise ValueError(f"baked: grid_box must be six finite numbers with max > min on every axis, got {box.tolist()}")
        p.nz, p.ny, p.nx = sh.shape[:3]
        p.grid_min[:], p.grid_max[:] = box[:3].tolist(), box[3:].tolist()
    elif grid_box is not None:
        raise ValueError("baked: grid_box without sh")
    if chain is not None:
        levels = [_f64(chain)] if isinstance(chain, np.ndarray) else [_f64(c) for c in chain]
        face = levels[0].shape[1] if levels and levels[0].ndim == 4 else 0
        if not 1 <= len(levels) <= CUBEMAP_MAX_LEVELS or face < 1 or face % (1 << (len(levels) - 1)):
            raise ValueError(f"baked: chain must be 1 .. {CUBEMAP_MAX_LEVELS} levels whose first face is divisible by 2^(levels - 1)")
        for l, c in enumerate(levels):
            if c.shape != (6, face >> l, face >> l, 3):
                raise ValueError(f"baked: level {l} of a chain of face {face} is [6][{face >> l}][{face >> l}][3], got {c.shape}")
        p.face, p.levels = face, len(levels)
        for l, e in enumerate(exponents if exponents is not None else ()):
            if l >= CUBEMAP_MAX_LEVELS:
                raise ValueError(f"baked: at most {CUBEMAP_MAX_LEVELS} exponents, got {len(exponents)}")
            p.log2_exponent[l] = _whole(f"exponents[{l}]", e, "baked")
        if any(not 0 <= p.log2_exponent[l] <= 16 for l in range(1, p.levels)):
            raise ValueError(f"baked: exponents must be 0 .. 16, got {list(p.log2_exponent)[:p.levels]}")
        chain = np.ascontiguousarray(np.concatenate([c.reshape(-1, 3) for c in levels]))
    elif exponents is not None:
        raise ValueError("baked: exponents without chain")
    if terms is None:
        terms = BAKED_DIRECT | BAKED_EMISSIVE | (BAKED_DIFFUSE if sh is not None or lightmap else 0) | (BAKED_SPECULAR if chain is not None else 0)
    p.terms = _whole("terms", terms, "baked")
    if p.terms == 0 or p.terms & ~BAKED_TERMS:
        raise ValueError(f"baked: terms must be a non-empty set of the BAKED_* bits, got {p.terms}")
    if (p.terms & BAKED_DIFFUSE and sh is None and not lightmap) or (p.terms & BAKED_SPECULAR and chain is None):
        raise ValueError("baked: the diffuse term needs sh, the specular term needs chain")
    return p, sh, chain


FINAL_GATHER_MAX_DIRS = 64


def final_gather_params(n=None, dirs=None, sh=None, grid_box=None, chain=None, exponents=None, terms=None, width=None, height=None):
    """(gi_final_gather_params, sh, chain) of RayTracer.run_final_gather: baked_params on the same arguments inside the library's defaults (16
    directions), with dirs set when given.  terms defaults as in baked_params: DIRECT | EMISSIVE, DIFFUSE with sh, SPECULAR with chain; a chain
    without the SPECULAR bit is kept for the secondary hits.  No device needed.  ValueError for what the library would refuse: everything
    baked_params refuses, dirs outside 1 .. 64."""
    p = FinalGatherParams()
    lib().gi_final_gather_default_params(C.byref(p))
    bp, sh, chain = baked_params(n=n, sh=sh, grid_box=grid_box, chain=chain, exponents=exponents, terms=terms, width=width, height=height)
    p.baked = bp
    if dirs is not None:
        p.n_dirs = _whole("dirs", dirs, "final_gather")
    if not 1 <= p.n_dirs <= FINAL_GATHER_MAX_DIRS:
        raise ValueError(f"final_gather: dirs must be 1 .. {FINAL_GATHER_MAX_DIRS}, got {p.n_dirs}")
    return p, sh, chain


def baked_lightmap_params(atlas, ent, uv, filter="bilinear"):
    """(gi_baked_lightmap_params, atlas, ent, uv) of RayTracer.run_baked_lightmap: atlas [height][width][3] as bake_lightmap returns it (float32
    stays, anything else becomes float64), the chart ent [n] and uv [n][3][2] it was baked for, filter "bilinear" / "nearest" or LM_BILINEAR /
    LM_NEAREST.  The arrays come back contiguous.  No device needed.  ValueError for what the library would refuse without looking at the scene
    and for shapes that do not fit."""
    p = BakedLightmapParams()
    lib().gi_baked_lightmap_default_params(C.byref(p))
    a = _floats(atlas)
    if a.ndim != 3 or a.shape[2] != 3 or not (1 <= a.shape[0] <= 8192 and 1 <= a.shape[1] <= 8192):
        raise ValueError(f"baked_lightmap: atlas [height][width][3] with height and width 1 .. 8192 expected, got {a.shape}")
    if isinstance(filter, str):
        if filter not in LM_FILTERS:
            raise ValueError(f"baked_lightmap: filter must be one of {sorted(LM_FILTERS)}, got {filter!r}")
        filter = LM_FILTERS[filter]
    p.filter = _whole("filter", filter, "baked_lightmap")
    if p.filter not in LM_FILTERS.values():
        raise ValueError(f"baked_lightmap: filter must be LM_NEAREST or LM_BILINEAR, got {p.filter}")
    try:
        e, c = _chart(ent, uv)
    except ValueError as err:
        raise ValueError(f"baked_lightmap: {err}") from None
    if not np.isfinite(c).all():
        raise ValueError("baked_lightmap: the chart has a non-finite coordinate")
    p.height, p.width, p.n_chart = a.shape[0], a.shape[1], len(e)
    return p, a, e, c


def baked_visibility_params(vis, grid=None, normal_bias=None, vis_floor=None):
    """(gi_baked_visibility_params, vis) of RayTracer.run_baked_visibility: vis [nz][ny][nx][M][M][2] the probes' maps (bake_probe_visibility on
    the grid's points, reshaped; float32 stays, anything else becomes float64), or None for no maps; grid = (nz, ny, nx) of the probe grid the maps
    must fit; normal_bias and vis_floor default to the library's 0.0 and 0.05.  The array comes back contiguous.  No device needed.  ValueError for
    what the library would refuse and for shapes that do not fit."""
    p = BakedVisibilityParams()
    lib().gi_baked_visibility_default_params(C.byref(p))
    if normal_bias is not None:
        p.normal_bias = float(normal_bias)
    if vis_floor is not None:
        p.vis_floor = float(vis_floor)
    if not (0.0 <= p.normal_bias < float("inf")):
        raise ValueError(f"baked_visibility: normal_bias must be finite and >= 0, got {p.normal_bias}")
    if not (0.0 < p.vis_floor <= 1.0):
        raise ValueError(f"baked_visibility: vis_floor must be in (0, 1], got {p.vis_floor}")
    if vis is None:
        return p, None
    v = _floats(vis)
    if v.ndim != 6 or v.shape[5] != 2 or v.shape[3] != v.shape[4] or not 1 <= v.shape[3] <= PROBE_VISIBILITY_MAX_SIZE or min(v.shape[:3]) < 1:
        raise ValueError(f"baked_visibility: vis [nz][ny][nx][M][M][2] with M 1 .. {PROBE_VISIBILITY_MAX_SIZE} expected, got {v.shape}")
    if grid is not None and tuple(v.shape[:3]) != tuple(int(g) for g in grid):
        raise ValueError(f"baked_visibility: the maps are those of a {v.shape[2]} x {v.shape[1]} x {v.shape[0]} grid, the probes' is {grid[2]} x {grid[1]} x {grid[0]}")
    p.size = v.shape[3]
    return p, v


def baked_reflections_params(probes, chains):
    """(gi_baked_reflections_params, probes, chains, face, levels) of RayTracer.run_baked_reflections: probes [K][10] the set's table, one row per
    probe = pos xyz, box_min xyz, box_max xyz, fade (reflection_probe_cells makes one); chains the K chains of the probes, each the list of levels
    [6][face >> l][face >> l][3] bake_reflection_probe returns (bake_reflection_probes returns them concatenated, [K][texels][3], which is taken
    as it is), all of one face and one number of levels.  probes None or of no rows: no set -- (params with 0 probes, None, None, None, None).
    The arrays come back contiguous float64, the chains as [K][texels][3]; a set given as [K][texels][3] has face and levels None, the caller's
    to state.  No device needed.  ValueError for what the library would refuse and for shapes that do not fit each other."""
    p = BakedReflectionsParams()
    lib().gi_baked_reflections_default_params(C.byref(p))
    if probes is None or len(probes) == 0:
        if chains is not None and len(chains):
            raise ValueError("baked_reflections: chains without probes")
        return p, None, None, None, None
    t = _f64(probes)
    if t.ndim != 2 or t.shape[1] != 10 or not 1 <= t.shape[0] <= REFLECTIONS_MAX_PROBES:
        raise ValueError(f"baked_reflections: probes [K][10] with K 1 .. {REFLECTIONS_MAX_PROBES} expected, got {t.shape}")
    if not np.isfinite(t).all():
        raise ValueError("baked_reflections: a probe has a non-finite position, box or fade")
    if not (t[:, 6:9] > t[:, 3:6]).all():
        raise ValueError("baked_reflections: every probe needs box_max > box_min on every axis")
    if (t[:, 9] < 0).any():
        raise ValueError("baked_reflections: fade must not be negative")
    if chains is None or len(chains) != len(t):
        raise ValueError(f"baked_reflections: {len(t)} probes need {len(t)} chains, got {0 if chains is None else len(chains)}")
    face = levels = None
    if isinstance(chains, np.ndarray) and chains.ndim == 3:
        c = _f64(chains)
        if c.shape[2] != 3 or c.shape[1] < 6:
            raise ValueError(f"baked_reflections: chains [K][texels][3] expected, got {c.shape}")
    else:
        flat = []
        for k, chain in enumerate(chains):
            lv = [_f64(chain)] if isinstance(chain, np.ndarray) else [_f64(q) for q in chain]
            f = lv[0].shape[1] if lv and lv[0].ndim == 4 else 0
            if not 1 <= len(lv) <= CUBEMAP_MAX_LEVELS or f < 1 or f % (1 << (len(lv) - 1)):
                raise ValueError(f"baked_reflections: chain {k} must be 1 .. {CUBEMAP_MAX_LEVELS} levels whose first face is divisible by 2^(levels - 1)")
            if face is None:
                face, levels = f, len(lv)
            if (f, len(lv)) != (face, levels):
                raise ValueError(f"baked_reflections: chain {k} has face {f} and {len(lv)} levels, chain 0 has face {face} and {levels}")
            for l, q in enumerate(lv):
                if q.shape != (6, face >> l, face >> l, 3):
                    raise ValueError(f"baked_reflections: level {l} of chain {k} of face {face} is [6][{face >> l}][{face >> l}][3], got {q.shape}")
            flat.append(np.concatenate([q.reshape(-1, 3) for q in lv]))
        c = np.ascontiguousarray(np.stack(flat))
    p.n_probes = len(t)
    return p, t, c, face, levels


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
