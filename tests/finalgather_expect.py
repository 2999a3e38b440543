"""Expectation of the final-gather pass (gi_render_final_gather_*; include/gi_hip.h states the definition), built from what exists:
baked_expect.sample_hits for the first hits, the oracle's counter RNG (gio_counter_rand) and cosine sampler (gio_hemi_cos_n, power 2, purposes 36
and 37) for the directions d_j as occlusion_expect.directions makes them, Oracle.trace on the rows (O, d_j) for the secondary hits,
features_expect.sample_features for their albedo, Oracle.visible on the light segments at Q, and baked_expect.irradiance, reflect and chain_texel
for the look-ups.  Shared by the GPU tests and the CPU tests.

Every product and sum is written in the header's order, one IEEE operation at a time.  Valid for scenes whose alpha test cannot depend on the
draw (features_expect.DRAW_FREE_SCENES) and whose emission is not textured.

What is exact and what is not.  The first hit, O and the RNG draws are the device's bit for bit.  d_j comes from sin, cos and sqrt of the host's
libm where the device calls OCML's, up to 4 ulp apart (parity_checks.check_kats): Q, and with it the grid's value at Q, move in the last bits, and a
ray that grazes an edge may hit another entity.  The light loop at Q calls acos, sin and cos for the point on the light and pow for a roughness
other than 1.  So the diffuse term is compared within an allowance, measured by tests/test_finalgather_cpu.py and written down here:

  DELTA_DIRS  the largest relative change of a pixel's diffuse term when every component of every d_j moves by +4 or by -4 ulp, against the
              pixel's own value floored at 1e-6 of the frame's largest, over FRAMES below -- the frames of the GPU tests' comparison with this
              statement -- with the materials cycled through the lobes, 2 samples and 1, 4 and 5 directions.  Measured: 1.844e-14 on cornell,
              7.208e-14 on test_scene, 4.167e-14 on spheres_opaque; the constant is the largest, rounded up.
  DELTA_POW   the same with i_Q moved by +4 or -4 ulp instead (pow's share, and the light point's).  Measured: 9.785e-16 on cornell, 0 on
              test_scene, 3.097e-16 on spheres_opaque.
  ALLOWANCE   16 * (DELTA_DIRS + DELTA_POW) = 1.184e-12: the corners of the ulp box under-sample the move, and the trilinear slope amplifies it
              with the ray's length.
test_finalgather_cpu.test_the_oracle_flips_no_gather_ray_and_the_allowance_is_the_measured_one measures both on exactly these frames, prints them
and fails when a scene exceeds a constant.

FRAMES names the frames on which secondary hits and values are compared.  The oracle alone must flip no gather ray on them under a 4-ulp move of
d_j.  test_scene and spheres_opaque flip none at 13x9 and 24x16.  Cornell flips none at 13x9 but 3 at 24x16 -- rays that leave a wall along it
and graze the next -- so its second frame is another size off the 8x8 tile grid with several tiles, 20x14, which flips none (of the sizes tried,
17x11, 19x13 and 20x14 flip none; 18x12, 20x12, 21x15, 22x14, 23x15, 24x17, 25x15, 26x14, 26x18, 27x17, 28x16, 29x19, 30x18 and 32x20 flip 1 to 8)."""
import ctypes as C

import numpy as np

import baked_expect as be
import features_expect as fe
import oracle_lib as ol

SHADOW_BIAS = 0.0001
P_LIGHT_X, P_LIGHT_Y = 2, 3
P_FG_U, P_FG_V = 36, 37
ID_MISS, ID_NONE = -1, -2
DEFAULT_SEED = ol.DEFAULT_SEED
PI = 3.14159265358979323846

DELTA_DIRS = 7.3e-14           # measured 7.208e-14 (test_scene)
DELTA_POW = 1.0e-15            # measured 9.785e-16 (cornell)
ALLOWANCE = 16.0 * (DELTA_DIRS + DELTA_POW)
FRAMES = {"cornell": ((13, 9), (20, 14)), "test_scene": ((13, 9), (24, 16)), "spheres_opaque": ((13, 9), (24, 16))}


def dot3(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def directions(nf, idx, dirs, seed=DEFAULT_SEED):
    """d_j = hemisphereSample_cos(Nf, u, v, 2), u = (float) draw(seed, stream idx, depth 0, purpose 36, a = j), v with purpose 37: [n][dirs][3]."""
    L = ol.lib()
    out = np.zeros((len(nf), dirs, 3))
    d = np.zeros(3)
    for i in range(len(nf)):
        n3 = np.ascontiguousarray(nf[i], np.float64)
        for j in range(dirs):
            u = np.float32(L.gio_counter_rand(C.c_uint64(seed), int(idx[i]), 0, P_FG_U, j, 0))
            v = np.float32(L.gio_counter_rand(C.c_uint64(seed), int(idx[i]), 0, P_FG_V, j, 0))
            L.gio_hemi_cos_n(n3.ctypes.data_as(ol.c_dp), C.c_float(u), C.c_float(v), 2.0, d.ctypes.data_as(ol.c_dp))
            out[i, j] = d
    return out


def moved(a, ulps):
    """Every entry of a moved by `ulps` ulp (of its own size), up for ulps > 0."""
    return a if not ulps else a + ulps * np.spacing(np.abs(a))


def gather_rows(g, dirs, seed=DEFAULT_SEED, tables=None, diffuse_on=True):
    """The gather rays of a sample's first hits g (baked_expect.sample_hits): sel [m] = the pixels that gather (a hit on the diffuse lobe), d
    [m][dirs][3], rows [m * dirs][6] = (O, d_j) as Oracle.trace takes them."""
    rough = tables["mats"][np.where(g["hit"], g["mat"], 0), 0]
    sel = np.flatnonzero(g["hit"] & (be.lobe_of(rough) == 2)) if diffuse_on else np.zeros(0, np.int64)
    O = g["P"][sel] + SHADOW_BIAS * g["Nf"][sel]
    d = directions(g["Nf"][sel], g["idx"][sel], dirs, seed)
    rows = np.concatenate([np.repeat(O[:, None, :], dirs, 1), d], 2).reshape(-1, 6)
    return sel, d, rows


def flips_under_perturbation(oracle, rows, ulps=4):
    """How many rows of Oracle.trace hit another entity (or start or stop hitting) when every component of the direction moves by `ulps` ulp, up
    or down: the room the oracle has on these rays.  Returns (flipped, asked)."""
    if not len(rows):
        return 0, 0
    hit, ent = oracle.trace(rows)[:2]
    base = np.where(hit.astype(bool), ent, ID_MISS)
    flipped = np.zeros(len(rows), bool)
    for sign in (+1.0, -1.0):
        q = rows.copy()
        q[:, 3:6] = moved(q[:, 3:6], sign * ulps)
        h2, e2 = oracle.trace(q)[:2]
        flipped |= np.where(h2.astype(bool), e2, ID_MISS) != base
    return int(flipped.sum()), len(rows)


def direct_at(oracle, tables, Q, norm, rough, idx, depth, seed=DEFAULT_SEED):
    """Step 2's i at the points Q under the turned normals norm (not renormalised) with the stream idx's RNG at `depth` [m]: per light from the
    last down the point drawn on it, the segment asked of Oracle.visible, and the share of the first visible one,
    (col * pow(max(0, dot(norm, normalize(lpos - Q))), 1 / roughness)) * (1 / (pi * |lpos - Q|^2))."""
    L = ol.lib()
    lights = tables["lights"]
    m = len(Q)
    i = np.zeros((m, 3))
    done = np.zeros(m, bool)
    so = Q + SHADOW_BIAS * norm
    uv = np.zeros(3)
    for li in range(len(lights) - 1, -1, -1):
        lpos, col, rad = lights[li, 0:3], lights[li, 3:6], lights[li, 6]
        T = np.zeros((m, 3))
        for k in range(m):
            ry = L.gio_counter_rand(C.c_uint64(seed), int(idx[k]), int(depth[k]), P_LIGHT_Y | (li << 8), 0, 0)
            rx = L.gio_counter_rand(C.c_uint64(seed), int(idx[k]), int(depth[k]), P_LIGHT_X | (li << 8), 0, 0)
            L.gio_unit_vec(rx, ry, uv.ctypes.data_as(ol.c_dp))
            T[k] = lpos + rad * uv
        vis = oracle.visible(np.concatenate([so, T], 1))[0].astype(bool) if m else np.zeros(0, bool)
        v = lpos - Q
        hfrac = 1 / (PI * ((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]))
        with np.errstate(divide="ignore", invalid="ignore"):
            unit = v * (1.0 / np.sqrt(dot3(v, v)))[:, None]
            dd = dot3(norm, unit)
            dd = np.where(dd < 0, 0.0, dd)
            ex = 1.0 / rough
            l = np.where(ex == 1.0, dd, np.where(np.isinf(ex), np.where(dd < 1.0, 0.0, np.where(dd == 1.0, 1.0, np.inf)), np.power(dd, ex)))
        share = (col[None, :] * l[:, None]) * hfrac[:, None]
        take = vis & ~done
        i[take] = share[take]
        done |= vis
    return i


def secondary(oracle, tables, rows, d, idx, depth, sh, box, chain, exponents, seed=DEFAULT_SEED, i_ulps=0):
    """L_j of the gather rays `rows` [r][6] (directions d [r][3], stream idx [r], RNG depth [r]): (L [r][3], ids [r], kind [r]) with kind 0 a miss,
    1 a diffuse-lobe hit inside the grid box, 2 one outside it, 3 a specular hit."""
    r = len(rows)
    L = np.zeros((r, 3))
    L[:] = tables["ambient"]
    kind = np.zeros(r, np.int64)
    if not r:
        return L, np.zeros(0, np.int32), kind
    hit, ent, mat, albedo, normal, _, _ = fe.sample_features(oracle, tables, rows)
    if len(tables["tex_kind"]):
        assert (tables["mat_tex"][:, 1] < 0).all(), "the statement does not look up emission textures"
    res = oracle.trace(rows)[2]
    h = np.flatnonzero(hit)
    N = normal[h]
    dj = d[h]
    norm = np.where((dot3(N, dj) > 0)[:, None], N * -1.0, N)
    with np.errstate(divide="ignore", invalid="ignore"):
        nf = norm * (1.0 / np.sqrt(dot3(norm, norm)))[:, None]
    Q = res[h, 0:3]
    mats = tables["mats"]
    rough, emissive, color = mats[mat[h], 0], mats[mat[h], 6:9], albedo[h]
    i = moved(direct_at(oracle, tables, Q, norm, rough, idx[h], depth[h], seed), i_ulps)
    base = emissive + color * i
    Lh = base.copy()
    lobe = be.lobe_of(rough)
    dsel = lobe == 2
    if dsel.any():
        Lh[dsel] = base[dsel] + color[dsel] * be.irradiance(sh, box, Q[dsel], nf[dsel])
    ssel = ~dsel
    if chain is not None and ssel.any():
        face, levels = chain[0].shape[1], len(chain)
        table = be.level_table(mats[:, 0], levels, exponents)
        level = np.where(lobe[ssel] == 0, 0, table[mat[h][ssel]])
        flat = np.concatenate([c.reshape(-1, 3) for c in chain])
        Lh[ssel] = base[ssel] + color[ssel] * flat[be.chain_texel(be.reflect(dj[ssel], nf[ssel]), level, face, levels)]
    L[h] = Lh
    b = np.asarray(box, np.float64).reshape(6)
    outside = ((Q < b[0:3]) | (Q > b[3:6])).any(1)
    kind[h] = np.where(dsel, np.where(outside, 2, 1), 3)
    return L, np.where(hit, ent, ID_MISS).astype(np.int32), kind


def sample_gather(oracle, tables, g, dirs, sh, box, chain=None, exponents=None, seed=DEFAULT_SEED, d_ulps=0, i_ulps=0, diffuse_on=True):
    """One sample from its first hits g: diffuse [n][3] (color * ((sum of L_j, ascending from +0.0) / dirs), +0.0 where nothing gathers), ids
    [n][dirs] (ID_NONE where nothing gathers), kind [n][dirs] (-1 there), rows [m * dirs][6]."""
    n = len(g["hit"])
    sel, d, rows = gather_rows(g, dirs, seed, tables, diffuse_on)
    if d_ulps:
        rows = rows.copy()
        rows[:, 3:6] = moved(rows[:, 3:6], d_ulps)
    m = len(sel)
    idx = np.repeat(g["idx"][sel], dirs)
    depth = np.tile(1 + np.arange(dirs), m)
    L, ids, kind = secondary(oracle, tables, rows, rows[:, 3:6], idx, depth, sh, box, chain, exponents, seed, i_ulps)
    L = L.reshape(m, dirs, 3)
    acc = np.zeros((m, 3))
    for j in range(dirs):
        acc = acc + L[:, j]
    diffuse = np.zeros((n, 3))
    diffuse[sel] = g["albedo"][sel] * (acc / float(dirs))
    all_ids = np.full((n, dirs), ID_NONE, np.int32)
    all_ids[sel] = ids.reshape(m, dirs)
    all_kind = np.full((n, dirs), -1, np.int64)
    all_kind[sel] = kind.reshape(m, dirs)
    return {"diffuse": diffuse, "ids": all_ids, "kind": all_kind, "rows": rows}


def expected_final_gather(oracle, tables, w, h, n, dirs, sh, box, chain=None, exponents=None, seed=DEFAULT_SEED, d_ulps=0, i_ulps=0, hits=None):
    """The pass's diffuse channel and ids tap on a whole w x h frame: diffuse [h][w][3] (the f64 sums over s in ascending order, divided once by n),
    ids [h][w][n][dirs], kind [h][w][n][dirs], rows = every sample's gather rows.  hits: sample_hits of samples 0 .. n-1 when the caller has them."""
    per, ids, kind, rows = [], [], [], []
    for s in range(n):
        g = hits[s] if hits is not None else be.sample_hits(oracle, tables, w, h, s)
        r = sample_gather(oracle, tables, g, dirs, sh, box, chain, exponents, seed, d_ulps, i_ulps)
        per.append(r["diffuse"]); ids.append(r["ids"]); kind.append(r["kind"]); rows.append(r["rows"])
    return {"diffuse": be.fold(per).reshape(h, w, 3), "ids": np.stack(ids, 1).reshape(h, w, n, dirs), "kind": np.stack(kind, 1).reshape(h, w, n, dirs),
            "rows": rows}


def relative_change(a, b):
    """The largest |a - b| of a pixel's diffuse term over the pixel's own value floored at 1e-6 of the frame's largest."""
    top = float(np.abs(b).max())
    if top == 0.0:
        return 0.0
    return float((np.abs(a - b) / np.maximum(np.abs(b), 1e-6 * top)).max())


# ---- the walk-free functions, one row at a time as tests/cpp/finalgather_lookup.cpp prints them
def lookup(sh, box, chain_levels, level_of_mat, Q, nf, color, emissive, rough, mat, d, i):
    """fg_secondary on rows: L [r][3].  chain_levels: the list of levels, or None."""
    base = emissive + color * i
    L = base.copy()
    lobe = be.lobe_of(rough)
    dsel = lobe == 2
    if dsel.any():
        L[dsel] = base[dsel] + color[dsel] * be.irradiance(sh, box, Q[dsel], nf[dsel])
    ssel = ~dsel
    if chain_levels is not None and ssel.any():
        face, levels = chain_levels[0].shape[1], len(chain_levels)
        level = np.where(lobe[ssel] == 0, 0, np.asarray(level_of_mat)[mat[ssel]])
        flat = np.concatenate([c.reshape(-1, 3) for c in chain_levels])
        with np.errstate(invalid="ignore"):
            R = be.reflect(d[ssel], nf[ssel])
        nan = np.isnan(R).all(1) | (R == 0.0).all(1)                      # all NaN, or 0 / 0: every compare of the texel rule fails: face 0, row 0, column 0 of the level
        texel = np.asarray(be.chain_offsets(face, levels))[level]
        if (~nan).any():
            texel[~nan] = be.chain_texel(R[~nan], level[~nan], face, levels)
        L[ssel] = base[ssel] + color[ssel] * flat[texel]
    return L


def fold_rows(color, L):
    """fg_diffuse: color * ((the sum of L [dirs][3], ascending from +0.0) / dirs)."""
    acc = np.zeros(3)
    for v in L:
        acc = acc + v
    return color * (acc / float(len(L)))
