"""Expectation of the first-hit feature buffers (gi_render_features_*), built from the oracle as it is: Oracle.primary_ray for the rays,
Oracle.trace for the hits, Oracle.tex_eval for texture colours.  Shared by the GPU tests and the oracle-only sanity test.

Valid for scenes whose alpha test cannot depend on the draw (opacity 0 or 1, binary cut-outs): Oracle.trace draws with seed 0 and
stream = ray number, the feature pass with the frame's seed and the Halton index."""
import numpy as np

# scenes of tests/parity_checks.SCN whose alpha test cannot depend on the draw
DRAW_FREE_SCENES = ("test_scene", "cornell", "caustics", "caustics_02", "teapot", "spheres_opaque", "textures_opaque")

ULP = 2.0 ** -52


def read_pfm(path):
    """A PFM file as [h][w][3] (`PF`) or [h][w] (`Pf`), rows top to bottom."""
    with open(path, "rb") as f:
        kind = f.readline().strip()
        w, h = (int(v) for v in f.readline().split())
        scale = float(f.readline())
        ch = {b"PF": 3, b"Pf": 1}[kind]
        a = np.frombuffer(f.read(), "<f4" if scale < 0 else ">f4")
    assert a.size == w * h * ch
    a = a.reshape(h, w, ch)[::-1]
    return a if ch == 3 else a[:, :, 0]


def frame_rows(h, stripe_h, rank, world):
    """Frame rows of a rank, in the order of its local rows (stripes k with k % world == rank)."""
    rows = []
    for k in range(rank, (h + stripe_h - 1) // stripe_h, world):
        rows.extend(range(k * stripe_h, min((k + 1) * stripe_h, h)))
    return rows


def sample_rays(oracle, w, h, s):
    """Primary rays of sample s of every pixel, row-major [h * w][6], and their Halton indices."""
    rays = np.zeros((h * w, 6))
    idx = np.zeros(h * w, np.uint32)
    for y in range(h):
        for x in range(w):
            idx[y * w + x], rays[y * w + x] = oracle.primary_ray(w, h, s, x, y)
    return rays, idx


def sample_features(oracle, tables, rays):
    """Features of one sample per ray: (hit [n] bool, ent [n], mat [n], albedo [n][3], normal [n][3], depth [n], textured [n] bool).
    textured = the albedo went through a checkerboard or image look-up (floor / pow table), not a stored constant."""
    hit, ent, res, _ = oracle.trace(rays)
    hit = hit.astype(bool)
    n = len(rays)
    mat = np.where(hit, tables["tri_mat"][np.where(hit, ent, 0)], -1).astype(np.int32)
    albedo = np.zeros((n, 3))
    textured = np.zeros(n, bool)
    albedo[hit] = tables["mats"][mat[hit], 3:6]
    if len(tables["tex_kind"]):
        dtex = np.where(hit, tables["mat_tex"][np.where(hit, mat, 0), 0], -1)
        for t in np.unique(dtex[dtex >= 0]):
            sel = dtex == t
            albedo[sel] = oracle.tex_eval(int(t), res[sel, 6:8])[:, :3]
            textured[sel] = tables["tex_kind"][t] != 0
    normal = np.where(hit[:, None], res[:, 3:6], 0.0)
    d = res[:, 0:3] - rays[:, 0:3]
    depth = np.where(hit, np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]), 0.0)
    return hit, np.where(hit, ent, -1).astype(np.int32), mat, albedo, normal, depth, textured


def expected_features(oracle, tables, w, h, n):
    """Per pixel the f64 sums over s = 0 .. n-1 in ascending order (a Python loop: np.sum adds pairwise), divided once by n.
    Returns feat [h][w][8], ids [h][w][2] of sample 0, textured [h][w] (some sample's albedo came from a look-up), and the largest
    per-sample magnitudes vmax [h][w][8] the tolerances of depth and textured albedo are taken from."""
    acc = np.zeros((h * w, 8))
    vmax = np.zeros((h * w, 8))
    ids = np.full((h * w, 2), -1, np.int32)
    textured = np.zeros(h * w, bool)
    for s in range(n):
        rays, _ = sample_rays(oracle, w, h, s)
        hit, ent, mat, albedo, normal, depth, tex = sample_features(oracle, tables, rays)
        v = np.concatenate([albedo, normal, depth[:, None], hit.astype(np.float64)[:, None]], 1)
        acc = acc + v
        vmax = np.maximum(vmax, np.abs(v))
        textured |= tex
        if s == 0:
            ids[:, 0], ids[:, 1] = ent, mat
    return (acc / float(n)).reshape(h, w, 8), ids.reshape(h, w, 2), textured.reshape(h, w), vmax.reshape(h, w, 8)


def oracle_is_draw_free(oracle, rays):
    """Oracle.trace twice over the same rays, once more with the rays in reverse order (every ray then draws from another stream):
    identical hit tables mean its alpha draws play no part."""
    a = oracle.trace(rays)
    b = oracle.trace(rays)
    c = oracle.trace(np.ascontiguousarray(rays[::-1]))
    same = all(np.array_equal(a[k], b[k]) for k in range(3))
    return same and all(np.array_equal(a[k], c[k][::-1]) for k in range(3))


def hit_depends_on_draw(oracle, rays, trials=12):
    """Whether the HIT FLAG of some ray depends on the alpha draw: Oracle.trace keys its draws by the ray's place in the batch, so the batch is
    traced `trials` times, rolled by a different amount each time.  (A translucent entity with other geometry behind it everywhere changes which
    entity is hit, never whether something is.)"""
    flags = []
    for k in range(trials):
        hit = oracle.trace(np.roll(rays, k * 37, axis=0))[0]
        flags.append(np.roll(hit, -k * 37))
    flags = np.array(flags)
    return bool((flags.min(0) != flags.max(0)).any())
