"""The windows, range tables, guides, edges and sizes tests/test_bilateral_host.py and tests/test_bilateral.py share, and the
rule of the bilateral stage restated in numpy int64 / float32 from its text (include/tiny_renderer.h), not from
tr_bilateral.h: pad, shift, distance, table, sums, one integer division."""
import numpy as np

from tests import convolve_cases as CC

PAPER = CC.PAPER
EDGES = CC.EDGES
IMAGES = CC.IMAGES
FRAMES = CC.FRAMES
CAM, LIGHT = CC.CAM, CC.LIGHT
image = CC.image
F32_MIN = np.float32(-3.4028234663852886e38)
F32_MIN_BITS = 0xFF7FFFFF
SCALE = 40.0   # the depth_scale of the host cases: planes() below steps by 0.02 a column and 0.05 a row


def bits(z):
    return np.ascontiguousarray(z, np.float32).view(np.uint32)


def _rng(seed):
    return np.random.default_rng(seed)


def _l_shape():
    """An asymmetric L of unequal weights in a 5 x 7 box (row 0 = top): mirrored in either axis it is another window -- the
    kernel's rows run bottom-up."""
    w = np.zeros((7, 5), np.uint8)
    w[:, 0] = (250, 200, 150, 100, 60, 30, 9)
    w[6, :4] = (9, 77, 140, 255)
    return w


def windows():
    """{name: [kh, kw] uint8}"""
    import tiny_renderer_amd as T
    hole = np.full((3, 3), 200, np.uint8)
    hole[1, 1] = 0
    return {
        "1x1": np.array([[255]], np.uint8), "3x3": T.spatial_box(3, 3), "15x1": T.spatial_box(15, 1), "1x15": T.spatial_box(1, 15),
        "5x3_random": _rng(11).integers(0, 256, (3, 5)).astype(np.uint8), "L": _l_shape(), "centre_zero": hole,
        "15x15": T.spatial_box(15, 15), "gaussian7": T.spatial_gaussian(3, 2.0),
    }


def tables():
    """{name: [256] uint8}"""
    import tiny_renderer_amd as T
    return {
        "all255": np.full(256, 255, np.uint8), "step0": T.range_step(0), "step6": T.range_step(6), "gaussian10": T.range_gaussian(10.0),
        "zeros": np.zeros(256, np.uint8), "random": _rng(12).integers(0, 256, 256).astype(np.uint8),
    }


def everything():
    """{name: dict(spatial, range, guide, depth_scale)}: every window under step6, every table under the 3 x 3 box and the
    random 5 x 3, the largest window under the plain mean and the random table -- each under both guides."""
    Wn, Tb = windows(), tables()
    pairs = [(w, "step6") for w in Wn] + [(w, t) for w in ("3x3", "5x3_random") for t in Tb if t != "step6"]
    pairs += [("15x15", "all255"), ("15x15", "random"), ("L", "gaussian10"), ("gaussian7", "gaussian10"), ("centre_zero", "step0")]
    out = {}
    for w, t in pairs:
        for guide in ("colour", "depth"):
            out["%s_%s_%s" % (w, t, guide)] = dict(spatial=Wn[w], range=Tb[t], guide=guide, depth_scale=SCALE)
    return out


def params(case, edge="clamp", border=(0, 0, 0), depth_scale=None):
    import tiny_renderer_amd as T
    return T.bilateral_params(case["spatial"], case["range"], guide=case["guide"], depth_scale=case["depth_scale"] if depth_scale is None else depth_scale,
                              edge=edge, border=border)


def planes(W, Hh, seed=0):
    """z [H, W] float32, y up: two drawn planes that meet in a step down the middle, each sloped so that neighbours lie
    0.8 (a column) and 2 (a row) apart under SCALE; a block that is not drawn; where there is room a NaN and an infinity."""
    x, y = np.arange(W, dtype=np.float32)[None, :], np.arange(Hh, dtype=np.float32)[:, None]
    z = (np.float32(-10.0) + np.float32(0.02) * x + np.float32(0.05) * y).astype(np.float32)
    z[:, W // 2:] += np.float32(3.0)
    z[Hh // 3:Hh // 3 + max(Hh // 4, 1), W // 4:W // 4 + max(W // 5, 1)] = F32_MIN
    if W * Hh >= 6:
        r = _rng(500 + seed + 3 * W + Hh)
        z[r.integers(0, Hh), r.integers(0, W)] = np.float32(np.nan)
        z[r.integers(0, Hh), r.integers(0, W)] = np.float32(np.inf) if seed % 2 == 0 else np.float32(-np.inf)
    return z


def depth_distance(zt, zc, scale):
    """d of the DEPTH guide: every f32 operation rounded once; NaN and infinity give 255."""
    with np.errstate(invalid="ignore", over="ignore"):
        diff = (np.asarray(zt, np.float32) - np.asarray(zc, np.float32)).astype(np.float32)
        t = (np.abs(diff) * np.float32(scale)).astype(np.float32)
        small = t < np.float32(255.0)
    return np.where(small, np.where(small, t, 0.0).astype(np.int64), 255)


def rule(rgb, case, edge="clamp", border=(0, 0, 0), z=None, depth_scale=None):
    """The rule's text.  rgb [H, W, 3] row 0 = top; z [H, W] y up (the DEPTH guide)."""
    w = np.asarray(case["spatial"], np.int64)
    table = np.asarray(case["range"], np.int64)
    scale = case["depth_scale"] if depth_scale is None else depth_scale
    depth = case["guide"] == "depth"
    kh, kw = w.shape
    Hh, W = rgb.shape[:2]
    F = rgb.astype(np.int64)
    pad = ((kh // 2, kh // 2), (kw // 2, kw // 2))
    if edge == "clamp":
        P = np.pad(F, pad + ((0, 0),), mode="edge")
    else:
        P = np.empty((Hh + kh - 1, W + kw - 1, 3), np.int64)
        P[...] = np.array(border, np.int64)
        P[kh // 2:kh // 2 + Hh, kw // 2:kw // 2 + W] = F
    if depth:
        Z = np.ascontiguousarray(z, np.float32)[::-1]   # row 0 = top, as the frame
        Zp = np.pad(Z, pad, mode="edge") if edge == "clamp" else np.pad(Z, pad, mode="constant", constant_values=F32_MIN)
    S = np.zeros((Hh, W), np.int64)
    A = np.zeros((Hh, W, 3), np.int64)
    for j in range(kh):
        for i in range(kw):
            if w[j, i] == 0:
                continue
            T = P[j:j + Hh, i:i + W]
            d = depth_distance(Zp[j:j + Hh, i:i + W], Z, scale) if depth else np.abs(T - F).max(-1)
            wt = w[j, i] * table[d]
            S += wt
            A += wt[..., None] * T
    assert S.max(initial=0) < 1 << 24 and (A + (S // 2)[..., None]).max(initial=0) < 1 << 32
    out = np.where((S == 0)[..., None], F, (A + (S // 2)[..., None]) // np.maximum(S, 1)[..., None])
    assert out.min(initial=0) >= 0 and out.max(initial=0) <= 255
    return out.astype(np.uint8)


def scale_for(z):
    """A depth_scale for a rendered frame's z: the drawn depths' span becomes 1200 steps, so that neighbours on a surface
    lie a few steps apart and a silhouette lies beyond every cutoff of tables()."""
    drawn = bits(z) != F32_MIN_BITS
    span = float(z[drawn].max() - z[drawn].min()) if drawn.any() else 0.0
    return float(np.float32(1200.0 / span)) if span > 0.0 else 1.0


def planted_colour(seed=0):
    """40 x 12: columns 0..19 at 60 and 20..39 at 180 in every channel, each value with independent noise in [-3, 3]."""
    base = np.where(np.arange(40) < 20, 60, 180)[None, :, None] + np.zeros((12, 1, 3), np.int64)
    return (base + _rng(300 + seed).integers(-3, 4, (12, 40, 3))).astype(np.uint8)


def same_side_mean(img, side, rx=2, ry=2):
    """The rounded mean over the taps of a CLAMPed (2 rx + 1) x (2 ry + 1) box that lie on the pixel's own side: side [H, W]
    of labels."""
    Hh, W = side.shape
    F = np.pad(img.astype(np.int64), ((ry, ry), (rx, rx), (0, 0)), mode="edge")
    L = np.pad(side, ((ry, ry), (rx, rx)), mode="edge")
    S = np.zeros((Hh, W), np.int64)
    A = np.zeros((Hh, W, 3), np.int64)
    for j in range(2 * ry + 1):
        for i in range(2 * rx + 1):
            own = (L[j:j + Hh, i:i + W] == side).astype(np.int64)
            S += own
            A += own[..., None] * F[j:j + Hh, i:i + W]
    assert S.min() >= 1
    return ((A + (S // 2)[..., None]) // S[..., None]).astype(np.uint8)
