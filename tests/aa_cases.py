"""What tests/test_aa_host.py (CPU) and tests/test_aa.py (GPU) share: the sizes, the models' placement, the camera and
the parameter sets of the GPU cases, and the anti-aliasing rule restated in numpy from the opening comment of
tiny_renderer_amd/csrc/tr_aa.h (which include/tiny_renderer.h repeats).

The thresholds were chosen on the CPU over the oracle's frames of these very cases; test_aa_host.py asserts the
conditions that make the GPU cases show something."""
import numpy as np

from tests import outline_cases as OC

# (W, H): OC.SIZES -- two tile rows with whole tiles; a width that is no multiple of the tile; a tile column 4 pixels wide
# and a tile row one pixel high; an odd width (the guarded bytes)
SIZES = OC.SIZES
CAM, LIGHT = OC.CAM, OC.LIGHT
MAX_SEARCH = 8
# The frames are wide and low, so the spheres of OC.table are flat ellipses whose rims are horizontal edges nearly
# everywhere.  Three tall, narrow ellipsoids in front of them (offset x, y, z, scale x, scale y) bring the vertical edges;
# the last one is cut by the frame's top, so its edges cross the one-pixel tile row of 132 x 17.
PILLARS = ((-0.8, 0.0, 0.4, 0.04, 0.9), (0.2, -0.1, 0.5, 0.05, 0.8), (0.45, 0.3, 0.45, 0.03, 1.0))
# on 512 x 64 (4 x 4 tiles): rows 18..31 (y up) of tile row 1 and columns 125..225 -- the model's top row is the last row
# of its tiles, so the black row above it, in the empty and flagged tile row 2, takes colour from it; tile row 0 is two
# rows away from the model and takes none
FLAGS_AT = np.array([[-0.4, -0.28 + 1.0 / 32.0, 0.0, 0.3]], np.float32)


def table(W, Hh):
    """The transform table (Scene(instance_transforms=...)) of the GPU cases: OC.table's spheres and the pillars."""
    import tiny_renderer_amd as T
    base = OC.table(W, Hh)
    linear = [np.eye(3) * b[3] for b in base] + [np.diag([sx, sy, sx]) for _, _, _, sx, sy in PILLARS]
    offset = [b[:3] for b in base] + [p[:3] for p in PILLARS]
    return T.instance_transforms(np.array(linear, np.float32), np.array(offset, np.float32))


def gpu_params():
    """The parameter sets of the GPU cases, as keyword arguments of aa_params: the defaults (search 8), a shorter search
    behind higher thresholds, and the diagnostic.  tests/test_aa_host.py shows for each that it is not vacuous."""
    return [dict(), dict(contrast_min=16, contrast_rel=64, search=4, subpixel=64), dict(search=5, show_blend=True)]


def edge_params():
    """The ends of every parameter's range.  search = 1 leaves the edge term at 0 (span 2, near 1) and subpixel = 0 the
    sub-pixel term, so the conditions on "who wins" cannot hold for them: they get a test of their own."""
    return [dict(search=1), dict(search=8, subpixel=0), dict(subpixel=256),
            dict(contrast_min=0, contrast_rel=0),                 # every pixel that is not flat is filtered
            dict(contrast_min=255, contrast_rel=256, subpixel=256)]  # next to nothing is


def luma_np(rgb):
    c = np.asarray(rgb, np.uint8).astype(np.int64)
    return (54 * c[..., 0] + 183 * c[..., 1] + 19 * c[..., 2] + 128) >> 8


def rule_np(rgb, contrast_min=8, contrast_rel=32, search=8, subpixel=192, show_blend=False):
    """The filtered frame and what the rule found on the way, rgb [H, W, 3] with row 0 = top.  Returns a dict: out (uint8
    [H, W, 3]) and, [H, W] each: off, off_e, off_s, passed (step 1), horizontal, side_b, dist_m, dist_p, stopped_m,
    stopped_p (did the walk stop before it ran out?).  What steps 2 to 6 give for a pixel that did not pass is
    meaningless; off is 0 there."""
    rgb = np.asarray(rgb, np.uint8)
    Hh, W, _ = rgb.shape
    c = rgb.astype(np.int64)
    lum = luma_np(rgb)
    ys, xs = np.mgrid[0:Hh, 0:W]

    def L(x, y):
        return lum[np.clip(y, 0, Hh - 1), np.clip(x, 0, W - 1)]

    M, N, S, Wl, E = L(xs, ys), L(xs, ys - 1), L(xs, ys + 1), L(xs - 1, ys), L(xs + 1, ys)
    NW, NE, SW, SE = L(xs - 1, ys - 1), L(xs + 1, ys - 1), L(xs - 1, ys + 1), L(xs + 1, ys + 1)
    five = np.stack([M, N, S, Wl, E])
    hi, lo = five.max(0), five.min(0)
    rng = hi - lo
    passed = (rng != 0) & (rng >= np.maximum(contrast_min, (hi * contrast_rel + 128) >> 8))
    EH = np.abs(NW + SW - 2 * Wl) + 2 * np.abs(N + S - 2 * M) + np.abs(NE + SE - 2 * E)
    EV = np.abs(NW + NE - 2 * N) + 2 * np.abs(Wl + E - 2 * M) + np.abs(SW + SE - 2 * S)
    horizontal = EH >= EV
    A, B = np.where(horizontal, N, Wl), np.where(horizontal, S, E)
    gA, gB = np.abs(A - M), np.abs(B - M)
    side_a = gA >= gB
    g, C = np.maximum(gA, gB), np.where(side_a, A, B)
    mid2 = M + C
    sign = np.where(side_a, -1, 1)
    nx, ny = np.where(horizontal, 0, sign), np.where(horizontal, sign, 0)
    tx, ty = horizontal.astype(np.int64), 1 - horizontal.astype(np.int64)
    dist, end, stopped = {}, {}, {}
    for s in (-1, 1):
        d, e, walking = np.full((Hh, W), search, np.int64), np.zeros((Hh, W), np.int64), np.ones((Hh, W), bool)
        for k in range(1, search + 1):
            qx, qy = xs + s * k * tx, ys + s * k * ty
            d2 = L(qx, qy) + L(qx + nx, qy + ny) - mid2
            e = np.where(walking, d2, e)
            stop = walking & (2 * np.abs(d2) >= g)
            d = np.where(stop, k, d)
            walking = walking & ~stop
        dist[s], end[s], stopped[s] = d, e, ~walking
    span = dist[-1] + dist[1]
    minus = dist[-1] < dist[1]
    near, end_near = np.where(minus, dist[-1], dist[1]), np.where(minus, end[-1], end[1])
    good = (end_near < 0) != (2 * M - mid2 < 0)
    off_e = np.where(good, ((span - 2 * near) * 128 + span // 2) // span, 0)
    a = np.abs(2 * (N + S + Wl + E) + NW + NE + SW + SE - 12 * M)
    tq = np.minimum(256, (a * 256) // (12 * np.maximum(rng, 1)))
    sm = (tq * tq * (768 - 2 * tq)) >> 16
    off_s = (((sm * sm) >> 8) * subpixel) >> 8
    off = np.where(passed, np.maximum(off_e, off_s), 0)
    Fn = c[np.clip(ys + ny, 0, Hh - 1), np.clip(xs + nx, 0, W - 1)]
    out = (c * (256 - off)[..., None] + Fn * off[..., None] + 128) >> 8
    if show_blend:
        out = np.broadcast_to(np.minimum(255, off)[..., None], c.shape)
    return {"out": out.astype(np.uint8), "off": off, "off_e": off_e, "off_s": off_s, "passed": passed, "horizontal": horizontal,
            "side_b": ~side_a, "dist_m": dist[-1], "dist_p": dist[1], "stopped_m": stopped[-1], "stopped_p": stopped[1]}
