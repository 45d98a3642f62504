"""What tests/test_distance_host.py (CPU) and tests/test_distance.py (GPU) share: the sizes, the scenes, the seed
patterns, and the distance rule restated in numpy from the words of include/tiny_renderer.h -- the field as a plain
all-pairs minimum, the integer square root corrected in integers, the ramp through ramp_cases.entries_np and
layer_cases.blend_np.

The scenes are ramp_cases' camera, light and three spheres on ramp_cases.SIZES, but the spheres are MOVED: under
ramp_cases' placements every tile of the 128 x 16 grid has a drawn pixel within four pixels on four of the five sizes, and
the cases need a tile that is all FAR at R = 4 at every size.  Here the spheres are smaller and stand in the lower half of
the frame (AT): the top tile row is all FAR, the partial tile column of 200, 132 and 131 still holds drawn pixels, and
seeds, near pixels (0 < d2 <= 16) and FAR pixels each hold well over 1 % of every frame (test_distance_host.py asserts
it on the oracle's frames).  40 x 300 and 37 x 5, which ramp_cases does not have, use outline_cases' small placement."""
import numpy as np

from tests import layer_cases as LC
from tests import outline_cases as OC
from tests import ramp_cases as RC

F32_MIN_BITS, F32_MIN, bits = OC.F32_MIN_BITS, OC.F32_MIN, OC.bits
FAR = 0xFFFF
SIZES = RC.SIZES
EXTRA = ((40, 300), (37, 5))                     # tall: many rows, one tile column; below one tile
HOST_SIZES = ((1, 1), (37, 5), (131, 19), (256, 48), (384, 48), (40, 300), (300, 300))
HOST_RADII = (1, 2, 5, 16, 254, 255)
GPU_RADII = (1, 4, 16, 255)
CAM, LIGHT = RC.CAM, RC.LIGHT
GLOW = (255, 200, 40)
AT = np.array([[-0.5, -0.35, 0.0, 0.3], [-0.15, -0.4, 0.3, 0.25], [0.95, -0.35, 0.1, 0.3]], np.float32)
INVERT_PIXELS = 13000                            # the all-pairs minimum of a sparse mask's complement: frames up to this size


def table(W, Hh):
    """The spheres' placement for a frame size."""
    return AT if (W, Hh) in RC.SIZES else OC.AT_SMALL


def seeds_np(rgb, z, seed="drawn", threshold=0, invert=False):
    """The seed mask [H, W], row 0 = top: rgb [H, W, 3] row 0 = top, z [H, W] y up (not looked at under "key")."""
    m = rgb.max(axis=2) >= threshold if seed == "key" else (bits(np.ascontiguousarray(z, np.float32)) != F32_MIN_BITS)[::-1]
    return ~m if invert else m


def nearest_np(mask):
    """The squared distance of every pixel to the nearest set pixel of mask, uncapped (int64; -1 without a set pixel):
    the minimum over all pairs, in chunks of pixels."""
    Hh, W = mask.shape
    ys, xs = np.nonzero(mask)
    if ys.size == 0:
        return np.full((Hh, W), -1, np.int64)
    py, px = np.divmod(np.arange(Hh * W, dtype=np.int64), W)
    out = np.empty(Hh * W, np.int64)
    chunk = max(1, 20_000_000 // ys.size)
    ys, xs = ys.astype(np.int32), xs.astype(np.int32)
    for k in range(0, Hh * W, chunk):
        dy = py[k:k + chunk, None].astype(np.int32) - ys
        dx = px[k:k + chunk, None].astype(np.int32) - xs
        out[k:k + chunk] = (dy * dy + dx * dx).min(axis=1)
    return out.reshape(Hh, W)


def cap_np(nearest, R):
    """The field of radius R from nearest_np's result."""
    return np.where((nearest >= 0) & (nearest <= R * R), nearest, FAR).astype(np.uint16)


def field_np(mask, R):
    return cap_np(nearest_np(mask), R)


def frame_of(mask, rng=None):
    """(rgb, z) whose seeds are `mask` (row 0 = top) under "drawn" and under "key" at any threshold 100..200: seeds are
    bright and have a depth, the rest is dim (random below 100 where rng is given, else black) and has none."""
    Hh, W = mask.shape
    rgb = np.zeros((Hh, W, 3), np.uint8)
    if rng is not None:
        rgb[...] = rng.integers(0, 100, (Hh, W, 3), dtype=np.uint8)
    rgb[mask] = (200, 90, 10)
    z = np.where(mask[::-1], np.float32(1.5), F32_MIN).astype(np.float32)
    return rgb, z


def planted(kind, W, Hh, R, rng):
    """The planted seed patterns of the issue, as masks [H, W]."""
    m = np.zeros((Hh, W), bool)
    if kind == "none":
        pass
    elif kind == "all":
        m[...] = True
    elif kind == "corners":
        for y, x in ((0, 0), (0, W - 1), (Hh - 1, 0), (Hh - 1, W - 1), (Hh // 2, W // 2)):
            m[y, x] = True
    elif kind == "edges":                       # mask-word and tile edges
        for i, x in enumerate((63, 64, 127, 128)):
            if x < W:
                m[(i * 7) % Hh, x] = True
    elif kind == "pair_x":                      # two seeds R and R + 1 apart along x: the pixels between see one or none
        m[Hh // 2, 0] = True
        if 2 * R + 1 < W:
            m[Hh // 2, 2 * R + 1] = True
        if Hh > 3 and 2 * R + 2 < W:
            m[0, 2 * R + 2] = m[0, 0] = True
    elif kind == "pair_y":
        m[0, W // 2] = True
        if 2 * R + 1 < Hh:
            m[2 * R + 1, W // 2] = True
    elif kind == "one_percent":
        m = rng.random((Hh, W)) < 0.01
    elif kind == "half":
        m = rng.random((Hh, W)) < 0.5
    else:
        raise ValueError(kind)
    return m


PATTERNS = ("none", "all", "corners", "edges", "pair_x", "pair_y", "one_percent", "half")


def isqrt_np(v):
    """floor(sqrt(v)) of an int64 array, corrected in integers."""
    v = np.asarray(v, np.int64)
    q = np.floor(np.sqrt(v.astype(np.float64))).astype(np.int64)
    q -= (q * q > v)
    q += ((q + 1) * (q + 1) <= v)
    return q


def ramp_np(rgb, field, tab, step=256, mode="normal", opacity=256, far=(0, 0, 0, 0), repeat=False, keep_seeds=False):
    """The frame ramped by its field: rgb [H, W, 3] and field [H, W], both row 0 = top, tab [n, 4]."""
    n = tab.shape[0]
    pmax = (n - 1) * 256
    kept = field != FAR
    d2 = np.where(kept, field, 0).astype(np.int64)
    p = (isqrt_np(d2 << 16) * int(step)) >> 8
    p = p % pmax if repeat else np.minimum(p, pmax)
    e = np.where(kept[..., None], RC.entries_np(tab, p), np.array(far, np.int64))
    d = rgb.astype(np.int64)
    cov = e[..., 3] * int(opacity)
    if keep_seeds:
        cov = np.where(field == 0, 0, cov)
    cov = cov[..., None]
    return ((LC.blend_np(mode, e[..., :3], d) * cov + d * (65280 - cov) + 32640) // 65280).astype(np.uint8)


# a short fixed list for the ramp on the device: (mode, opacity, repeat, far alpha, keep_seeds), after ramp_cases.SHORT
SHORT = tuple(c + (i % 2 == 1,) for i, c in enumerate(RC.SHORT))


def far_of(alpha):
    return (GLOW[0], GLOW[1], GLOW[2], alpha)
