"""What tests/test_lines_host.py (CPU) and tests/test_lines.py (GPU) share: the sizes, the scenes, the random tables of
segments, and the rule of lines restated in numpy from the words of include/tiny_renderer.h -- the pixels in 64-bit
integers with floor division, the depths as np.float32 steps (each operation rounds once; numpy's f32 quotient is
correctly rounded), the winner as a maximum of (key << 32) | (index + 1), the blend as layer_cases' true division.

The scenes are outline_cases' three spheres and camera.  The oracle's drawn depths there run from about 10 to 91 (nearer
is larger), so the tables draw their depths from 0..100, a third of the segments at one of three constant depths (ties in
key where two of them cross): tests/test_lines_host.py asserts on the oracle's frames of these very cases that the depth
test rejects and passes candidates, that pixels have several survivors and that keys tie."""
import numpy as np

from tests import outline_cases as OC

F32_MIN_BITS, F32_MIN, bits = OC.F32_MIN_BITS, OC.F32_MIN, OC.bits
# outline_cases.SIZES and 384 x 48, which has a tile with all eight neighbours; the GPU cases add a frame below one tile
SIZES = tuple(OC.SIZES) + ((384, 48),)
GPU_SIZES = SIZES + ((5, 3),)
CAM, LIGHT = OC.CAM, OC.LIGHT
N_SEGMENTS = 300
LIMIT = 1 << 20
FLAT_DEPTHS = (25.0, 50.0, 75.0)
# (width, depth_test, painter, opacity, depth_bias): width 1, 2 and 15, with and without the test, PAINTER
COMBOS = ((1, True, False, 256, 0.0), (2, True, False, 200, 0.5), (15, True, False, 256, -1.0), (1, False, False, 256, 0.0),
          (15, False, False, 131, 0.0), (2, False, True, 256, 0.0), (3, True, True, 255, 2.0))


def table(W, Hh):
    """The spheres' placement for a frame size."""
    return OC.table(W, Hh)


def seed_of(W, Hh):
    return 1000 * W + Hh


def segments(W, Hh, n=N_SEGMENTS, seed=None):
    """n random segments for a W x H frame as a LINE_DTYPE array: short ones, long ones, axis-parallel ones, exact
    diagonals, single pixels, endpoints far outside the frame and coordinates at +-2^20, in turn; every third one at one
    constant depth of FLAT_DEPTHS, the others with two depths from 0..100; random colours, the alpha 0, 255 or between."""
    import tiny_renderer_amd as T
    rng = np.random.default_rng(seed_of(W, Hh) if seed is None else seed)
    t = np.zeros(n, T.LINE_DTYPE)
    for i in range(n):
        kind = i % 7
        x0, y0 = int(rng.integers(-4, W + 4)), int(rng.integers(-4, Hh + 4))
        if kind == 0:      # short
            x1, y1 = x0 + int(rng.integers(-12, 13)), y0 + int(rng.integers(-12, 13))
        elif kind == 1:    # long
            x1, y1 = int(rng.integers(-4, W + 4)), int(rng.integers(-4, Hh + 4))
        elif kind == 2:    # axis-parallel
            if rng.integers(0, 2):
                x1, y1 = int(rng.integers(-4, W + 4)), y0
            else:
                x1, y1 = x0, int(rng.integers(-4, Hh + 4))
        elif kind == 3:    # an exact diagonal
            d = int(rng.integers(-max(W, Hh), max(W, Hh) + 1))
            x1, y1 = x0 + d, y0 + (d if rng.integers(0, 2) else -d)
        elif kind == 4:    # a single pixel
            x1, y1 = x0, y0
        elif kind == 5:    # far outside
            x1, y1 = x0 + int(rng.integers(-5000, 5001)), y0 + int(rng.integers(-5000, 5001))
        else:              # at the limit of the coordinates, through the frame or past it
            x1, y1 = int(rng.choice((-LIMIT, LIMIT))), int(rng.choice((-LIMIT, LIMIT, y0)))
            if rng.integers(0, 2):
                x0, y0 = -x1, -y1 if abs(y1) == LIMIT else y0
        if rng.integers(0, 2):
            x0, y0, x1, y1 = x1, y1, x0, y0
        z0, z1 = rng.random(2, np.float32) * np.float32(100.0)
        if i % 3 == 0:
            z0 = z1 = np.float32(FLAT_DEPTHS[(i // 3) % 3])
        if kind == 4:
            z1 = z0        # (n == 0 takes z0: a single pixel with two depths is the one segment whose reverse differs)
        t[i] = (x0, y0, z0, x1, y1, z1, rng.integers(0, 256, 4), 0)
        t["rgba"][i, 3] = (0, 255, 255, int(t["rgba"][i, 3]))[int(rng.integers(0, 4))]
    return t


def geometry(seg):
    """(xmajor, a0, b0, n, db, z0, z1) of a segment after the swap, in Python integers and np.float32."""
    x0, y0, x1, y1 = int(seg["x0"]), int(seg["y0"]), int(seg["x1"]), int(seg["y1"])
    z0, z1 = np.float32(seg["z0"]), np.float32(seg["z1"])
    dx, dy = x1 - x0, y1 - y0
    xmajor = abs(dx) >= abs(dy)
    a0, b0, a1, b1 = (x0, y0, x1, y1) if xmajor else (y0, x0, y1, x1)
    if a1 < a0:
        a0, b0, a1, b1, z0, z1 = a1, b1, a0, b0, z1, z0
    return xmajor, a0, b0, a1 - a0, b1 - b0, z0, z1


def candidates(seg, width, bias, W, Hh):
    """The candidates of a segment inside a W x H frame: (x, y, zl) arrays, one entry a pixel (y up)."""
    xmajor, a0, b0, n, db, z0, z1 = geometry(seg)
    A = W if xmajor else Hh
    k = np.arange(max(0, -a0), min(n, A - 1 - a0) + 1, dtype=np.int64)     # (the steps outside the frame give no pixel)
    if k.size == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.float32)
    minor = b0 + ((2 * k * db + n) // (2 * n) if n else np.zeros_like(k))
    with np.errstate(over="ignore"):
        t = (k.astype(np.float32) / np.float32(n)).astype(np.float32) if n else np.zeros(k.size, np.float32)
        z = (z0 + ((z1 - z0).astype(np.float32) * t).astype(np.float32)).astype(np.float32)
        zl = (z + np.float32(bias)).astype(np.float32)
    offs = np.arange(-((width - 1) // 2), width // 2 + 1, dtype=np.int64)
    major = np.repeat(a0 + k, offs.size)
    mn = (minor[:, None] + offs[None, :]).reshape(-1)
    zz = np.repeat(zl, offs.size)
    x, y = (major, mn) if xmajor else (mn, major)
    inside = (x >= 0) & (x < W) & (y >= 0) & (y < Hh)
    return x[inside], y[inside], zz[inside]


def keys(zl):
    b = bits(zl).astype(np.uint64)
    return np.where(b >> np.uint64(31) != 0, b ^ np.uint64(0xFFFFFFFF), b ^ np.uint64(0x80000000))


def winners(z, lines, width=1, depth_test=True, painter=False, bias=0.0, shape=None, census=None):
    """The winner word of every pixel [H, W] (y up; 0: none).  census: a dict that receives per-pixel counts."""
    Hh, W = shape if shape is not None else z.shape
    best = np.zeros((Hh, W), np.uint64)
    surv = np.zeros((Hh, W), np.int64)
    rej = np.zeros((Hh, W), np.int64)
    kept = []
    for i in range(lines.shape[0]):
        x, y, zl = candidates(lines[i], width, bias, W, Hh)
        if depth_test:
            with np.errstate(invalid="ignore"):
                ok = ~(zl <= z[y, x])
            np.add.at(rej, (y[~ok], x[~ok]), 1)
            x, y, zl = x[ok], y[ok], zl[ok]
        word = ((np.zeros(zl.size, np.uint64) if painter else keys(zl)) << np.uint64(32)) | np.uint64(i + 1)
        np.maximum.at(best, (y, x), word)
        np.add.at(surv, (y, x), 1)
        kept.append((x, y, word))
    if census is not None:
        ties = np.zeros((Hh, W), np.int64)
        for x, y, word in kept:
            np.add.at(ties, (y, x), (word >> np.uint64(32) == best[y, x] >> np.uint64(32)).astype(np.int64))
        census.update(survivors=surv, rejected=rej, tied=ties)
    return best


def rule_np(rgb, z, lines, width=1, depth_test=True, painter=False, opacity=256, bias=0.0, census=None):
    """The frame with the lines: rgb [H, W, 3] row 0 = top, z [H, W] y up (None without the test)."""
    best = winners(z, lines, width, depth_test, painter, bias, rgb.shape[:2], census)[::-1]
    won = best != 0
    index = np.where(won, (best & np.uint64(0xFFFFFFFF)).astype(np.int64) - 1, 0)
    c = lines["rgba"][index].astype(np.int64) if lines.shape[0] else np.zeros(rgb.shape[:2] + (4,), np.int64)
    d = rgb.astype(np.int64)
    a = (c[..., 3] * int(opacity))[..., None]
    mixed = (c[..., :3] * a + d * (65280 - a) + 32640) // 65280
    return np.where(won[..., None], mixed, d).astype(np.uint8)


def reverse(lines):
    out = lines.copy()
    for a, b in (("x0", "x1"), ("y0", "y1"), ("z0", "z1")):
        out[a], out[b] = lines[b], lines[a]
    return out
