"""What tests/test_yuv_host.py (CPU) and tests/test_yuv.py (GPU) share: the YUV rule restated in numpy int64 from the text
of include/tiny_renderer.h (not from tr_yuv.h), the four coefficient tables derived in fractions.Fraction from Kr, Kb and
the range scales, and the sizes.

The rule: coefficients in units of 1 / 65536, the nearest integers to the real matrix (limited range: Y scaled by
219 / 255, chroma by 224 / 255), the green entry adjusted so that a Y row sums to the rounded scale and a chroma row to 0.
    Y = (yr R + yg G + yb B + (y0 << 16) + 32768) >> 16
    4:4:4  U = (ur R + ug G + ub B + (128 << 16) + 32768) >> 16
    4:2:0  U = (ur Rs + ug Gs + ub Bs + (128 << 18) + (1 << 17)) >> 18 over the sums of columns 2i, min(2i + 1, W - 1) and
           rows 2j, min(2j + 1, H - 1)
each clamped to 0..255."""
from fractions import Fraction

import numpy as np

LAYOUTS = ("i420", "nv12", "i444")
MATRICES = ("bt601", "bt709")
RANGES = ("full", "limited")
TABLES = tuple((m, r) for m in MATRICES for r in RANGES)
KR_KB = {"bt601": (Fraction(299, 1000), Fraction(114, 1000)), "bt709": (Fraction(2126, 10000), Fraction(722, 10000))}

# CPU: the smallest, an even square, both odd, a unit of four pixels, both odd past a tile, odd height with width % 4 == 0
# past a tile, and several units of eight
HOST_SIZES = ((1, 1), (2, 2), (7, 5), (8, 4), (131, 19), (132, 17), (64, 48))
# GPU: flagged and unflagged tiles, units of 8 (640, 1000 with a partial tile column and partial top tile row 488 % 16),
# units of 4 and an odd height (132 x 17), bytes and unaligned chroma planes (131 x 19), one unit (8 x 8), one pixel
GPU_ALL = ((640, 480), (132, 17), (131, 19))
GPU_ONE = ((1000, 488), (8, 8), (1, 1))
CAM, LIGHT = 0.3, 0.7


def nearest(q):
    """The nearest integer to a Fraction (no tie occurs in these tables; halves would go up)."""
    return int((2 * q.numerator + q.denominator) // (2 * q.denominator))


def derive(matrix, rng):
    """(Y row, U row, V row, y0) from Kr, Kb and the scales, in exact fractions."""
    kr, kb = KR_KB[matrix]
    kg = 1 - kr - kb
    sy, sc, y0 = (Fraction(1), Fraction(1), 0) if rng == "full" else (Fraction(219, 255), Fraction(224, 255), 16)
    one = 65536
    y_real = [kr * sy, kg * sy, kb * sy]
    u_real = [-kr / (2 * (1 - kb)) * sc, -kg / (2 * (1 - kb)) * sc, Fraction(1, 2) * sc]
    v_real = [Fraction(1, 2) * sc, -kg / (2 * (1 - kr)) * sc, -kb / (2 * (1 - kr)) * sc]
    rows = []
    for real, total in ((y_real, nearest(sy * one)), (u_real, 0), (v_real, 0)):
        r = [nearest(c * one) for c in real]
        r[1] = total - r[0] - r[2]
        assert abs(r[1] - nearest(real[1] * one)) <= 1, "the adjustment of green is at most one unit"
        rows.append(tuple(r))
    return rows[0], rows[1], rows[2], y0


def real_matrix(matrix, rng):
    """The real (float64) matrix rows and offsets: Y, U, V."""
    kr, kb = (float(v) for v in KR_KB[matrix])
    kg = 1.0 - kr - kb
    sy, sc, y0 = (1.0, 1.0, 0.0) if rng == "full" else (219.0 / 255.0, 224.0 / 255.0, 16.0)
    y = np.array([kr, kg, kb]) * sy
    u = np.array([-kr, -kg, 1.0 - kb]) / (2.0 * (1.0 - kb)) * sc
    v = np.array([1.0 - kr, -kg, -kb]) / (2.0 * (1.0 - kr)) * sc
    return y, u, v, y0


def clamp(v):
    return np.clip(v, 0, 255).astype(np.uint8)


def rule_np(rgb, layout, matrix, rng, table=None, raw=False):
    """The planes of rgb [H, W, 3] uint8 by the rule, in int64: a tuple like yuv_planes gives.  raw: before the clamp."""
    yr, ur, vr, y0 = table if table is not None else derive(matrix, rng)
    p = rgb.astype(np.int64)
    Hh, W = p.shape[:2]
    fin = (lambda v: v) if raw else clamp
    dot = lambda row, q: row[0] * q[..., 0] + row[1] * q[..., 1] + row[2] * q[..., 2]
    Y = (dot(yr, p) + (y0 << 16) + 32768) >> 16
    if layout == "i444":
        return fin(Y), fin((dot(ur, p) + (128 << 16) + 32768) >> 16), fin((dot(vr, p) + (128 << 16) + 32768) >> 16)
    cw, ch = (W + 1) // 2, (Hh + 1) // 2
    xs0, ys0 = 2 * np.arange(cw), 2 * np.arange(ch)
    xs1, ys1 = np.minimum(xs0 + 1, W - 1), np.minimum(ys0 + 1, Hh - 1)
    s = p[ys0][:, xs0] + p[ys0][:, xs1] + p[ys1][:, xs0] + p[ys1][:, xs1]
    assert s.max() <= 1020
    U = (dot(ur, s) + (128 << 18) + (1 << 17)) >> 18
    V = (dot(vr, s) + (128 << 18) + (1 << 17)) >> 18
    if layout == "nv12":
        return fin(Y), fin(np.stack([U, V], -1))
    return fin(Y), fin(U), fin(V)


def flat_np(rgb, layout, matrix, rng):
    return np.concatenate([p.reshape(-1) for p in rule_np(rgb, layout, matrix, rng)])


def nbytes(W, Hh, layout):
    cw, ch = (W + 1) // 2, (Hh + 1) // 2
    return 3 * W * Hh if layout == "i444" else W * Hh + 2 * cw * ch


def noise(W, Hh, seed=0):
    return np.random.default_rng(1000 * W + Hh + seed).integers(0, 256, (Hh, W, 3), dtype=np.uint8)


def parse_y4m(path):
    """(header fields as a list of strings, [flat frames]) of a YUV4MPEG2 file of 8-bit 4:2:0 or 4:4:4 frames."""
    data = open(path, "rb").read()
    end = data.index(b"\n")
    fields = data[:end].decode("ascii").split(" ")
    assert fields[0] == "YUV4MPEG2"
    W, Hh = int([f for f in fields if f[0] == "W"][0][1:]), int([f for f in fields if f[0] == "H"][0][1:])
    colour = [f for f in fields if f[0] == "C"][0]
    n = nbytes(W, Hh, {"C420jpeg": "i420", "C444": "i444"}[colour])
    frames, at = [], end + 1
    while at < len(data):
        assert data[at:at + 6] == b"FRAME\n"
        frames.append(np.frombuffer(data[at + 6:at + 6 + n], np.uint8))
        assert frames[-1].size == n
        at += 6 + n
    return fields, frames
