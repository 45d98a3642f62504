"""What tests/test_outline_host.py (CPU) and tests/test_outline.py (GPU) share: the sizes, the models' placement, the
camera and the thresholds of the GPU cases, and the outline rule restated in numpy from the words of
include/tiny_renderer.h.

The thresholds were chosen on the CPU with tr_outline_kinds over the oracle's frames of these very cases, so that every
kind occurs and the ink covers a sensible part of the frame; test_outline_host.py asserts those conditions."""
import numpy as np

F32_MIN_BITS = np.uint32(0xFF7FFFFF)
F32_MIN = F32_MIN_BITS.view(np.float32)
SIL, STEP, CREASE = 1, 2, 4

# (W, H): two tiles each way with whole tiles; a partial tile column and row; a tile column 4 pixels wide and a tile row
# one pixel high; an odd width, which no 16-byte piece and no 12-byte unit fits (the guarded form)
SIZES = ((256, 48), (200, 40), (132, 17), (131, 19))
# three spheres (offset x, y, z, scale): two that overlap at different depths, so that the nearer one's rim is a depth
# step, and one at the top right; on the two small frames the third is cut by the frame's corner
AT_WIDE = np.array([[-0.45, 0.0, 0.0, 0.5], [0.0, 0.1, 0.35, 0.4], [0.66, 0.42, 0.1, 0.5]], np.float32)
AT_SMALL = np.array([[-0.5, -0.1, 0.0, 0.35], [-0.15, 0.05, 0.3, 0.3], [0.95, 0.75, 0.1, 0.4]], np.float32)
CAM, LIGHT = 0.3, 0.7
DEPTH_STEP, CREASE_T = 6.0, 1.5
INK = (20, 30, 120)
PAPER = (250, 240, 200)


def table(W, Hh):
    return AT_WIDE if W >= 200 else AT_SMALL


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def kinds_np(z, depth_step, crease=None):
    """The kind bits of every pixel, z [H, W] y up; crease None: TR_OUTLINE_CREASES is not set."""
    z = np.ascontiguousarray(z, np.float32)
    Hh, W = z.shape
    drawn = bits(z) != F32_MIN_BITS
    step = np.float32(depth_step)
    k = np.zeros((Hh, W), np.uint8)

    def shifted(a, dx, dy, fill):
        """a at (x + dx, y + dy), `fill` where that lies outside the frame."""
        out = np.full(a.shape, fill, a.dtype)
        ys, yd = (slice(dy, None), slice(None, Hh - dy)) if dy >= 0 else (slice(None, dy), slice(-dy, None))
        xs, xd = (slice(dx, None), slice(None, W - dx)) if dx >= 0 else (slice(None, dx), slice(-dx, None))
        out[yd, xd] = a[ys, xs]
        return out

    exists = np.ones((Hh, W), bool)
    nb = {}
    for dx, dy in ((-1, 0), (1, 0), (0, -1), (0, 1)):
        nb[dx, dy] = (shifted(z, dx, dy, np.float32(0.0)), shifted(drawn, dx, dy, False), shifted(exists, dx, dy, False))
    with np.errstate(invalid="ignore", over="ignore"):
        for zq, dq, eq in nb.values():
            k |= np.where(drawn & eq & ~dq, SIL, 0).astype(np.uint8)
            k |= np.where(drawn & eq & dq & ((z - zq).astype(np.float32) > step), STEP, 0).astype(np.uint8)
        if crease is not None:
            cr = np.float32(crease)
            for a, b in (((-1, 0), (1, 0)), ((0, -1), (0, 1))):
                (za, da, ea), (zb, db, eb) = nb[a], nb[b]
                both = drawn & ea & eb & da & db
                flat_a = ~(np.abs((z - za).astype(np.float32)) > step)
                flat_b = ~(np.abs((z - zb).astype(np.float32)) > step)
                second = np.abs(((za + zb).astype(np.float32) - (z + z).astype(np.float32)).astype(np.float32)) > cr
                k |= np.where(both & flat_a & flat_b & second, CREASE, 0).astype(np.uint8)
    return k


def inked_np(kinds, radius):
    """Which pixels are inked: within `radius` (Chebyshev) of a seed, inside the frame."""
    Hh, W = kinds.shape
    seed = kinds != 0
    pad = np.zeros((Hh + 2 * radius, W + 2 * radius), bool)
    pad[radius:radius + Hh, radius:radius + W] = seed
    out = np.zeros((Hh, W), bool)
    for dy in range(2 * radius + 1):
        for dx in range(2 * radius + 1):
            out |= pad[dy:dy + Hh, dx:dx + W]
    return out


def rule_np(z, rgb, radius, depth_step, crease=None, ink=(0, 0, 0), opacity=256, only=False, paper=(255, 255, 255)):
    """The outlined frame: z [H, W] y up, rgb [H, W, 3] row 0 = top."""
    inked = inked_np(kinds_np(z, depth_step, crease), radius)[::-1]
    base = np.broadcast_to(np.array(paper, np.uint32), rgb.shape) if only else rgb.astype(np.uint32)
    mixed = (np.array(ink, np.uint32) * np.uint32(opacity) + base * np.uint32(256 - opacity) + np.uint32(128)) >> np.uint32(8)
    return np.where(inked[..., None], mixed, base).astype(np.uint8)


def gpu_params():
    """The parameter sets of the GPU cases, as keyword arguments of outline_params."""
    out = []
    for radius in (0, 1, 3):
        out.append(dict(radius=radius, depth_step=DEPTH_STEP, ink=INK))
        out.append(dict(radius=radius, depth_step=DEPTH_STEP, crease=CREASE_T, ink=INK, opacity=100))
    out.append(dict(radius=1, depth_step=DEPTH_STEP, crease=CREASE_T, ink=INK, only=True, paper=(0, 0, 0)))
    out.append(dict(radius=3, depth_step=DEPTH_STEP, ink=INK, only=True, paper=PAPER, opacity=100))
    return out
