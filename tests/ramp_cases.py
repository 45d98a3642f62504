"""What tests/test_ramp_host.py (CPU) and tests/test_ramp.py (GPU) share: the sizes, the scenes, the span of the GPU
cases, the tables, and the ramp rule restated in numpy from the words of include/tiny_renderer.h (f32 steps as
np.float32, the cast through float64, true division in int64 as layer_cases.blend_np).

The span (NEAR, FAR) was chosen on the CPU with tr_ramp_positions over the oracle's frames of these very cases -- their
drawn depths run from about 10 to 91, nearer is larger -- so that about a fifth of the drawn pixels lie in front of the
ramp (p == 0), about a fifth behind it (clamped at pmax) and the rest inside; tests/test_ramp_host.py asserts those
conditions.

The scenes are outline_cases' three spheres and camera, with ONE exception: on 131 x 19 outline_cases' third sphere
(0.95, 0.75) reaches all four tiles of the frame, and the cases need a tile in which nothing is drawn at every size --
in the byte form too.  There the third sphere stands at (0.95, 0.5): the partial tile column still holds drawn pixels,
the top tile row (three rows high) is empty."""
import numpy as np

from tests import layer_cases as LC
from tests import outline_cases as OC

F32_MIN_BITS, F32_MIN, bits = OC.F32_MIN_BITS, OC.F32_MIN, OC.bits
MODES = LC.MODES
OPACITIES = LC.OPACITIES
# outline_cases.SIZES -- whole tiles with WORDS; a partial tile column and row; a 4-pixel tile column and a 1-row tile row;
# an odd width for the byte form -- and 384 x 48, which has a tile with all eight neighbours
SIZES = tuple(OC.SIZES) + ((384, 48),)
CAM, LIGHT = OC.CAM, OC.LIGHT
AT_ODD = OC.AT_SMALL.copy()
AT_ODD[2] = (0.95, 0.5, 0.1, 0.4)
NEAR, FAR = 82.0, 42.0
NS = (2, 3, 256, 1024)
FOG = (200, 210, 230)
# a short fixed list for the sizes that do not run every mode: (mode, opacity, repeat, undrawn alpha)
SHORT = (("normal", 256, False, 0), ("normal", 200, False, 255), ("multiply", 256, False, 255), ("add", 180, True, 0), ("difference", 77, True, 130))


def table(W, Hh):
    """The spheres' placement for a frame size."""
    return AT_ODD if (W, Hh) == (131, 19) else OC.table(W, Hh)


def random_table(rng, n):
    """n random rgba entries: every byte value is likely; the alpha column holds 0, 255 and values between."""
    t = rng.integers(0, 256, (n, 4), dtype=np.uint8)
    pick = rng.integers(0, 4, n)
    t[:, 3] = np.where(pick == 0, 0, np.where(pick == 1, 255, t[:, 3]))
    return t


def undrawn_of(alpha):
    return (FOG[0], FOG[1], FOG[2], alpha)


def span(n, near=NEAR, far=FAR):
    """(z0, scale) as np.float32: position 0 at `near`, pmax at `far` -- ramp_span's definition, restated."""
    a, b = np.float32(near), np.float32(far)
    return a, np.float32(float((n - 1) * 256) / (float(b) - float(a)))


def positions_np(z, z0, scale, n, repeat=False):
    """(p, drawn) of every depth: p uint64 after the clamp or the wrap (whatever it is where nothing is drawn)."""
    z = np.ascontiguousarray(z, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        d = (z - np.float32(z0)).astype(np.float32)
        c = (d * np.float32(scale)).astype(np.float32)
    c64 = c.astype(np.float64)
    c64 = np.where(np.isnan(c64), 0.0, c64)
    p = np.floor(np.clip(c64, 0.0, float(2 ** 32 - 1))).astype(np.uint64)
    pmax = np.uint64((n - 1) * 256)
    p = p % pmax if repeat else np.minimum(p, pmax)
    return p, bits(z) != F32_MIN_BITS


def entries_np(tab, p):
    """The interpolated entries [..., 4] (int64) at the positions p."""
    n = tab.shape[0]
    p = p.astype(np.int64)
    i, f = p >> 8, p & 255
    j = np.minimum(i + 1, n - 1)
    E = tab.astype(np.int64)
    return (E[i] * (256 - f)[..., None] + E[j] * f[..., None] + 128) >> 8


def rule_np(rgb, z, tab, z0, scale, mode="normal", opacity=256, undrawn=(0, 0, 0, 0), repeat=False):
    """The ramped frame: rgb [H, W, 3] row 0 = top, z [H, W] y up, tab [n, 4]."""
    p, drawn = positions_np(z, z0, scale, tab.shape[0], repeat)
    e = np.where(drawn[..., None], entries_np(tab, p), np.array(undrawn, np.int64))[::-1]
    d = rgb.astype(np.int64)
    cov = (e[..., 3] * int(opacity))[..., None]
    return ((LC.blend_np(mode, e[..., :3], d) * cov + d * (65280 - cov) + 32640) // 65280).astype(np.uint8)
