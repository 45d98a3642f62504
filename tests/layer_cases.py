"""What tests/test_layer_host.py (CPU) and tests/test_layer.py (GPU) share: the sizes, the layer placements, the random
layers, and the layer rule restated in numpy from the words of include/tiny_renderer.h (true division in int64, no
multiply-shift)."""
import numpy as np

from tests import outline_cases as OC

F32_MIN_BITS, F32_MIN, bits = OC.F32_MIN_BITS, OC.F32_MIN, OC.bits
MODES = ("normal", "add", "multiply", "screen", "lighten", "darken", "difference")
FORMATS = ("rgb8", "rgba8")
OPACITIES = (0, 1, 128, 255, 256)
KEY = (17, 130, 240)
# outline_cases.SIZES -- whole tiles with WORDS; a partial tile column; a 4-pixel tile column and a 1-row tile row; the
# byte form with odd rows -- and 384 x 48, which has a tile with all eight neighbours: a rectangle can end inside it on
# every side
SIZES = tuple(OC.SIZES) + ((384, 48),)
# a short fixed list for the sizes that do not run every mode: (mode, format, opacity)
SHORT = (("normal", "rgb8", 256), ("normal", "rgba8", 200), ("multiply", "rgb8", 256), ("add", "rgba8", 256), ("difference", "rgb8", 77))


def placements(W, Hh):
    """(name, x, y, w, h) per frame size: frame-sized at (0, 0); insets whose left edge is 1, 2 and 3 mod 4 and whose
    width is no multiple of 4 (the 384-wide frame's ends inside its middle tile on every side); one over the top-left
    corner, one over the bottom-right; one pixel; one that misses the frame."""
    out = [("frame", 0, 0, W, Hh)]
    for k in (1, 2, 3):
        x = (132 if W >= 384 else 4) + k
        w = min(W - x - 2, 117 if W >= 384 else 61) | 1          # odd: no multiple of 4
        y = 18 if Hh >= 48 else 2
        out.append(("inset%d" % k, x, y, w, max(1, min(Hh - y - 3, 11))))
    out.append(("top-left", -7, -5, 41, 14))
    out.append(("bottom-right", W - 30, Hh - 6, 50, 13))
    out.append(("pixel", W // 2 + 1, Hh // 2, 1, 1))
    out.append(("miss", W, -3, 9, 9))
    return out


def random_layer(rng, w, h, channels, key=None):
    """A random layer [h, w, channels]: every byte value is likely; with four channels the alpha plane holds 0, 255 and
    values between; a quarter of the pixels carry `key` where one is given."""
    img = rng.integers(0, 256, (h, w, channels), dtype=np.uint8)
    if channels == 4:
        pick = rng.integers(0, 4, (h, w))
        img[..., 3] = np.where(pick == 0, 0, np.where(pick == 1, 255, img[..., 3]))
    if key is not None:
        img[rng.integers(0, 4, (h, w)) == 0, :3] = key
    return img


def blend_np(mode, s, d):
    s, d = s.astype(np.int64), d.astype(np.int64)
    if mode == "normal":
        return s
    if mode == "add":
        return np.minimum(255, s + d)
    if mode == "multiply":
        return (s * d + 127) // 255
    if mode == "screen":
        return 255 - ((255 - s) * (255 - d) + 127) // 255
    if mode == "lighten":
        return np.maximum(s, d)
    if mode == "darken":
        return np.minimum(s, d)
    if mode == "difference":
        return np.abs(s - d)
    raise ValueError(mode)


def rule_np(rgb, image, x=0, y=0, mode="normal", opacity=256, where=None, key=None, z=None):
    """The layered frame: rgb [H, W, 3] row 0 = top, image [h, w, 3 | 4], z [H, W] y up (with `where`)."""
    Hh, W, _ = rgb.shape
    h, w, ch = image.shape
    out = rgb.copy()
    x0, y0, x1, y1 = max(0, x), max(0, y), min(W, x + w), min(Hh, y + h)
    if x0 >= x1 or y0 >= y1:
        return out
    layer = image[y0 - y:y1 - y, x0 - x:x1 - x].astype(np.int64)
    d = rgb[y0:y1, x0:x1].astype(np.int64)
    s = layer[..., :3]
    alpha = layer[..., 3] if ch == 4 else np.full(s.shape[:2], 255, np.int64)
    a = alpha * opacity
    if key is not None:
        a = np.where((s == np.array(key, np.int64)).all(-1), 0, a)
    if where is not None:
        drawn = (bits(z) != F32_MIN_BITS)[::-1][y0:y1, x0:x1]
        a = np.where(drawn if where == "undrawn" else ~drawn, 0, a)
    a = a[..., None]
    out[y0:y1, x0:x1] = ((blend_np(mode, s, d) * a + d * (65280 - a) + 32640) // 65280).astype(np.uint8)
    return out
