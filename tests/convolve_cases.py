"""The kernels, edges and sizes tests/test_convolve_host.py and tests/test_convolve.py share, and the rule of the convolve
stage restated in numpy int64 from its text (include/tiny_renderer.h), not from tr_convolve.h."""
import numpy as np

PAPER = (250, 240, 200)
EDGES = (("border", (0, 0, 0)), ("border", PAPER), ("clamp", (0, 0, 0)))
# images of the host test: narrower and shorter than a 31-tap kernel among them
IMAGES = ((1, 1), (2, 3), (7, 5), (20, 9), (64, 1), (1, 40), (131, 19))
# rendered frames of the device test: both tile borders, a 4-pixel tile column, a 1-row tile row, an odd width, a tile with
# all eight neighbours, the smallest
FRAMES = ((640, 480), (256, 48), (200, 40), (132, 17), (131, 19), (384, 48), (20, 9))
CAM, LIGHT = 0.3, 0.7


def _rng(seed):
    return np.random.default_rng(seed)


def _tap(i, j):
    k = np.zeros((3, 3), np.int32)
    k[j, i] = 1
    return k


def _signed(seed, kh, kw):
    return _rng(seed).integers(-300, 301, (kh, kw)).astype(np.int32)


def tent(R):
    return (R + 1 - np.abs(np.arange(-R, R + 1))).astype(np.int32)


def gaussian31():
    import tiny_renderer_amd as T
    return T.kernel_gaussian(5.0, 15)


def general():
    """{name: dict(kernel=[kh, kw], shift, bias, absolute)}"""
    alt = (32767 * (1 - 2 * (np.add.outer(np.arange(9), np.arange(9)) % 2))).astype(np.int32)
    return {
        "identity": dict(kernel=np.array([[1]], np.int32)),
        "shift_left": dict(kernel=_tap(0, 1)), "shift_right": dict(kernel=_tap(2, 1)),
        "shift_up": dict(kernel=_tap(1, 0)), "shift_down": dict(kernel=_tap(1, 2)),
        "box3": dict(kernel=np.ones((3, 3), np.int32)),
        "sobel_x_abs": dict(kernel=np.array([[-1, 0, 1], [-2, 0, 2], [-1, 0, 1]], np.int32), absolute=True),
        "emboss": dict(kernel=np.array([[-1, -1, 0], [-1, 0, 1], [0, 1, 1]], np.int32), bias=128),
        "9x1": dict(kernel=_signed(1, 1, 9), shift=8, bias=100), "1x9": dict(kernel=_signed(2, 9, 1), shift=8, bias=100),
        "5x3": dict(kernel=_signed(3, 3, 5), shift=9, bias=90), "3x7": dict(kernel=_signed(4, 7, 3), shift=10, bias=110),
        "9x9_max": dict(kernel=np.full((9, 9), 32767, np.int32), shift=22),
        "9x9_alternating": dict(kernel=alt, shift=15, bias=128),
    }


def separable():
    """{name: dict(kernel=(row, col), shift, bias, unsharp)}"""
    import tiny_renderer_amd as T
    one = np.array([1], np.int32)
    g31, s31 = gaussian31()
    g2, s2 = T.kernel_gaussian(2.0)
    out = {
        "1x1": dict(kernel=(one, one)),
        "31x1": dict(kernel=(_rng(5).integers(-200, 201, 31).astype(np.int32), one), shift=10, bias=120),
        "1x31": dict(kernel=(one, _rng(6).integers(-200, 201, 31).astype(np.int32)), shift=10, bias=120),
        "3x5": dict(kernel=(_rng(7).integers(-90, 91, 3).astype(np.int32), _rng(8).integers(-90, 91, 5).astype(np.int32)), shift=12, bias=100),
        "gaussian31": dict(kernel=g31, shift=s31),
        "extreme": dict(kernel=(np.full(31, 1057, np.int32), (4 * (1 - 2 * (np.arange(31) % 2))).astype(np.int32)), shift=22),
        "unsharp": dict(kernel=g2, shift=s2, unsharp=1024),
    }
    # the device runs the vertical pass first, so the COLUMN's sum decides its 24-bit or 32-bit horizontal pass:
    # the extreme kernel transposed (a vertical sum at 255 * 32767), a column of exactly 2^15 with A exactly 2^22, a column
    # beyond 2^15 (vertical sums beyond 2^23: the 32-bit form), and a kernel without cancellation at A = 2^22 exactly
    at_bound = np.full(31, 1024, np.int32)
    at_bound[15] = 2048
    out["extreme_transposed"] = dict(kernel=((4 * (1 - 2 * (np.arange(31) % 2))).astype(np.int32), np.full(31, 1057, np.int32)), shift=22)
    out["column_at_bound"] = dict(kernel=(np.array([20, -30, 28, -30, 20], np.int32), at_bound.copy()), shift=22, bias=100)
    out["column_beyond"] = dict(kernel=(np.array([22, -23, 22], np.int32), np.full(31, 2000, np.int32)), shift=20, bias=-60)
    out["full_A"] = dict(kernel=(at_bound.copy(), np.array([128], np.int32)), shift=22)
    for R in (1, 3, 7, 15):
        out["tent%d" % R] = dict(kernel=(tent(R), tent(R)), shift=4 * int(np.log2(R + 1)))
    return out


EXTREME = ("9x9_max", "9x9_alternating", "extreme", "extreme_transposed", "column_at_bound", "column_beyond", "full_A")   # the kernels at the bounds


def everything():
    d = dict(general())
    d.update(separable())
    return d


def refused():
    """[(kernel, the refusal behind the call's name)]"""
    # (no general kernel reaches 2^22: 81 * 32767 is below it.)  2^22 + 1 = 1985 * 2113, a row's sum times a column's
    r, c = np.full(31, 64, np.int32), np.full(31, -68, np.int32)
    r[3] += 1
    c[30] -= 5
    assert int(np.abs(r).sum()) * int(np.abs(c).sum()) == (1 << 22) + 1
    too_much = (r, c)
    row = np.full(31, 1057, np.int32)
    row[0] += 2                  # 32767 + 2 = 2^15 + 1
    assert int(row.sum()) == (1 << 15) + 1
    return [(too_much, ": the weights' absolute sum exceeds 2^22 (separable: the product of the row's and the column's)"),
            ((row, np.array([1], np.int32)), ": the row's absolute sum exceeds 2^15")]


def params(case, edge="border", border=(0, 0, 0)):
    import tiny_renderer_amd as T
    return T.convolve_params(case["kernel"], shift=case.get("shift", 0), bias=case.get("bias", 0), edge=edge, border=border,
                             absolute=case.get("absolute", False), unsharp=case.get("unsharp"))


def weights2d(case):
    k = case["kernel"]
    if isinstance(k, tuple):
        return np.outer(np.asarray(k[1], np.int64), np.asarray(k[0], np.int64))
    return np.asarray(k, np.int64)


def accumulate(rgb, case, edge="border", border=(0, 0, 0)):
    """acc of the rule, int64 [H, W, 3]: the 2-D sum over the padded image."""
    w = weights2d(case)
    kh, kw = w.shape
    Hh, W = rgb.shape[:2]
    F = rgb.astype(np.int64)
    if edge == "clamp":
        P = np.pad(F, ((kh // 2, kh // 2), (kw // 2, kw // 2), (0, 0)), mode="edge")
    else:
        P = np.empty((Hh + kh - 1, W + kw - 1, 3), np.int64)
        P[...] = np.array(border, np.int64)
        P[kh // 2:kh // 2 + Hh, kw // 2:kw // 2 + W] = F
    acc = np.zeros((Hh, W, 3), np.int64)
    for j in range(kh):
        for i in range(kw):
            if w[j, i]:
                acc += w[j, i] * P[j:j + Hh, i:i + W]
    return acc


def rule(rgb, case, edge="border", border=(0, 0, 0)):
    """The rule's text in int64 (numpy's >> on int64 is arithmetic)."""
    acc = accumulate(rgb, case, edge, border)
    shift = case.get("shift", 0)
    v = (acc + ((1 << (shift - 1)) if shift else 0)) >> shift
    if case.get("absolute"):
        v = np.abs(v)
    if case.get("unsharp") is not None:
        F = rgb.astype(np.int64)
        v = np.clip(v, 0, 255)
        return np.clip(F + ((case["unsharp"] * (F - v) + 128) >> 8), 0, 255).astype(np.uint8)
    return np.clip(v + case.get("bias", 0), 0, 255).astype(np.uint8)


def image(kind, W, Hh, seed=0):
    if kind == "noise":
        return _rng(1000 + seed + 7 * W + Hh).integers(0, 256, (Hh, W, 3)).astype(np.uint8)
    return np.full((Hh, W, 3), 255 if kind == "white" else 0, np.uint8)
