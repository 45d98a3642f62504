"""What tests/test_resize_host.py (CPU) and tests/test_resize.py (GPU) share: the rule of the resize stage restated in
Python integers and numpy from its description (one axis: raw taps, the run of positive ones, weights that sum to 4096
by cumulative rounding; the frame: int64 matrix products of the two axes' weight matrices, + 2^23 >> 24), and the sizes."""
import numpy as np

AREA, BILINEAR = 0, 1
FILTERS = ("area", "bilinear")
ONE, MAX_TAPS, MAX_SIDE = 4096, 16, 8192
CAM, LIGHT = 0.3, 0.7
# k_resize's compiled output tiles (width, height): the GPU cases put an output width and height one past a multiple of each
TILES = ((64, 16), (32, 8), (32, 4))


# ... with the rows of horizontal sums each shape holds: the first shape whose rows the vertical table's span fits is taken
TILE_ROWS = (24, 40, 48)
# from 300 x 200: (output size, shape) -- one past a multiple of the shape's tile on both sides
TILE_CASES = (((129, 209), 0), ((97, 65), 1), ((65, 25), 2))


def allowed(n, m):
    return 1 <= m <= MAX_SIDE and m >= -(-n // 8)


def raw(filt, n, m, X, x):
    """o[x] of output index X, a Python integer."""
    if filt == AREA:
        return max(0, min((x + 1) * m, (X + 1) * n) - max(x * m, X * n))
    S, Cc = 2 * max(m, n), (2 * X + 1) * n
    return max(0, S - abs((2 * x + 1) * m - Cc))


def taps(filt, n, m, X):
    """(first, [weights]) of output index X: every source index is asked, nothing is assumed about where the run lies
    beyond a window that is generous on both sides."""
    centre = ((2 * X + 1) * n) // (2 * m)
    reach = 2 * max(1, -(-n // m)) + 3
    xs = [x for x in range(max(0, centre - reach), min(n, centre + reach + 1)) if raw(filt, n, m, X, x) > 0]
    assert xs and xs == list(range(xs[0], xs[0] + len(xs))), "the positive taps form one run"
    assert xs[0] == 0 or xs[0] > centre - reach, "the window cut the run on the left"
    assert xs[-1] == n - 1 or xs[-1] < centre + reach, "the window cut the run on the right"
    o = [raw(filt, n, m, X, x) for x in xs]
    O, cum, before, w = sum(o), 0, 0, []
    for v in o:
        cum += v
        c = (ONE * cum + O // 2) // O
        w.append(c - before)
        before = c
    return xs[0], w


def tables_np(filt, n, m):
    """(first [m], count [m], weights [m, 16]) of a whole axis: `taps` for every X at once in int64 (every intermediate
    is below 2^44), so that all pairs of small sizes can be checked in seconds; test_resize_host.py pins it to `taps`."""
    X = np.arange(m, dtype=np.int64)[:, None]
    reach = 2 * max(1, -(-n // m)) + 3
    x = ((2 * X + 1) * n) // (2 * m) + np.arange(-reach, reach + 1, dtype=np.int64)[None, :]
    if filt == AREA:
        o = np.minimum((x + 1) * m, (X + 1) * n) - np.maximum(x * m, X * n)
    else:
        o = 2 * max(m, n) - np.abs((2 * x + 1) * m - (2 * X + 1) * n)
    o = np.where((x >= 0) & (x < n), np.maximum(o, 0), 0)
    pos = o > 0
    a, count = pos.argmax(1), pos.sum(1)
    assert (count >= 1).all() and (count <= MAX_TAPS).all()
    k = np.arange(MAX_TAPS, dtype=np.int64)[None, :]
    run = np.take_along_axis(o, np.minimum(a[:, None] + k, o.shape[1] - 1), 1) * (k < count[:, None])
    assert (run.sum(1) == o.sum(1)).all(), "the positive taps form one run inside the window"
    inside = np.take_along_axis(x, a[:, None], 1)[:, 0]
    assert ((a > 0) | (inside == 0)).all() and ((a + count < o.shape[1]) | (inside + count == n)).all(), "the window cut a run"
    O = run.sum(1)[:, None]
    c = (ONE * np.cumsum(run, 1) + O // 2) // O
    w = np.diff(c, axis=1, prepend=0) * (k < count[:, None])
    return inside.astype(np.uint16), count.astype(np.uint16), w.astype(np.uint16)


def matrix(filt, n, m):
    """[m, n] int64: row X holds the weights of output index X."""
    first, count, w = tables_np(filt, n, m)
    out = np.zeros((m, n), np.int64)
    for X in range(m):
        out[X, first[X]:first[X] + count[X]] = w[X, :count[X]]
    return out


def filter_id(name):
    return {"area": AREA, "bilinear": BILINEAR}[name]


def resize_np(rgb, width, height, filt):
    """The rule over a frame [H, W, 3] uint8: int64 matrix products, then + 2^23 >> 24.  The largest accumulator is
    asserted to stay below 2^32."""
    f = filter_id(filt) if isinstance(filt, str) else filt
    Hh, W, _ = rgb.shape
    mx, my = matrix(f, W, width), matrix(f, Hh, height)
    inner = np.einsum("Xx,yxc->yXc", mx, rgb.astype(np.int64))
    assert inner.max() <= 255 * ONE
    acc = np.einsum("Yy,yXc->YXc", my, inner) + (1 << 23)
    assert acc.max() < 1 << 32
    return (acc >> 24).astype(np.uint8)


def box(F, f):
    Hh, W, _ = F.shape
    return ((F.reshape(Hh // f, f, W // f, f, 3).astype(np.uint32).sum((1, 3)) + f * f // 2) // (f * f)).astype(np.uint8)


def up8(n):
    return -(-n // 8)


# GPU: the sources (W, H) and, per source, the output sizes
SOURCES = ((132, 17), (640, 480), (1000, 488), (300, 200))


def outputs(W, Hh):
    """Exactly / 8 (rounded up where it does not divide) and that plus one; / 2 and / 4 (rounded up); the same size; W + 1 x
    H - 1; x 2; down in x and up in y; one past a multiple of every compiled tile width and height."""
    out = [(up8(W), up8(Hh)), (up8(W) + 1, up8(Hh) + 1), (-(-W // 2), -(-Hh // 2)), (-(-W // 4), -(-Hh // 4)), (W, Hh),
           (W + 1, Hh - 1), (2 * W, 2 * Hh), (-(-W // 3), Hh + Hh // 2)]
    if (W, Hh) == (300, 200):
        out += [(211, 97)] + [o for o, _ in TILE_CASES]
    if (W, Hh) == (132, 17):
        out.append((1056, 136))
    seen = []
    for o in out:
        if o not in seen:
            seen.append(o)
    return seen


def shape_of(filt, n, m):
    """The shape k_resize runs in for a vertical axis of n source and m output rows, by the rule written beside
    kResizeShapes: the most source rows that a tile's output rows reach over must fit the shape's rows."""
    f = filter_id(filt) if isinstance(filt, str) else filt
    runs = [taps(f, n, m, Y) for Y in range(m)]
    for i, ((_, h), rows) in enumerate(zip(TILES, TILE_ROWS)):
        span = max(runs[min(a + h, m) - 1][0] + len(runs[min(a + h, m) - 1][1]) - runs[a][0] for a in range(0, m, h))
        if span <= rows:
            return i
    return None
