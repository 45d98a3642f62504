"""What tests/test_warp_host.py (CPU) and tests/test_warp.py (GPU) share: the rule of the warp stage restated from its
description -- once in plain Python integers, pixel by pixel (`rule`), once in numpy int64 for whole frames (`rule_np`;
the CPU file pins the two to each other) -- and the grids and sizes of the GPU cases."""
import numpy as np

CELL, NODE_MAX, BORDER, CLAMP = 16, 1 << 22, 0, 1
CAM, LIGHT = 0.3, 0.7
# GPU: a width that is no multiple of 4 with one partial tile row and two tile columns; flagged and unflagged tiles; the smallest
SOURCES = ((134, 21), (640, 480), (8, 8))
PAPER = (200, 30, 90)   # a border that is not black


def grid_shape(w, h):
    return (h + 15) // 16 + 1, (w + 15) // 16 + 1


def outputs(W, Hh):
    """The frame's own size, one pixel, a partial cell in both directions, a multiple of 16 and one past it."""
    return [(W, Hh), (1, 1), (17, 33), (160, 48), (161, 47)]


def _texel(F, x, y, c, edge, border):
    Hh, W, _ = F.shape
    if edge == CLAMP:
        x, y = min(max(x, 0), W - 1), min(max(y, 0), Hh - 1)
    elif not (0 <= x < W and 0 <= y < Hh):
        return int(border[c])
    return int(F[y, x, c])


def rule(F, grid, w, h, edge=BORDER, border=(0, 0, 0)):
    """The rule in Python integers.  grid: [n, gh, gw, 2] with n = 1 or 3."""
    g = np.asarray(grid)
    g = g[None] if g.ndim == 3 else g
    out = np.zeros((h, w, 3), np.uint8)
    for Y in range(h):
        for X in range(w):
            gx, fx, gy, fy = X >> 4, X & 15, Y >> 4, Y & 15
            for c in range(3):
                n = g[c if g.shape[0] == 3 else 0]
                s = []
                for k in (0, 1):
                    n00, n10, n01, n11 = (int(n[gy + j, gx + i, k]) for j, i in ((0, 0), (0, 1), (1, 0), (1, 1)))
                    v = (16 - fx) * (16 - fy) * n00 + fx * (16 - fy) * n10 + (16 - fx) * fy * n01 + fx * fy * n11 + 128
                    assert -(1 << 31) <= v < 1 << 31
                    s.append(v >> 8)          # (Python's >> floors)
                ix, ax, iy, ay = s[0] >> 8, s[0] & 255, s[1] >> 8, s[1] & 255
                acc = ((256 - ax) * (256 - ay) * _texel(F, ix, iy, c, edge, border) + ax * (256 - ay) * _texel(F, ix + 1, iy, c, edge, border)
                       + (256 - ax) * ay * _texel(F, ix, iy + 1, c, edge, border) + ax * ay * _texel(F, ix + 1, iy + 1, c, edge, border) + (1 << 15))
                assert acc < 1 << 32
                out[Y, X, c] = acc >> 16
    return out


def rule_np(F, grid, w, h, edge=BORDER, border=(0, 0, 0)):
    """The same over whole frames in int64."""
    g = np.asarray(grid, np.int64)
    g = g[None] if g.ndim == 3 else g
    Hh, W, _ = F.shape
    Y, X = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    gx, fx, gy, fy = X >> 4, X & 15, Y >> 4, Y & 15
    out = np.zeros((h, w, 3), np.uint8)
    for c in range(3):
        n = g[c if g.shape[0] == 3 else 0]
        s = ((16 - fx)[..., None] * (16 - fy)[..., None] * n[gy, gx] + fx[..., None] * (16 - fy)[..., None] * n[gy, gx + 1]
             + (16 - fx)[..., None] * fy[..., None] * n[gy + 1, gx] + fx[..., None] * fy[..., None] * n[gy + 1, gx + 1] + 128) >> 8
        ix, ax, iy, ay = s[..., 0] >> 8, s[..., 0] & 255, s[..., 1] >> 8, s[..., 1] & 255

        def T(x, y):
            v = F[np.clip(y, 0, Hh - 1), np.clip(x, 0, W - 1), c].astype(np.int64)
            if edge == CLAMP:
                return v
            return np.where((x >= 0) & (x < W) & (y >= 0) & (y < Hh), v, int(border[c]))
        acc = (256 - ax) * (256 - ay) * T(ix, iy) + ax * (256 - ay) * T(ix + 1, iy) + (256 - ax) * ay * T(ix, iy + 1) + ax * ay * T(ix + 1, iy + 1)
        out[..., c] = (acc + (1 << 15)) >> 16
    return out


def nodes(f, w, h):
    """int32 [gh, gw, 2] from f(X, Y) -> (sx, sy) in source pixels, by the builders' rounding: floor(256 v + 0.5), clipped."""
    gh, gw = grid_shape(w, h)
    Y, X = np.meshgrid(np.arange(gh) * 16.0, np.arange(gw) * 16.0, indexing="ij")
    sx, sy = f(X, Y)
    g = np.stack([sx + 0 * X, sy + 0 * X], -1)
    return np.clip(np.floor(256.0 * g + 0.5), -NODE_MAX, NODE_MAX).astype(np.int32)


def grids(W, Hh, w, h):
    """{name: grid} for a W x Hh source and a w x h output: [gh, gw, 2], or [3, gh, gw, 2] for "chromatic"."""
    ax, ay = W / float(w), Hh / float(h)
    cxo, cyo, cxs, cys = (w - 1) / 2.0, (h - 1) / 2.0, (W - 1) / 2.0, (Hh - 1) / 2.0
    c7, s7 = np.cos(np.radians(7.0)), np.sin(np.radians(7.0))

    def lens(X, Y):
        u, v = (X - cxo) / max(w / 2.0, 1.0), (Y - cyo) / max(h / 2.0, 1.0)
        r2 = u * u + v * v
        m = 1.0 - 0.18 * r2 + 0.03 * r2 * r2
        return cxs + u * m * W / 2.0, cys + v * m * Hh / 2.0

    def far(X, Y):
        # the right part of the output 12000 pixels to the right, the lower part 9000 above: wholly outside and, in the
        # cells between, footprints that span the whole image
        return X * ax + np.where(X > w / 2.0, 12000.0, 0.0), Y * ay - np.where(Y > h / 2.0, 9000.0, 0.0)

    def scaled(m):
        return lambda X, Y: (cxs + (X - cxo) * ax * m, cys + (Y - cyo) * ay * m)
    return {
        "identity": nodes(lambda X, Y: (X, Y), w, h),
        "flip": nodes(lambda X, Y: (W - 1 - X, Y), w, h),
        "rotate7": nodes(lambda X, Y: (cxs + c7 * (X - cxo) * ax - s7 * (Y - cyo) * ay, cys + s7 * (X - cxo) * ax + c7 * (Y - cyo) * ay), w, h),
        "lens": nodes(lens, w, h),
        "chromatic": np.stack([nodes(scaled(m), w, h) for m in (0.97, 1.0, 1.03)]),
        "far": nodes(far, w, h),
    }
