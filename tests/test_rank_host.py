"""The rank stage on the host (no GPU): tr_rank_host against the rule restated in numpy from its text
(tests/rank_cases.py: pad, gather, np.sort, index), the known answers that follow from the rule, the footprint builders
and the parameter refusals with their full texts.  tests/test_rank.py then pins the device to tr_rank_host.  Every
comparison is np.array_equal."""
import ctypes as C

import numpy as np
import pytest

from tests import rank_cases as RC

ALL = RC.everything()


def same(got, want, what):
    assert got.shape == want.shape and np.array_equal(got, want), "%s: %d bytes differ" % (what, int((got != want).sum()))


def value(T, img, f, rank, edge="border", border=(0, 0, 0)):
    return T.rank_host(img, T.rank_params(f, rank, edge=edge, border=border))


@pytest.mark.parametrize("name", sorted(ALL))
def test_host_rule_equals_the_text(name):
    """Noise and white force ties (white everywhere, noise in the large footprints: 225 taps of 256 values)."""
    import tiny_renderer_amd as T
    case = ALL[name]
    for W, Hh in RC.IMAGES:
        imgs = [RC.image(kind, W, Hh) for kind in ("noise", "white")] + ([RC.planted(W, Hh)[0]] if W >= 7 and Hh >= 5 else [])
        for k, img in enumerate(imgs):
            for edge, border in RC.EDGES:
                same(T.rank_host(img, RC.params(case, edge, border)), RC.rule(img, case, edge, border), "%s %dx%d image %d %s %r" % (name, W, Hh, k, edge, border))


def test_known_answers():
    import tiny_renderer_amd as T
    img = RC.image("noise", 37, 23)
    F = RC.footprints()
    same(value(T, img, F["1x1"], 0), img, "one centre tap is a copy")
    paper = np.array(RC.PAPER, np.uint8)
    for name, (dx, dy) in (("tap_left", (-1, 0)), ("tap_right", (1, 0)), ("tap_up", (0, -1)), ("tap_down", (0, 1)), ("tap_far", (-2, 3))):
        # a tap at column i, row j (from the top) of a kw x kh box shows F(x + i - kw / 2, y + j - kh / 2)
        want = np.empty_like(img)
        want[...] = paper
        ys, xs = np.arange(23)[:, None] + dy, np.arange(37)[None, :] + dx
        ok = (ys >= 0) & (ys < 23) & (xs >= 0) & (xs < 37)
        want[ok] = img[np.clip(ys, 0, 22), np.clip(xs, 0, 36)][ok]
        same(value(T, img, F[name], 0, "border", RC.PAPER), want, name)
    assert np.array_equal(value(T, img, F["tap_right"], 0)[:, :-1], img[:, 1:]) and np.array_equal(value(T, img, F["tap_down"], 0)[:-1], img[1:])
    for c in (0, 7, 255):
        flat = np.full((9, 11, 3), c, np.uint8)
        for name, case in ALL.items():
            got = T.rank_host(flat, RC.params(case, "clamp"))
            assert (got == (0 if case.get("op") == "range" else c)).all(), (name, c)
    empty = np.zeros((0, 5, 3), np.uint8)
    assert T.rank_host(empty, RC.params(ALL["3x3_rank4"])).shape == (0, 5, 3)


def test_salt_and_pepper_is_removed_exactly():
    import tiny_renderer_amd as T
    speckled, ramp = RC.planted(64, 40)
    assert int((speckled != ramp).any(-1).sum()) > 30
    square = T.footprint_rect(3, 3)
    same(T.rank_host(speckled, T.rank_params(square, "median", edge="clamp")), ramp, "the 3 x 3 median")
    despeckle = T.rank_params(square, 1, 7, op="clamp_centre", edge="clamp")
    same(T.rank_host(speckled, despeckle), ramp, "despeckle")
    same(T.rank_host(ramp, despeckle), ramp, "despeckle leaves the clean ramp alone")
    noise = RC.image("noise", 31, 17)
    changed = T.rank_host(noise, despeckle) != noise
    assert changed.any() and not changed.all()


def test_complement_duality():
    """Rank k of F equals 255 - rank (n - 1 - k) of (255 - F), with the border complemented."""
    import tiny_renderer_amd as T
    img = RC.image("noise", 29, 21)
    for name in ("3x3", "disc3", "L", "hollow", "15x1"):
        f = RC.footprints()[name]
        n = int(f.sum())
        for k in sorted({0, 1, (n - 1) // 2, n - 1}):
            for edge, border in RC.EDGES:
                inv = tuple(255 - v for v in border)
                same(value(T, img, f, k, edge, border), 255 - value(T, 255 - img, f, n - 1 - k, edge, inv), "%s rank %d %s" % (name, k, edge))


def test_rectangles_separate_at_the_extremes():
    """min and max over a full kw x kh rectangle equal the kw x 1 call followed by the 1 x kh call, under either edge mode
    (a border colour enters both passes, and the minimum or maximum with it is idempotent)."""
    import tiny_renderer_amd as T
    img = RC.image("noise", 33, 20)
    for kw, kh in ((3, 3), (5, 3), (3, 7), (15, 15)):
        for which in ("min", "max"):
            for edge, border in RC.EDGES:
                whole = value(T, img, T.footprint_rect(kw, kh), which, edge, border)
                rows = value(T, img, T.footprint_rect(kw, 1), which, edge, border)
                same(value(T, rows, T.footprint_rect(1, kh), which, edge, border), whole, "%dx%d %s %s %r" % (kw, kh, which, edge, border))


def test_mid_and_range_from_two_values():
    import tiny_renderer_amd as T
    img = RC.image("noise", 30, 18)
    for name in ("gradient3", "range_inner", "mid_extremes", "mid_inner", "mid_mixed", "two_mid"):
        case = ALL[name]
        for edge, border in RC.EDGES:
            lo = value(T, img, case["footprint"], case["rank"], edge, border).astype(np.int64)
            hi = value(T, img, case["footprint"], case["rank2"], edge, border).astype(np.int64)
            assert (lo <= hi).all()
            want = hi - lo if case["op"] == "range" else (lo + hi + 1) >> 1
            same(T.rank_host(img, RC.params(case, edge, border)), want.astype(np.uint8), name)


def test_builders():
    import tiny_renderer_amd as T
    assert [int(T.footprint_disc(r).sum()) for r in range(8)] == [1, 9, 21, 37, 69, 97, 137, 177]
    assert [int(T.footprint_cross(r).sum()) for r in range(8)] == [4 * r + 1 for r in range(8)]
    assert T.footprint_rect(5, 3).shape == (3, 5) and T.footprint_rect(5, 3).all()
    assert T.footprint_disc(1).all() and T.footprint_disc(1).shape == (3, 3), "1 + 1 <= 1 + 1: the corners are taps"
    assert np.array_equal(T.footprint_disc(2), np.array([[0, 1, 1, 1, 0], [1, 1, 1, 1, 1], [1, 1, 1, 1, 1], [1, 1, 1, 1, 1], [0, 1, 1, 1, 0]], bool))
    assert np.array_equal(T.footprint_cross(1), np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], bool))
    d = T.footprint_disc(3)
    assert np.array_equal(d, d.T) and np.array_equal(d, d[::-1]) and not d[0, 0] and not d[0, 1] and d[0, 2]
    assert np.array_equal(T.footprint_line(5, 0.0), np.ones((1, 5), bool)) and np.array_equal(T.footprint_line(5, 90.0), np.ones((5, 1), bool))
    assert np.array_equal(T.footprint_line(3, 45.0), np.array([[0, 0, 1], [0, 1, 0], [1, 0, 0]], bool)), "counter-clockwise as the picture is seen"
    line = T.footprint_line(9, 30.0)
    assert line.shape == (5, 7) and int(line.sum()) == 9 and np.array_equal(line, line[::-1, ::-1]) and line[0, 6] and line[4, 0]
    # a disc dilates a single bright pixel into itself, a cross erodes a hole into itself
    dot = np.zeros((9, 9, 3), np.uint8)
    dot[4, 4] = 200
    assert np.array_equal(T.rank_host(dot, T.rank_params(d, "max"))[..., 0] != 0, np.pad(d, 1))
    hole = 255 - dot
    assert np.array_equal(T.rank_host(hole, T.rank_params(T.footprint_cross(2), "min", edge="clamp"))[..., 0] != 255, np.pad(T.footprint_cross(2), 2))
    p = T.rank_params(d, "median")
    assert (p.rank, p.rank2, p.kw, p.kh) == (18, 0, 7, 7) and list(p.rows[:8]) == [0x1C, 0x3E, 0x7F, 0x7F, 0x7F, 0x3E, 0x1C, 0]
    assert T.rank_params(d, "max").rank == 36 and T.rank_params(d, "min", "max", op="range").rank2 == 36
    for bad in (lambda: T.footprint_rect(2, 3), lambda: T.footprint_rect(17, 1), lambda: T.footprint_disc(8), lambda: T.footprint_cross(-1),
                lambda: T.footprint_line(4, 0), lambda: T.footprint_line(17, 0)):
        with pytest.raises(ValueError):
            bad()


def test_struct_and_refusals():
    import tiny_renderer_amd as T
    from tiny_renderer_amd import _lib
    L = T.load_library()
    assert C.sizeof(T.RankParams) == 64 and T.RankParams.rows.offset == 32 and T.RankParams.pad2.offset == 62
    img = RC.image("noise", 8, 6)
    out = np.full_like(img, 0xAA)
    text = lambda: L.tr_last_error().decode()

    def refused(p, why, rgb=img, o=out):
        assert L.tr_rank_host(8, 6, None if rgb is None else rgb.ctypes.data, None if o is None else o.ctypes.data,
                              None if p is None else C.addressof(p)) == _lib.TR_E_INVALID
        assert text() == "tr_rank_host" + why
        assert (out == 0xAA).all()

    def base(**kw):
        p = RC.params(ALL["3x3_rank4"])
        for k, v in kw.items():
            if k.startswith("row"):
                p.rows[int(k[3:])] = v
            else:
                setattr(p, k, v)
        return p

    refused(None, ": null argument")
    refused(base(struct_size=60), ": struct_size is not sizeof(tr_rank_params)")
    for kw in (dict(kw=2), dict(kh=4), dict(kw=17), dict(kh=0)):
        refused(base(**kw), ": kw and kh must be odd and 1..15")
    for kw in (dict(row0=0xF), dict(row3=1), dict(row14=1), dict(kw=1)):
        refused(base(**kw), ": footprint bits outside the kw x kh box")
    refused(base(row0=0, row1=0, row2=0), ": the footprint is empty")
    refused(base(op=4), ": op must be TR_RANK_VALUE, TR_RANK_RANGE, TR_RANK_MID or TR_RANK_CLAMP_CENTRE")
    refused(base(edge=2), ": edge must be TR_RANK_BORDER or TR_RANK_CLAMP")
    refused(base(pad=1), ": pad and pad2 must be 0")
    refused(base(pad2=1), ": pad and pad2 must be 0")
    refused(base(rank=9), ": rank and rank2 must be below the number of taps")
    refused(base(op=1, rank2=9), ": rank and rank2 must be below the number of taps")
    refused(base(row1=0b101, rank=8), ": rank and rank2 must be below the number of taps")
    refused(base(rank2=1), ": rank2 must be 0 under TR_RANK_VALUE")
    for op in (1, 2, 3):
        refused(base(op=op, rank=5, rank2=4), ": rank must not exceed rank2")
    ok = base()
    refused(ok, ": null argument", rgb=None)
    refused(ok, ": null argument", o=None)
    refused(ok, ": out is rgb (the rule reads neighbours: not in place)", o=img)
    # what passes at the ends: the last rank, equal ranks, every bit of the largest box
    T.rank_host(img, base(rank=8)), T.rank_host(img, base(op=3, rank=8, rank2=8))
    assert T.rank_params(T.footprint_rect(15, 15), 224).rows[14] == 0x7FFF
    for bad, match in ((dict(footprint=np.ones((2, 3), bool)), "odd"), (dict(footprint=np.ones((3, 3))), "2-D"), (dict(footprint=np.ones((3, 17), bool)), "odd"),
                       (dict(footprint=np.zeros((3, 3), bool)), "rank: the footprint is empty"), (dict(footprint=np.ones((3, 3), bool), rank=9), "rank: rank and rank2"),
                       (dict(footprint=np.ones((3, 3), bool), rank="mean"), "median"), (dict(footprint=np.ones((3, 3), bool), edge="mirror"), "edge"),
                       (dict(footprint=np.ones((3, 3), bool), op="mean"), "op"), (dict(footprint=np.ones((3, 3), bool), rank=1, rank2=2), "rank: rank2 must be 0"),
                       (dict(footprint=np.ones((3, 3), bool), rank=3, rank2=2, op="mid"), "rank: rank must not exceed"), (dict(footprint=np.ones((3, 3), bool), border=(0, 0, 256)), "border")):
        with pytest.raises(ValueError, match=match):
            T.rank_params(**bad)
    with pytest.raises(ValueError):
        T.rank_host(img, T.convolve_params(np.ones((3, 3), np.int32)))
