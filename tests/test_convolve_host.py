"""The convolve stage on the host (no GPU): tr_convolve_host against the rule restated in numpy int64 from its text
(tests/convolve_cases.py), the known answers that follow from the rule, the parameter refusals with their full texts and
the kernel builders' taps.  tests/test_convolve.py then pins the device to tr_convolve_host.

The bound.  The issue behind this stage asks that the extreme kernels reach at least half of 2^31 in |acc| on the all-255
image.  No accepted kernel can: A <= 2^22 gives |acc| <= 255 * 2^22 = 1,069,547,520 < 2^30.  What is asserted instead, in
int64, is what the bound allows: 255 * A of every extreme kernel is at least 2^29 (a quarter of 2^31; 676,802,385 for the
9 x 9 kernels, 1,036,092,540 for the separable one), the all-+32767 kernel reaches exactly that |acc| on the white image,
and the separable one's horizontal sum reaches 255 * 32767 = 8,355,585, above half of the 2^23 it must stay below.  A
separable kernel without cancellation at A = 2^22 exactly ("full_A") reaches |acc| = 255 * 2^22, 0.996 of 2^30: the int32
bound at its limit.  The device sums columns first, so the column's sum is exercised the same way: the transposed extreme
and a column of exactly 2^15 reach a vertical sum of at least 2^22, a column beyond 2^15 exceeds 2^23."""
import ctypes as C

import numpy as np
import pytest

from tests import convolve_cases as CC

ALL = CC.everything()


def same(got, want, what):
    assert got.shape == want.shape and np.array_equal(got, want), "%s: %d bytes differ" % (what, int((got != want).sum()))


@pytest.mark.parametrize("name", sorted(ALL))
def test_host_rule_equals_the_text_in_int64(name):
    import tiny_renderer_amd as T
    case = ALL[name]
    for W, Hh in CC.IMAGES:
        for kind in ("noise", "white", "black"):
            img = CC.image(kind, W, Hh)
            for edge, border in CC.EDGES:
                acc = CC.accumulate(img, case, edge, border)
                assert int(np.abs(acc).max()) + (1 << 21) < (1 << 31), "the case itself breaks the bound"
                same(T.convolve_host(img, CC.params(case, edge, border)), CC.rule(img, case, edge, border),
                     "%s %dx%d %s %s %r" % (name, W, Hh, kind, edge, border))


def test_the_extreme_kernels_exercise_the_bound():
    white = CC.image("white", 131, 19)
    for name in CC.EXTREME:
        A = int(np.abs(CC.weights2d(ALL[name])).sum())
        assert A <= 1 << 22 and 255 * A >= 1 << 29, (name, A)
    acc = CC.accumulate(white, ALL["9x9_max"], "clamp")
    assert int(np.abs(acc).max()) == 255 * 81 * 32767 >= 1 << 29
    row = np.asarray(ALL["extreme"]["kernel"][0], np.int64)
    assert int(np.abs(row).sum()) == 32767 and 255 * int(row.sum()) >= 1 << 22 and 255 * int(row.sum()) < 1 << 23
    full = CC.accumulate(white, ALL["full_A"], "clamp")
    assert int(np.abs(full).max()) == 255 * (1 << 22) and int(np.abs(full).max()) + (1 << 21) < 1 << 31
    one = np.array([1], np.int32)
    for name, lo, hi in (("extreme_transposed", 1 << 22, 1 << 23), ("column_at_bound", 1 << 22, 1 << 23), ("column_beyond", (1 << 23) + 1, 1 << 31)):
        row, col = ALL[name]["kernel"]
        assert int(np.abs(row).sum()) <= 1 << 15 and int(np.abs(row).sum()) * int(np.abs(col).sum()) <= 1 << 22, name
        v = int(np.abs(CC.accumulate(white, dict(kernel=(one, col)), "clamp")).max())   # the vertical sum alone
        assert lo <= v < hi, (name, v)
    assert int(np.abs(ALL["column_at_bound"]["kernel"][1]).sum()) == 1 << 15
    assert int(np.abs(ALL["column_at_bound"]["kernel"][0]).sum()) << 15 == 1 << 22
    alt = CC.weights2d(ALL["9x9_alternating"])
    assert 255 * int(alt[alt > 0].sum()) >= 1 << 28, "a partial sum of the alternating kernel is large before it cancels"


def test_known_answers():
    import tiny_renderer_amd as T
    img = CC.image("noise", 37, 23)
    G = CC.general()
    same(T.convolve_host(img, CC.params(G["identity"])), img, "1 x 1 is a copy")
    paper = np.array(CC.PAPER, np.uint8)
    for name, (dx, dy) in (("shift_left", (-1, 0)), ("shift_right", (1, 0)), ("shift_up", (0, -1)), ("shift_down", (0, 1))):
        # a tap of 1 at column i, row j (from the top) shows F(x + i - 1, y + j - 1)
        want = np.empty_like(img)
        want[...] = paper
        ys, xs = np.arange(23)[:, None] + dy, np.arange(37)[None, :] + dx
        ok = (ys >= 0) & (ys < 23) & (xs >= 0) & (xs < 37)
        want[ok] = img[np.clip(ys, 0, 22), np.clip(xs, 0, 36)][ok]
        same(T.convolve_host(img, CC.params(G[name], "border", CC.PAPER)), want, name)
    assert np.array_equal(T.convolve_host(img, CC.params(G["shift_right"]))[:, :-1], img[:, 1:])
    assert np.array_equal(T.convolve_host(img, CC.params(G["shift_down"]))[:-1], img[1:])
    for c in (0, 7, 28, 29, 255):
        flat = np.full((9, 11, 3), c, np.uint8)
        assert (T.convolve_host(flat, CC.params(G["box3"], "clamp")) == min(255, 9 * c)).all()
    for name, case in CC.separable().items():
        row, col = case["kernel"]
        if row.size <= 9 and col.size <= 9:
            outer = dict(case, kernel=np.outer(col, row).astype(np.int32))
            for edge, border in CC.EDGES:
                same(T.convolve_host(img, CC.params(case, edge, border)), T.convolve_host(img, CC.params(outer, edge, border)), name + " as its outer product")
    for R in (1, 3, 7, 15):
        k, shift = T.kernel_tent(R)
        assert shift == 4 * int(np.log2(R + 1)) and np.array_equal(k[0], CC.tent(R))
        same(T.convolve_host(img, T.convolve_params(k, shift=shift)), T.bloom_host(img, T.bloom_params(R, 0, 256, T.scene.BLOOM_GLOW_ONLY)),
             "the tent of radius %d is bloom's glow at threshold 0" % R)
    empty = np.zeros((0, 5, 3), np.uint8)
    assert T.convolve_host(empty, CC.params(G["box3"])).shape == (0, 5, 3)


def test_struct_and_refusals():
    import tiny_renderer_amd as T
    from tiny_renderer_amd import _lib
    L = T.load_library()
    assert C.sizeof(T.ConvolveParams) == 200
    img = CC.image("noise", 8, 6)
    out = np.full_like(img, 0xAA)
    text = lambda: L.tr_last_error().decode()

    def refused(p, why, rgb=img, o=out):
        assert L.tr_convolve_host(8, 6, None if rgb is None else rgb.ctypes.data, None if o is None else o.ctypes.data,
                                  None if p is None else C.addressof(p)) == _lib.TR_E_INVALID
        assert text() == "tr_convolve_host" + why
        assert (out == 0xAA).all()

    def base(**kw):
        p = CC.params(CC.general()["box3"])
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    refused(None, ": null argument")
    refused(base(struct_size=196), ": struct_size is not sizeof(tr_convolve_params)")
    refused(base(flags=8), ": unknown flags")
    for kw in (dict(kw=2), dict(kh=4), dict(kw=11), dict(kh=0)):
        refused(base(**kw), ": kw and kh must be odd and 1..9 (1..31 with TR_CONVOLVE_SEPARABLE)")
    for kw in (dict(kw=33, flags=1), dict(kh=2, flags=1)):
        refused(base(**kw), ": kw and kh must be odd and 1..31 (TR_CONVOLVE_SEPARABLE)")
    refused(base(shift=23), ": shift must be 0..22")
    refused(base(bias=256), ": bias must be -255..255")
    refused(base(bias=-256), ": bias must be -255..255")
    refused(base(amount=1025, flags=4), ": amount must be 0..1024")
    refused(base(amount=1), ": amount must be 0 without TR_CONVOLVE_UNSHARP")
    refused(base(edge=2), ": edge must be TR_CONVOLVE_BORDER or TR_CONVOLVE_CLAMP")
    refused(base(pad=1), ": pad must be 0")
    refused(base(flags=6), ": TR_CONVOLVE_UNSHARP does not go with TR_CONVOLVE_ABS")
    refused(base(flags=4, bias=1), ": TR_CONVOLVE_UNSHARP needs a bias of 0")
    for kernel, why in CC.refused():
        p = T.ConvolveParams(200, kernel[0].size, kernel[1].size, 1, 22, 0, 0, 0, (C.c_uint8 * 3)(), 0)
        for i, v in enumerate(np.concatenate(kernel)):
            p.weights[i] = int(v)
        refused(p, why)
        with pytest.raises(ValueError, match="convolve: the"):
            T.convolve_params(kernel, shift=22)
    ok = base()
    refused(ok, ": null argument", rgb=None)
    refused(ok, ": null argument", o=None)
    refused(ok, ": out is rgb (the rule reads neighbours: not in place)", o=img)
    # the largest sums that pass: A = 2^22 exactly, a row of 2^15 exactly
    r, c = np.full(31, 1024, np.int32), np.full(1, 128, np.int32)
    r[0] += 1024
    assert int(r.sum()) == 1 << 15 and int(r.sum()) * 128 == 1 << 22
    T.convolve_params((r, c), shift=22)
    # entries behind the last one used are not read
    p = base()
    for i in range(9, 82):
        p.weights[i] = -32768
    same(T.convolve_host(img, p), T.convolve_host(img, base()), "weights behind the kernel")
    for bad in (dict(kernel=np.ones((2, 3), np.int32)), dict(kernel=np.ones((3, 3))), dict(kernel=np.ones((3, 3), np.int32), shift=23),
                dict(kernel=np.ones((3, 3), np.int32), edge="mirror"), dict(kernel=np.full((3, 3), 40000, np.int32)),
                dict(kernel=np.ones((3, 3), np.int32), unsharp=256, absolute=True), dict(kernel=(np.ones(33, np.int32), np.ones(1, np.int32)))):
        with pytest.raises(ValueError):
            T.convolve_params(**bad)


def test_builders_sum_to_a_power_of_two_and_are_symmetric():
    import tiny_renderer_amd as T
    flat = np.full((40, 45, 3), 0, np.uint8)
    flat[...] = (3, 128, 255)
    for label, (k, shift) in (("gaussian 0.8", T.kernel_gaussian(0.8)), ("gaussian 2", T.kernel_gaussian(2.0)), ("gaussian 5/15", T.kernel_gaussian(5.0, 15)),
                              ("gaussian 40", T.kernel_gaussian(40.0)), ("box", T.kernel_box(3, 1)), ("box 15", T.kernel_box(15, 15)), ("box 0", T.kernel_box(0, 0)),
                              ("tent 2", T.kernel_tent(2)), ("tent 7", T.kernel_tent(7)), ("tent 0", T.kernel_tent(0)),
                              ("motion x", T.kernel_motion(9)), ("motion y", T.kernel_motion(31, False))):
        row, col = k
        assert row.dtype.kind == "i" and int(row.sum()) * int(col.sum()) == 1 << shift, label
        assert np.array_equal(row, row[::-1]) and np.array_equal(col, col[::-1]) and row.min() >= 0 and col.min() >= 0, label
        # (cumulative rounding keeps every tap within 1 of its exact value: a rising flank may step back by 1, no more)
        assert (np.diff(row[:row.size // 2]) >= -1).all(), label
        same(T.convolve_host(flat, T.convolve_params(k, shift=shift, edge="clamp")), flat, label + " keeps a flat colour")
    assert T.kernel_gaussian(5.0)[0][0].size == 31 and T.kernel_gaussian(0.5)[0][0].size == 5 and T.kernel_motion(9)[0][1].size == 1
    for axis in ("x", "y"):
        k, shift = T.kernel_sobel(axis)
        assert shift == 0 and k.shape == (3, 3) and int(k.sum()) == 0
    assert np.array_equal(T.kernel_sobel("y")[0], T.kernel_sobel("x")[0].T) and np.array_equal(T.kernel_sobel("x")[0][:, 0], [-1, -2, -1])
    lap, _ = T.kernel_laplacian()
    assert int(lap.sum()) == 0 and np.array_equal(lap, lap.T) and np.array_equal(lap, lap[::-1])
    emb, _ = T.kernel_emboss()
    assert int(emb.sum()) == 0 and np.array_equal(emb, -emb[::-1, ::-1])
    ramp = np.zeros((9, 12, 3), np.uint8)
    ramp[...] = (np.arange(12, dtype=np.uint8) * 10)[None, :, None]
    assert (T.convolve_host(ramp, T.convolve_params(T.kernel_sobel("x")[0], edge="clamp"))[:, 1:-1] == 80).all()
    assert not T.convolve_host(ramp, T.convolve_params(T.kernel_sobel("y")[0], edge="clamp", absolute=True)).any()
    assert not T.convolve_host(ramp, T.convolve_params(lap, edge="clamp", absolute=True))[:, 1:-1].any()
