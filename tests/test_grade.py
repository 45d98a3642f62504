"""Colour grading: tr_scene_set_lut / tr_scene_grade / tr_scene_get_graded (k_grade) and tr_grade_host against the rule in
numpy.

The rule, from the words of include/tiny_renderer.h, for a table of n^3 rgb8 entries (red fastest) and a pixel's stored
channels v: p = v * (n - 1), i = p // 255, f = p % 255, j = min(i + 1, n - 1) per channel; the channels ordered by f,
largest first (a, b, c); V0 = entry(i_r, i_g, i_b), V1 = V0 with channel a stepped to j_a, V2 = V1 with channel b stepped
to j_b, V3 = entry(j_r, j_g, j_b); out = ((255 - f_a) V0 + (f_a - f_b) V1 + (f_b - f_c) V2 + f_c V3 + 127) // 255.  The
contract is exact: every comparison is np.array_equal.

On the CPU tr_grade_host is pinned against that restatement, written as the six-case comparison chain (the library sorts).
On the GPU the expectation is tr_grade_host applied to a snapshot of the very frame that is then rendered again (so that
its flags are fresh) and graded; every case first asserts ON THE EXPECTATION that a byte changes."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import helpers as H
from tests import test_composite as TC

from tiny_renderer_amd import grade_host, lut_identity   # without the feature every case fails here

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32_MIN_BITS = np.uint32(0xFF7FFFFF)
bits, drive, scene, snap, clean_flags, tiles_any = TC.bits, TC.drive, TC.scene, TC.snap, TC.clean_flags, TC.tiles_any


# ------------------------------------------------------------------------------------------------------------------
# The rule in numpy
# ------------------------------------------------------------------------------------------------------------------

def rule(rgb, lut):
    """The rule by the comparison chain over uint8 [..., 3] colours and a table [n, n, n, 3] indexed [b][g][r]."""
    n = lut.shape[0]
    v = np.asarray(rgb).reshape(-1, 3).astype(np.int64)
    T = lut.astype(np.int64)
    p = v * (n - 1)
    i, f = p // 255, p % 255
    j = np.minimum(i + 1, n - 1)
    fr, fg, fb = f[:, 0], f[:, 1], f[:, 2]
    entry = lambda r, g, b: T[b, g, r]
    ir, ig, ib, jr, jg, jb = i[:, 0], i[:, 1], i[:, 2], j[:, 0], j[:, 1], j[:, 2]
    V0, V3 = entry(ir, ig, ib), entry(jr, jg, jb)
    out = np.zeros_like(v)
    done = np.zeros(len(v), bool)
    # (condition, V1, V2, the fractions largest first)
    chain = [((fr >= fg) & (fg >= fb), entry(jr, ig, ib), entry(jr, jg, ib), (fr, fg, fb)),
             ((fr >= fg) & (fg < fb) & (fr >= fb), entry(jr, ig, ib), entry(jr, ig, jb), (fr, fb, fg)),
             ((fr >= fg) & (fg < fb) & (fr < fb), entry(ir, ig, jb), entry(jr, ig, jb), (fb, fr, fg)),
             ((fr < fg) & (fb >= fg), entry(ir, ig, jb), entry(ir, jg, jb), (fb, fg, fr)),
             ((fr < fg) & (fb < fg) & (fb >= fr), entry(ir, jg, ib), entry(ir, jg, jb), (fg, fb, fr)),
             ((fr < fg) & (fb < fg) & (fb < fr), entry(ir, jg, ib), entry(jr, jg, ib), (fg, fr, fb))]
    for cond, V1, V2, (fa, fm, fc) in chain:
        assert not (cond & done).any()
        num = ((255 - fa)[:, None] * V0 + (fa - fm)[:, None] * V1 + (fm - fc)[:, None] * V2 + fc[:, None] * V3 + 127)
        assert not cond.any() or (num[cond].max() <= 255 * 255 + 127 and num[cond].min() >= 0)
        out[cond] = (num // 255)[cond]
        done |= cond
    assert done.all()
    return out.astype(np.uint8).reshape(np.asarray(rgb).shape)


def random_lut(n, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, n, n, 3), dtype=np.uint8)


def lut_c0(n, c0, seed):
    t = random_lut(n, seed)
    t[0, 0, 0] = c0
    return t


def tied_colours(n, count, seed):
    """Colours with two or three equal fractions under a table of edge n: channels that share a value, and (where n - 1
    divides 255) channels that differ by whole cells."""
    rng = np.random.default_rng(seed)
    a, b = rng.integers(0, 256, count), rng.integers(0, 256, count)
    kind = np.arange(count) % 4
    out = np.stack([np.where(kind == 2, b, a), np.where(kind == 1, b, a), np.where(kind == 0, b, a)], -1)
    if 255 % (n - 1) == 0:
        cell = 255 // (n - 1)
        base = rng.integers(0, cell, count // 2)
        out[:count // 2] = rng.integers(0, n - 1, (count // 2, 3)) * cell + base[:, None]
    out = out.astype(np.uint8)
    f = (out.astype(np.int64) * (n - 1)) % 255
    assert ((f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 0] == f[:, 2])).all()
    return out


# ------------------------------------------------------------------------------------------------------------------
# CPU
# ------------------------------------------------------------------------------------------------------------------

def test_entry_points_declared_exported_and_typed(built):
    import tiny_renderer_amd as T
    from tiny_renderer_amd import _lib
    header = open(os.path.join(REPO, "include", "tiny_renderer.h")).read()
    assert re.search(r"int\s+tr_scene_set_lut\(tr_scene \*s, uint32_t n, const uint8_t \*lut", header)
    assert re.search(r"int\s+tr_scene_grade\(tr_scene \*s, void \*out", header)
    assert re.search(r"int\s+tr_scene_get_graded\(tr_scene \*s, uint8_t \*rgb\);", header)
    assert re.search(r"int\s+tr_grade_host\(size_t n_pixels, const uint8_t \*rgb, uint8_t \*out", header)
    for word in ("#define TR_GRADE_MAX_N 33", "#define TR_ABI_VERSION 3"):
        assert word in header, word
    exports = open(os.path.join(REPO, "tiny_renderer_amd", "csrc", "exports.map")).read()
    assert re.search(r"global:\s*tr_\*;", exports)
    raw = C.CDLL(_lib.library_path())
    for name in ("tr_scene_set_lut", "tr_scene_grade", "tr_scene_get_graded", "tr_grade_host"):
        assert hasattr(raw, name), name + " is not exported"
        assert name in _lib.SYMBOLS
    assert _lib.SYMBOLS["tr_scene_set_lut"] == (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p])
    assert _lib.SYMBOLS["tr_scene_grade"] == (C.c_int, [C.c_void_p, C.c_void_p])
    assert _lib.SYMBOLS["tr_scene_get_graded"] == (C.c_int, [C.c_void_p, C.c_void_p])
    assert _lib.SYMBOLS["tr_grade_host"] == (C.c_int, [C.c_size_t, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p])
    assert T.load_library().tr_abi_version() == 3
    for name in ("grade_host", "lut_identity", "lut_from_function", "load_cube"):
        assert hasattr(T, name) and name in T.__all__, name
    assert callable(T.Scene.set_lut) and callable(T.Scene.grade) and callable(T.Scene.get_graded)


def test_every_refusal_on_the_host(built):
    import tiny_renderer_amd as T
    from tiny_renderer_amd import _lib
    L = T.load_library()
    lut = random_lut(34, 1)
    rgb, out = np.zeros((4, 3), np.uint8), np.zeros((4, 3), np.uint8)
    ok = lambda code: code == 0
    bad = lambda code, word=b"": code == _lib.TR_E_INVALID and word in L.tr_last_error() and L.tr_last_error()
    assert ok(L.tr_grade_host(4, rgb.ctypes.data, out.ctypes.data, 2, lut.ctypes.data))
    assert ok(L.tr_grade_host(4, rgb.ctypes.data, out.ctypes.data, 33, lut.ctypes.data))
    for n in (0, 1, 34, 0xFFFFFFFF):
        assert bad(L.tr_grade_host(4, rgb.ctypes.data, out.ctypes.data, n, lut.ctypes.data), b"2..TR_GRADE_MAX_N"), n
        assert bad(L.tr_scene_set_lut(None, n, lut.ctypes.data), b"null"), n
    assert bad(L.tr_grade_host(4, None, out.ctypes.data, 2, lut.ctypes.data), b"null")
    assert bad(L.tr_grade_host(4, rgb.ctypes.data, None, 2, lut.ctypes.data), b"null")
    assert bad(L.tr_grade_host(4, rgb.ctypes.data, out.ctypes.data, 2, None), b"null")
    assert ok(L.tr_grade_host(0, None, None, 2, lut.ctypes.data))
    assert bad(L.tr_scene_set_lut(None, 0, None), b"null")
    assert bad(L.tr_scene_grade(None, None), b"null")
    assert bad(L.tr_scene_get_graded(None, out.ctypes.data), b"null")
    # python: ValueError before anything reaches the library
    good = random_lut(3, 2)
    for table in (good.astype(np.int32), good.astype(np.float32), good[..., :2], good[:2], good.reshape(-1), random_lut(34, 3)[:34],
                  np.zeros((1, 1, 1, 3), np.uint8), good.tolist(), None):
        with pytest.raises(ValueError):
            T.grade_host(rgb, table)
    for px in (rgb.astype(np.int16), rgb.astype(np.float32), np.zeros((4, 2), np.uint8), np.zeros((), np.uint8), rgb.tolist()):
        with pytest.raises(ValueError):
            T.grade_host(px, good)
    s = T.Scene.__new__(T.Scene)
    s.width, s.height, s._h, s._pinned = 64, 64, None, []
    for table in (good.astype(np.float64), good[..., :2], np.zeros((34, 34, 34, 3), np.uint8), np.zeros((1, 1, 1, 3), np.uint8), [1, 2]):
        with pytest.raises(ValueError):
            s.set_lut(table)
    with pytest.raises(ValueError):
        s.grade(out=np.zeros((3, 3, 3), np.uint8))
    for n in (1, 34, 2.0, True):
        with pytest.raises(ValueError):
            T.lut_identity(n)
        with pytest.raises(ValueError):
            T.lut_from_function(n, lambda v: v)
    with pytest.raises(ValueError):
        T.lut_from_function(4, lambda v: v[..., :2])


@pytest.mark.parametrize("n", [2, 3, 17, 25, 26, 33])
def test_host_rule_equals_the_numpy_rule(built, n):
    lut = random_lut(n, 100 + n)
    rng = np.random.default_rng(n)
    corners = np.array([0, 1, 127, 128, 254, 255], np.uint8)
    sets = {"random": rng.integers(0, 256, (50000, 3), dtype=np.uint8),
            "greys": np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, 1),
            "corners": np.stack(np.meshgrid(corners, corners, corners, indexing="ij"), -1).reshape(-1, 3),
            "tied": tied_colours(n, 5000, n)}
    assert len(sets["corners"]) == 216
    keep_lut = lut.copy()
    for name, px in sets.items():
        keep = px.copy()
        want = rule(px, lut)
        got = grade_host(px, lut)
        assert got.dtype == np.uint8 and got.shape == px.shape
        assert np.array_equal(got, want), "%s: %d bytes differ" % (name, int((got != want).sum()))
        assert np.array_equal(px, keep) and np.array_equal(lut, keep_lut), "the arguments are left alone"
        assert not np.array_equal(got, px)
    # in place: out == rgb
    import tiny_renderer_amd as T
    px = sets["random"].copy()
    assert T.load_library().tr_grade_host(len(px), px.ctypes.data, px.ctypes.data, n, lut.ctypes.data) == 0
    assert np.array_equal(px, rule(sets["random"], lut))
    # an image-shaped argument
    img = sets["random"][:35].reshape(5, 7, 3)
    assert np.array_equal(grade_host(img, lut), rule(img, lut))


def test_table_facts(built):
    every = np.stack(np.meshgrid(np.arange(256), np.arange(0, 256, 5), np.arange(0, 256, 15), indexing="ij"), -1).reshape(-1, 3).astype(np.uint8)
    every = np.concatenate([every, every[:, [1, 2, 0]], every[:, [2, 0, 1]]])      # all of 0..255 in each channel
    for c in range(3):
        assert len(np.unique(every[:, c])) == 256
    for n in (2, 4, 6, 16, 18):
        assert 255 % (n - 1) == 0
        assert np.array_equal(grade_host(every, lut_identity(n)), every), "identity at n = %d" % n
    for n in (17, 33):
        got = grade_host(every, lut_identity(n)).astype(np.int64)
        assert np.abs(got - every).max() <= 1, "within one where n - 1 does not divide 255 (equality is not promised there)"
    inv = (255 - lut_identity(2)).astype(np.uint8)
    assert np.array_equal(grade_host(every, inv), 255 - every)
    swap = np.ascontiguousarray(lut_identity(2)[..., [2, 1, 0]])
    assert np.array_equal(grade_host(every, swap), every[:, [2, 1, 0]])
    for n in (2, 17, 26, 33):
        t = random_lut(n, n)
        assert np.array_equal(grade_host(np.zeros((1, 3), np.uint8), t)[0], t[0, 0, 0]), "c0 is entry 0"
        assert np.array_equal(grade_host(np.full((1, 3), 255, np.uint8), t)[0], t[n - 1, n - 1, n - 1])
        # [b][g][r]: red runs fastest
        assert np.array_equal(grade_host(np.array([[255, 0, 0]], np.uint8), t)[0], t[0, 0, n - 1])
        assert np.array_equal(grade_host(np.array([[0, 0, 255]], np.uint8), t)[0], t[n - 1, 0, 0])


def write_cube(path, lut, extra=()):
    n = lut.shape[0]
    with open(path, "w") as fh:
        fh.write("# a test table\nTITLE \"t\"\nLUT_3D_SIZE %d\nDOMAIN_MIN 0.0 0.0 0.0\nDOMAIN_MAX 1.0 1.0 1.0\n\n" % n)
        for line in extra:
            fh.write(line + "\n")
        for e in lut.reshape(-1, 3):          # [b][g][r] flattened: red fastest
            fh.write("%.6f %.6f %.6f\n" % tuple(e / 255.0))


def test_helpers(built, tmp_path):
    import tiny_renderer_amd as T
    for n in (2, 5, 17, 33):
        assert np.array_equal(T.lut_from_function(n, lambda v: v), T.lut_identity(n))
        e = T.lut_identity(n)
        assert e.shape == (n, n, n, 3) and e.dtype == np.uint8
        assert np.array_equal(e[0, 0, :, 0], np.floor(255.0 * np.arange(n) / (n - 1) + 0.5).astype(np.uint8))
        assert (e[3 % n, 1, 0] == (e[0, 0, 0, 0], e[0, 0, 1, 0], e[0, 0, 3 % n, 0])).all()
    g = T.lut_from_function(9, lambda v: v ** (1 / 2.2))
    assert g[0, 0, 4, 0] == int(np.floor((0.5 ** (1 / 2.2)) * 255 + 0.5)) and g[0, 0, 4, 1] == 0
    lut = random_lut(7, 5)
    path = str(tmp_path / "t.cube")
    write_cube(path, lut)
    assert np.array_equal(T.load_cube(path), lut)
    one_d = str(tmp_path / "one.cube")
    open(one_d, "w").write("LUT_1D_SIZE 4\n0 0 0\n0.3 0.3 0.3\n0.6 0.6 0.6\n1 1 1\n")
    with pytest.raises(ValueError):
        T.load_cube(one_d)
    big = str(tmp_path / "big.cube")
    open(big, "w").write("LUT_3D_SIZE 34\n")
    with pytest.raises(ValueError):
        T.load_cube(big)
    dom = str(tmp_path / "dom.cube")
    open(dom, "w").write("LUT_3D_SIZE 2\nDOMAIN_MAX 2.0 2.0 2.0\n" + "0 0 0\n" * 8)
    with pytest.raises(ValueError):
        T.load_cube(dom)
    short = str(tmp_path / "short.cube")
    open(short, "w").write("LUT_3D_SIZE 2\n" + "0 0 0\n" * 7)
    with pytest.raises(ValueError):
        T.load_cube(short)


# ------------------------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------------------------

AT = TC.DST_AT
PIPE = "phong"
PLACE = {(130, 17): np.array([[0.8, 0.8, 0.0, 0.8]], np.float32), (300, 50): np.array([[0.7, 0.7, 0.0, 0.7]], np.float32)}
CORNER_AT = np.array([[0.66, 0.0, 0.0, 0.22]], np.float32)   # the model inside the right tile column of 384 x 48


def expectation(fb, lut):
    """tr_grade_host of the snapshot, asserted not to be vacuous."""
    want = grade_host(fb, lut)
    assert not np.array_equal(want, fb), "the expectation is the input"
    return want


def state(s):
    return {"z": bits(s.read_z_f32()), "win": s.read_winner_u32() if getattr(s, "_tap", False) else None}


def same_state(a, b):
    for k in a:
        assert (a[k] is None and b[k] is None) or np.array_equal(a[k], b[k]), k + " changed"


def box(img, f):
    Hh, W, _ = img.shape
    return ((img.reshape(Hh // f, f, W // f, f, 3).astype(np.uint32).sum((1, 3)) + f * f // 2) // (f * f)).astype(np.uint8)


def device_buffer(n, fill=0xAB):
    import torch
    t = torch.full((n,), fill, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return t


@pytest.mark.gpu
@pytest.mark.parametrize("W,Hh", [(7, 5), (128, 16), (130, 17), (256, 48), (300, 50), (384, 48)])
def test_graded_frame_equals_the_host_rule(small_synthetic, W, Hh):
    """7 x 5: one partial tile, 21-byte rows; 128 x 16: one tile; 130 x 17: 390-byte rows, a two-pixel tile column and a
    one-row tile row; 256 x 48 and 384 x 48: whole words, several tiles; 300 x 50: ragged, whole words.  n = 2 the smallest
    table, 25 and 26 the two sides of the LDS / global split, 33 the largest.  Through the getter and in place."""
    s = scene(W, Hh, small_synthetic, PIPE, PLACE.get((W, Hh), AT), tap=True)
    drive(s)
    f, before = snap(s), state(s)
    if (W, Hh) in PLACE:
        drawn = (f["fb"].max(-1) > 0)[::-1]
        assert drawn[:, W // 128 * 128:].any() and drawn[Hh // 16 * 16:].any(), "nothing drawn in the partial tiles"
    for n in (2, 17, 25, 26, 33):
        lut = random_lut(n, 7 * n + W)
        want = expectation(f["fb"], lut)
        s.set_lut(lut)
        drive(s)                                          # a fresh frame: flags as a render leaves them
        got = s.get_graded()
        assert np.array_equal(got, want), "getter, n %d: %d bytes differ" % (n, int((got != want).sum()))
        assert np.array_equal(s.get_frame_buffer(), f["fb"]), "the getter graded the frame"
        drive(s)
        s.grade()
        assert s.sync() == 0
        got = s.get_frame_buffer()
        assert np.array_equal(got, want), "in place, n %d: %d bytes differ" % (n, int((got != want).sum()))
        same_state(state(s), before)
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("W,Hh", [(130, 17), (384, 48)])
def test_random_colours_in_a_callers_buffer(small_synthetic, W, Hh):
    """A caller's buffer of random bytes, rendered into without a clear: colours from all over the cube go through the
    kernel, between guard bytes that must survive."""
    import torch
    guard, nb = 64, W * Hh * 3
    rng = np.random.default_rng(W)
    noise = rng.integers(0, 256, nb, dtype=np.uint8)
    for n in (17, 33):
        lut = random_lut(n, n + Hh)
        raw = np.concatenate([np.full(guard, 0xAA, np.uint8), noise, np.full(guard, 0xAA, np.uint8)])
        buf = torch.from_numpy(raw).cuda()
        torch.cuda.synchronize()
        s = scene(W, Hh, small_synthetic, PIPE, PLACE.get((W, Hh), AT))
        s.set_lut(lut)
        s.set_frame_buffer_device(buf.data_ptr() + guard)
        drive(s, clear=False)
        fb = s.get_frame_buffer()
        assert len(np.unique(fb.reshape(-1, 3), axis=0)) > nb // 6, "the frame is not noise"
        assert not np.array_equal(fb.reshape(-1), noise), "nothing was drawn over the noise"
        want = expectation(fb, lut)
        s.grade()
        assert s.sync() == 0
        got = buf.cpu().numpy()
        assert np.array_equal(got[guard:guard + nb].reshape(Hh, W, 3), want), "n %d: %d bytes differ" % (
            n, int((got[guard:guard + nb] != want.reshape(-1)).sum()))
        assert (got[:guard] == 0xAA).all() and (got[guard + nb:] == 0xAA).all(), "a guard byte changed"
        assert np.array_equal(s.get_frame_buffer(), want)
        s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("c0", [(0, 0, 0), (9, 0, 200)])
def test_fast_clear_flags(small_synthetic, c0):
    W, Hh = 384, 48
    s = scene(W, Hh, small_synthetic, PIPE, CORNER_AT, tap=True)
    drive(s)
    f, flags, before = snap(s), clean_flags(s), state(s)
    assert flags.sum() >= 1 and (~flags).sum() >= 1, "the frame needs flagged tiles and drawn ones"
    assert not (flags & tiles_any((f["fb"] != 0).any(-1)[::-1])).any()
    for n in (17, 33):
        lut = lut_c0(n, c0, n)
        want = expectation(f["fb"], lut)
        s.set_lut(lut)
        # out of place: every byte is stored over the fill, the frame and its flags stay
        drive(s)
        dev = device_buffer(W * Hh * 3)
        s.grade(out=dev.data_ptr())
        assert s.sync() == 0
        got = dev.cpu().numpy().reshape(Hh, W, 3)
        assert np.array_equal(got, want), "out of place: %d bytes differ" % int((got != want).sum())
        assert np.array_equal(clean_flags(s), flags), "an out-of-place call changed the frame's flags"
        assert np.array_equal(s.get_frame_buffer(), f["fb"])
        pinned = s.pinned_frame()
        pinned[:] = 0xAB
        s.grade(out=pinned)
        assert s.sync() == 0 and np.array_equal(pinned, want)
        for j, i in zip(*np.nonzero(flags)):
            assert (got[::-1][j * 16:j * 16 + 16, i * 128:i * 128 + 128] == np.array(c0, np.uint8)).all(), "a flagged tile is c0"
        # in place
        drive(s)
        assert np.array_equal(clean_flags(s), flags)
        s.grade()
        assert s.sync() == 0
        after = clean_flags(s)
        if c0 == (0, 0, 0):
            assert np.array_equal(after, flags), "flagged tiles keep their flags where c0 is black"
        else:
            assert not after.any(), "a tile that holds c0 != 0 is still flagged clean"
        got = s.get_frame_buffer()
        assert np.array_equal(got, want), "in place: %d bytes differ" % int((got != want).sum())
        assert np.array_equal(s.resolve(2), box(want, 2)), "resolve reads the flags"
        same_state(state(s), before)
    s.close()


@pytest.mark.gpu
def test_band_scene_touches_its_rows_only(small_synthetic):
    W, Hh, band = 256, 64, (16, 48)
    whole = scene(W, Hh, small_synthetic, PIPE, AT)
    drive(whole)
    ref = whole.get_frame_buffer()
    whole.close()
    assert ref[band[0]:band[1]].any()
    for c0 in ((0, 0, 0), (9, 0, 200)):
        lut = lut_c0(17, c0, 3)
        want = expectation(ref[band[0]:band[1]], lut)
        s = scene(W, Hh, small_synthetic, PIPE, AT, band_rows=band)
        s.set_lut(lut)
        drive(s)
        fb = s.get_frame_buffer()
        assert np.array_equal(fb[band[0]:band[1]], ref[band[0]:band[1]])
        out = device_buffer(W * Hh * 3)
        s.grade(out=out.data_ptr())
        assert s.sync() == 0
        got = out.cpu().numpy().reshape(Hh, W, 3)
        assert np.array_equal(got[band[0]:band[1]], want), "%d bytes differ" % int((got[band[0]:band[1]] != want).sum())
        assert (got[:band[0]] == 0xAB).all() and (got[band[1]:] == 0xAB).all(), "a row outside the band was written"
        own = s.get_graded()
        assert np.array_equal(own[band[0]:band[1]], want) and not own[:band[0]].any() and not own[band[1]:].any()
        s.grade()
        assert s.sync() == 0
        got = s.get_frame_buffer()
        assert np.array_equal(got[band[0]:band[1]], want)
        assert np.array_equal(got[:band[0]], fb[:band[0]]) and np.array_equal(got[band[1]:], fb[band[1]:]), "rows outside the band changed"
        s.close()


@pytest.mark.gpu
def test_a_logically_cleared_scene(small_synthetic):
    W, Hh = 256, 48
    ref = scene(W, Hh, small_synthetic, PIPE, AT)
    drive(ref)
    f = snap(ref)
    ref.close()
    drawn = (bits(f["z"]) != F32_MIN_BITS)[::-1]
    assert drawn.any() and not drawn.all()
    black = np.zeros((Hh, W, 3), np.uint8)
    # c0 = 0: nothing happens in place, zeros out of place
    s = scene(W, Hh, small_synthetic, PIPE, AT)
    s.set_lut(lut_c0(17, (0, 0, 0), 1))
    drive(s)
    s.clear()
    s.grade()
    assert s.sync() == 0 and not s.get_frame_buffer().any() and (bits(s.read_z_f32()) == F32_MIN_BITS).all()
    s.clear()
    dev = device_buffer(W * Hh * 3)
    s.grade(out=dev.data_ptr())
    assert s.sync() == 0 and not dev.cpu().numpy().any()
    assert not s.get_graded().any()
    drive(s)
    assert np.array_equal(s.get_frame_buffer(), f["fb"]), "the scene renders as before"
    # c0 != 0: the frame is the constant, and a render without a clear draws over it as over a backdrop
    lut = lut_c0(33, (9, 0, 200), 2)
    want = grade_host(black, lut)
    assert (want == np.array([9, 0, 200], np.uint8)).all()
    s.set_lut(lut)
    s.clear()
    assert np.array_equal(s.get_graded(), want)
    s.clear()
    dev = device_buffer(W * Hh * 3)
    s.grade(out=dev.data_ptr())
    assert s.sync() == 0 and np.array_equal(dev.cpu().numpy().reshape(Hh, W, 3), want)
    s.clear()
    s.grade()
    assert s.sync() == 0
    assert np.array_equal(s.get_frame_buffer(), want) and (bits(s.read_z_f32()) == F32_MIN_BITS).all()
    assert not clean_flags(s).any()
    drive(s, clear=False)
    got = s.get_frame_buffer()
    assert np.array_equal(got, np.where(drawn[..., None], f["fb"], want)), "the render's own pixels where z is drawn, c0 elsewhere"
    assert np.array_equal(bits(s.read_z_f32()), bits(f["z"]))
    s.close()


@pytest.mark.gpu
def test_in_place_consumers_see_the_graded_frame(small_synthetic, other_synthetic):
    W, Hh = 384, 48
    mk = lambda ms=None, at=None, **kw: scene(W, Hh, ms or small_synthetic, PIPE, TC._small(-0.4, 0.1) if at is None else at, **kw)
    ref = mk(tap=True)
    drive(ref)
    f = snap(ref)
    ref.close()
    lut = lut_c0(17, (0, 0, 0), 11)
    once = expectation(f["fb"], lut)
    twice = grade_host(once, lut)
    assert not np.array_equal(twice, once)
    graded = dict(f, fb=once, win=None)
    s = mk(tap=True)
    s.set_lut(lut)
    drive(s), s.grade()
    assert np.array_equal(s.resolve(2), box(once, 2))
    # the sparse read-back into a page-locked buffer
    out = s.pinned_frame()
    out[:] = 0x5A
    drive(s), s.grade()
    s.get_frame_buffer_async(out)
    assert s.sync() == 0 and np.array_equal(out, once)
    assert np.array_equal(s.get_frame_buffer(), once)
    assert np.array_equal(bits(s.read_z_f32()), bits(f["z"])) and np.array_equal(s.read_winner_u32(), f["win"])
    # twice
    s.grade()
    assert np.array_equal(s.get_frame_buffer(), twice), "grading twice is the rule applied twice"
    assert np.array_equal(bits(s.read_z_f32()), bits(f["z"])) and np.array_equal(s.read_winner_u32(), f["win"])
    s.close()
    # composite: the graded scene as dst and as src
    o = mk(other_synthetic, TC._small(-0.2, 0.0, 0.2))
    drive(o, light=0.2)
    fo = snap(o)
    fo["win"] = None
    o.close()
    for role in ("dst", "src"):
        a, b = mk(), mk(other_synthetic, TC._small(-0.2, 0.0, 0.2))
        a.set_lut(lut)
        drive(a), drive(b, light=0.2)
        a.grade()
        if role == "dst":
            a.composite(b)
            want, wins = TC.merge(graded, fo)
            got = a
        else:
            b.composite(a)
            want, wins = TC.merge(fo, graded)
            got = b
        assert wins.any() and not wins.all()
        TC.same(snap(got), want)
        a.close(), b.close()
    # render to texture: the graded frame as another scene's image, with a table that colours the cleared tiles too
    mesh, texs = small_synthetic
    th, tw = texs[0].shape[:2]
    src = scene(tw, th, small_synthetic, PIPE, AT)
    drive(src)
    tf = src.get_frame_buffer()
    tl = lut_c0(26, (9, 0, 200), 12)
    tex_want = expectation(tf, tl)
    src.set_lut(tl)
    drive(src), src.grade()
    dst = scene(64, 64, small_synthetic, PIPE)
    dst.set_texture_from(src, 0)
    assert np.array_equal(dst.read_texture(0), tex_want)
    src.close(), dst.close()


@pytest.mark.gpu
def test_transient_depth_stays_transient(small_synthetic):
    """The observable of test_bloom.py: the profile's k_tile launches -- one for the frame, none for the grade calls, and
    the depth-only repeat only when z is read afterwards."""
    W, Hh = 256, 48
    ref = scene(W, Hh, small_synthetic, PIPE, AT, auto_group=False)
    drive(ref)
    f = snap(ref)
    ref.close()
    lut = random_lut(17, 21)
    want = expectation(f["fb"], lut)
    s = scene(W, Hh, small_synthetic, PIPE, AT, auto_group=False)
    s.set_lut(lut)
    s.profile_enable(True)
    drive(s)
    assert np.array_equal(s.get_graded(), want)
    s.grade()
    assert s.sync() == 0
    prof = s.profile_read()
    assert prof["k_tile"]["launches"] == 1, "grade repeated the pass for its depth: %r" % (prof,)
    assert prof.get("k_grade", {}).get("launches") == 2 and prof["k_grade"]["total_ms"] > 0.0, prof
    assert np.array_equal(bits(s.read_z_f32()), bits(f["z"]))
    assert s.profile_read()["k_tile"]["launches"] == 2, "the depth was not transient: the case shows nothing"
    assert np.array_equal(s.get_frame_buffer(), want)
    s.close()


@pytest.mark.gpu
def test_refusals_queue_nothing_and_a_selected_frame(small_synthetic):
    import tiny_renderer_amd as T
    from tiny_renderer_amd import _lib
    L = T.load_library()
    W, Hh = 256, 48
    s = scene(W, Hh, small_synthetic, PIPE, AT, tap=True)
    drive(s)
    f, flags = snap(s), clean_flags(s)
    host_out = np.zeros((Hh, W, 3), np.uint8)
    # no table
    assert L.tr_scene_grade(s._h, None) == _lib.TR_E_INVALID and b"table" in L.tr_last_error()
    assert L.tr_scene_get_graded(s._h, host_out.ctypes.data) == _lib.TR_E_INVALID and b"table" in L.tr_last_error()
    lut = random_lut(17, 31)
    want = expectation(f["fb"], lut)
    for n in (1, 34):
        assert L.tr_scene_set_lut(s._h, n, lut.ctypes.data) == _lib.TR_E_INVALID and L.tr_last_error()
    assert L.tr_scene_set_lut(s._h, 17, None) == _lib.TR_E_INVALID and b"null" in L.tr_last_error()
    assert L.tr_scene_grade(s._h, None) == _lib.TR_E_INVALID, "a refused table was taken"
    s.set_lut(lut)
    assert L.tr_scene_get_graded(s._h, None) == _lib.TR_E_INVALID and b"null" in L.tr_last_error()
    fb_dev = int(s.frame_buffer_device())
    for off in (0, 3 * W, W * Hh * 3 - 1):
        assert L.tr_scene_grade(s._h, fb_dev + off) == _lib.TR_E_INVALID and b"overlaps" in L.tr_last_error()
    small = L.tr_host_alloc(W * Hh * 3 - 1)
    assert small
    assert L.tr_scene_grade(s._h, small) == _lib.TR_E_INVALID and b"smaller" in L.tr_last_error()
    L.tr_host_free(small)
    assert L.tr_scene_grade(s._h, host_out.ctypes.data) == _lib.TR_E_INVALID and b"tr_host_alloc" in L.tr_last_error()
    with pytest.raises(T.TinyRendererError):
        s.grade(out=host_out)
    assert not host_out.any()
    assert s.sync() == 0 and np.array_equal(clean_flags(s), flags)
    TC.same(snap(s), f)
    # the table works, is replaced, and is dropped again
    assert np.array_equal(s.get_graded(), want)
    other = random_lut(26, 32)
    s.set_lut(other)
    assert np.array_equal(s.get_graded(), grade_host(f["fb"], other))
    assert L.tr_scene_set_lut(s._h, 0, None) == 0
    assert L.tr_scene_grade(s._h, None) == _lib.TR_E_INVALID and b"table" in L.tr_last_error()
    s.set_lut(lut), s.set_lut(None)
    with pytest.raises(T.TinyRendererError):
        s.get_graded()
    TC.same(snap(s), f)
    s.close()
    # a kept frame chosen with select_frame: it alone is graded
    par = TC._params(4)
    kept = []
    for twin in (True, False):
        g = scene(W, Hh, small_synthetic, PIPE, AT, frames_per_launch=4)
        g.set_lut(lut)
        g.render_frames(par)
        assert g.frames_kept() >= 3
        if twin:
            for back in range(3):
                g.select_frame(back)
                kept.append(snap(g))
            want1 = expectation(kept[1]["fb"], lut)
            assert not np.array_equal(want1, grade_host(kept[0]["fb"], lut))
        else:
            g.select_frame(1)
            g.grade()
            assert np.array_equal(g.get_frame_buffer(), want1)
            for back in (0, 2):
                g.select_frame(back)
                TC.same(snap(g), kept[back])
            g.select_frame(1)
            assert np.array_equal(g.get_frame_buffer(), want1) and np.array_equal(bits(g.read_z_f32()), bits(kept[1]["z"]))
        g.close()


@pytest.mark.gpu
def test_chain_ao_dof_bloom_grade_resolve(small_synthetic):
    """Ambient occlusion, depth of field, bloom, grade, resolve by 2, on 256 x 48: the host rules in that order."""
    import tiny_renderer_amd as T
    from tests import test_depth_of_field as TD
    W, Hh = 256, 48
    ref = scene(W, Hh, small_synthetic, PIPE, AT)
    drive(ref)
    f = snap(ref)
    ref.close()
    ao = dict(radius=8, rings=2)
    shaded = T.ambient_occlusion_host(f["z"], f["fb"], **ao)
    assert not np.array_equal(shaded, f["fb"])
    dp = TD.params_for(f, 3)
    soft = T.depth_of_field_host(f["z"], shaded, dp)
    assert not np.array_equal(soft, shaded)
    m = soft.max(-1)
    bp = T.bloom_params(8, threshold=int(np.quantile(m[m > 0], 0.6)), strength=512)
    lit = T.bloom_host(soft, bp)
    assert not np.array_equal(lit, soft)
    lut = T.lut_from_function(33, lambda v: v ** (1 / 2.2))
    want = expectation(lit, lut)
    s = scene(W, Hh, small_synthetic, PIPE, AT)
    s.set_lut(lut)
    drive(s)
    s.ambient_occlusion(**ao)
    s.depth_of_field(dp)
    s.bloom(bp)
    s.grade()
    assert np.array_equal(s.resolve(2), box(want, 2))
    assert np.array_equal(s.get_frame_buffer(), want)
    assert np.array_equal(bits(s.read_z_f32()), bits(f["z"]))
    s.close()


@pytest.mark.gpu
def test_cli_gamma_and_lut_write_the_host_rule_of_the_plain_run(african_head, tmp_path):
    import tiny_renderer_amd as T
    from tiny_renderer_amd import cli
    common = ["-p", H.asset_dir("african_head"), "-s", "phong", "--width", "256", "--height", "128", "--camera-angle", "0.3",
              "--light-angle", "0.7"]
    plain, gam, cub = (str(tmp_path / n) for n in ("plain.ppm", "gamma.ppm", "cube.ppm"))
    assert cli.main(common + ["--out", plain]) == 0
    hd = b"P6\n256 128\n255\n"
    read = lambda p: np.frombuffer(open(p, "rb").read()[len(hd):], np.uint8).reshape(128, 256, 3)
    a = read(plain)
    assert cli.main(common + ["--gamma", "2.2", "--out", gam]) == 0
    assert np.array_equal(read(gam), expectation(a, T.lut_from_function(33, lambda v: v ** (1 / 2.2))))
    lut = random_lut(9, 77)
    path = str(tmp_path / "grade.cube")
    write_cube(path, lut)
    assert cli.main(common + ["--lut", path, "--out", cub]) == 0
    assert np.array_equal(read(cub), expectation(a, lut))


@pytest.fixture(scope="module")
def other_synthetic(built):
    import tiny_renderer_amd as T
    return T.synthetic_scene(n_lat=9, n_lon=17, tex_size=128, radius=0.75)
