"""Bloom: tr_scene_bloom / tr_scene_get_bloom (k_bloom) and tr_bloom_host against the rule in numpy.

The rule, from the words of include/tiny_renderer.h, over the stored u8 values F of a frame (a pixel outside it is
black): key B_p = F_p where max(F_p) > threshold, else 0; tent w(d) = R + 1 - |d|; V_p[c] = the sum over |dx|, |dy| <= R of
w(dx) * w(dy) * B_(x + dx, y + dy)[c]; D = (R + 1)^4; glow G = (V + D // 2) // D; out = min(255, F + ((strength * G + 128)
>> 8)), or G alone under TR_BLOOM_GLOW_ONLY.  The contract is exact: every comparison is np.array_equal.

On the CPU tr_bloom_host is pinned against that restatement, written as the 2-D sum (the library makes two separable
passes).  On the GPU the expectation is tr_bloom_host applied to a snapshot of the very frame that is then rendered again
(so that its flags are fresh) and bloomed; every case first asserts ON THE EXPECTATION that it is not vacuous."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

from tests import helpers as H
from tests import test_composite as TC

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32_MIN_BITS = np.uint32(0xFF7FFFFF)
bits, drive, scene, snap, clean_flags, tiles_any = TC.bits, TC.drive, TC.scene, TC.snap, TC.clean_flags, TC.tiles_any
GLOW = 1


def P(R, thr=200, strength=256, flags=0):
    from tiny_renderer_amd.scene import bloom_params
    return bloom_params(R, threshold=thr, strength=strength, flags=flags)


# ------------------------------------------------------------------------------------------------------------------
# The rule in numpy
# ------------------------------------------------------------------------------------------------------------------

def blur_sums(rgb, R, thr):
    """V [H, W, 3] int64: the 2-D sum of the rule."""
    F = np.asarray(rgb).astype(np.int64)
    Hh, W, _ = F.shape
    B = np.where((F.max(-1) > thr)[..., None], F, 0)
    pb = np.zeros((Hh + 2 * R, W + 2 * R, 3), np.int64)   # outside the frame: black
    pb[R:R + Hh, R:R + W] = B
    V = np.zeros((Hh, W, 3), np.int64)
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            V += (R + 1 - abs(dx)) * (R + 1 - abs(dy)) * pb[R + dy:R + dy + Hh, R + dx:R + dx + W]
    return V


def finish(rgb, V, R, strength, flags):
    D = (R + 1) ** 4
    assert V.max() + D // 2 < 2 ** 32
    G = (V + D // 2) // D
    if flags & GLOW:
        return G.astype(np.uint8)
    return np.minimum(255, np.asarray(rgb).astype(np.int64) + ((strength * G + 128) >> 8)).astype(np.uint8)


def rule(rgb, R, thr=200, strength=256, flags=0):
    return finish(rgb, blur_sums(rgb, R, thr), R, strength, flags)


# ------------------------------------------------------------------------------------------------------------------
# CPU
# ------------------------------------------------------------------------------------------------------------------

BAD = [("struct_size", 16), ("struct_size", 24), ("struct_size", 0), ("radius", 0), ("radius", 16), ("radius", 0xFFFFFFFF),
       ("threshold", 256), ("threshold", 0x80000000), ("strength", 1025), ("strength", 0xFFFFFFFF), ("flags", 2), ("flags", 0x80000001)]


def test_entry_points_declared_exported_and_typed(built):
    import tiny_renderer_amd as T
    from tiny_renderer_amd import _lib
    from tiny_renderer_amd.scene import BloomParams, bloom_params
    header = open(os.path.join(REPO, "include", "tiny_renderer.h")).read()
    assert re.search(r"int\s+tr_scene_bloom\(tr_scene \*s, const tr_bloom_params \*p, void \*out", header)
    assert re.search(r"int\s+tr_scene_get_bloom\(tr_scene \*s, const tr_bloom_params \*p, uint8_t \*rgb\);", header)
    assert re.search(r"int\s+tr_bloom_host\(uint32_t width, uint32_t height, const uint8_t \*rgb", header)
    for word in ("#define TR_BLOOM_MAX_RADIUS 15", "#define TR_BLOOM_GLOW_ONLY 0x1u", "} tr_bloom_params;", "#define TR_ABI_VERSION 3"):
        assert word in header, word
    exports = open(os.path.join(REPO, "tiny_renderer_amd", "csrc", "exports.map")).read()
    assert re.search(r"global:\s*tr_\*;", exports)
    raw = C.CDLL(_lib.library_path())
    for name in ("tr_scene_bloom", "tr_scene_get_bloom", "tr_bloom_host"):
        assert hasattr(raw, name), name + " is not exported"
        assert name in _lib.SYMBOLS
    assert _lib.SYMBOLS["tr_scene_bloom"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p])
    assert _lib.SYMBOLS["tr_scene_get_bloom"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p])
    assert _lib.SYMBOLS["tr_bloom_host"] == (C.c_int, [C.c_uint32, C.c_uint32] + [C.c_void_p] * 3)
    assert C.sizeof(BloomParams) == 20
    L = T.load_library()
    assert L.tr_abi_version() == 3
    p = bloom_params(4)
    assert (p.struct_size, p.radius, p.threshold, p.strength, p.flags) == (20, 4, 200, 256, 0)
    with pytest.raises(TypeError):
        bloom_params()                                     # the radius is required
    for name in ("bloom_host", "bloom_params", "BloomParams"):
        assert hasattr(T, name) and name in T.__all__, name
    assert callable(T.Scene.bloom) and callable(T.Scene.get_bloom)


def test_null_arguments_are_refused_with_a_text(built):
    import tiny_renderer_amd as T
    from tiny_renderer_amd import _lib
    L = T.load_library()
    p = P(3)
    out = np.zeros((2, 2, 3), np.uint8)
    assert L.tr_scene_bloom(None, C.addressof(p), None) == _lib.TR_E_INVALID and b"null" in L.tr_last_error()
    assert L.tr_scene_get_bloom(None, C.addressof(p), out.ctypes.data) == _lib.TR_E_INVALID and b"null" in L.tr_last_error()
    assert L.tr_bloom_host(2, 2, out.ctypes.data, out.ctypes.data, None) == _lib.TR_E_INVALID and b"null" in L.tr_last_error()


def test_host_refuses_every_invalid_parameter(built):
    import tiny_renderer_amd as T
    from tiny_renderer_amd import _lib
    from tiny_renderer_amd.scene import bloom_params
    L = T.load_library()
    rgb, out = np.zeros((2, 2, 3), np.uint8), np.zeros((2, 2, 3), np.uint8)
    host = lambda q: L.tr_bloom_host(2, 2, rgb.ctypes.data, out.ctypes.data, C.addressof(q))
    assert host(P(3)) == 0
    for field, v in BAD:
        q = P(3)
        setattr(q, field, v)
        assert host(q) == _lib.TR_E_INVALID and L.tr_last_error(), (field, v)
    for field, v in (("radius", 1), ("radius", 15), ("threshold", 0), ("threshold", 255), ("strength", 0), ("strength", 1024), ("flags", 1)):
        q = P(3)
        setattr(q, field, v)
        assert host(q) == 0, (field, v)
    q = P(3)
    assert L.tr_bloom_host(2, 2, None, out.ctypes.data, C.addressof(q)) == _lib.TR_E_INVALID
    assert L.tr_bloom_host(2, 2, rgb.ctypes.data, None, C.addressof(q)) == _lib.TR_E_INVALID
    assert L.tr_bloom_host(2, 2, rgb.ctypes.data, rgb.ctypes.data, C.addressof(q)) == _lib.TR_E_INVALID   # out == rgb
    assert L.tr_bloom_host(0, 5, None, None, C.addressof(q)) == 0 and L.tr_bloom_host(5, 0, None, None, C.addressof(q)) == 0
    # python: ValueError before anything reaches the library
    for kw in (dict(radius=0), dict(radius=16), dict(radius=2.5), dict(radius=True), dict(threshold=256), dict(threshold=-1),
               dict(threshold=1.5), dict(strength=1025), dict(strength=-1), dict(flags=2)):
        with pytest.raises(ValueError):
            bloom_params(**dict(dict(radius=3), **kw))
    s = T.Scene.__new__(T.Scene)
    s.width, s.height, s._h, s._pinned = 64, 64, None, []
    with pytest.raises(ValueError):
        s.bloom(None)
    with pytest.raises(ValueError):
        s.get_bloom((3, 200))
    with pytest.raises(ValueError):
        T.bloom_host(rgb[..., :2], q)


def speckled(W, Hh, seed):
    """Mostly dark, with bright speckles and whole pixels of 255 and of 0."""
    rng = np.random.default_rng(seed)
    rgb = rng.integers(0, 130, (Hh, W, 3), dtype=np.uint8)
    bright = rng.random((Hh, W)) < 0.15
    rgb[bright] = rng.integers(129, 256, (int(bright.sum()), 3), dtype=np.uint8)
    rgb[rng.random((Hh, W)) < 0.03] = 255
    rgb[rng.random((Hh, W)) < 0.03] = 0
    return rgb


@pytest.mark.parametrize("W,Hh", [(1, 1), (7, 5), (31, 33), (130, 17)])
def test_host_rule_equals_the_numpy_rule(built, W, Hh):
    import tiny_renderer_amd as T
    rgb = speckled(W, Hh, W * 100 + Hh)
    if W == 1:
        rgb[:] = (3, 250, 128)
    keep = rgb.copy()
    changed = 0
    for R, thr in itertools.product((1, 2, 8, 15), (0, 128, 254, 255)):
        V = blur_sums(rgb, R, thr)
        for strength, flags in itertools.product((0, 256, 1024), (0, GLOW)):
            want = finish(rgb, V, R, strength, flags)
            got = T.bloom_host(rgb, P(R, thr, strength, flags))
            assert got.dtype == np.uint8 and got.shape == rgb.shape
            assert np.array_equal(got, want), "R %d thr %d strength %d flags %d: %d bytes differ" % (R, thr, strength, flags, int((got != want).sum()))
            changed += int((got != rgb).sum())
    assert changed > 100
    assert np.array_equal(rgb, keep), "the argument is left alone"


def test_threshold_255_returns_the_input(built):
    import tiny_renderer_amd as T
    rgb = speckled(40, 23, 1)
    assert (rgb == 255).any()
    for R in (1, 7, 15):
        for strength in (0, 256, 1024):
            assert np.array_equal(T.bloom_host(rgb, P(R, 255, strength)), rgb)
        assert not T.bloom_host(rgb, P(R, 255, flags=GLOW)).any()
    # strength 0: the input at any threshold
    assert np.array_equal(T.bloom_host(rgb, P(8, 0, 0)), rgb)


def test_glow_only_of_a_constant_image_is_the_clipped_tent(built):
    """Threshold 0 keys every pixel of value v > 0 in: along one axis a pixel at distance e from the border sums the
    weights of the taps inside the frame, so the glow is (v * sx * sy + D / 2) / D with sx, sy those clipped sums, and v
    itself where neither axis is clipped."""
    import tiny_renderer_amd as T
    W, Hh = 45, 37
    for R in (1, 2, 8, 15):
        S, D = (R + 1) ** 2, (R + 1) ** 4
        axis = lambda n: np.array([sum(R + 1 - abs(d) for d in range(-R, R + 1) if 0 <= i + d < n) for i in range(n)], np.int64)
        sx, sy = axis(W), axis(Hh)
        assert sx[R] == S and sx[0] == (R + 1) * (R + 2) // 2 and sx[W - 1] == sx[0]
        for v in (1, 77, 255):
            rgb = np.full((Hh, W, 3), v, np.uint8)
            rgb[..., 1] = max(v // 2, 1)
            got = T.bloom_host(rgb, P(R, 0, flags=GLOW))
            for c, val in enumerate((v, max(v // 2, 1), v)):
                want = (val * sy[:, None] * sx[None, :] + D // 2) // D
                assert np.array_equal(got[..., c].astype(np.int64), want), (R, v, c)
            assert np.array_equal(got[R:Hh - R, R:W - R], rgb[R:Hh - R, R:W - R]), "inside: the value itself"
            assert (got[0, 0] < rgb[0, 0]).all() or v == 1


def test_a_single_bright_pixel_spreads_as_the_tent(built):
    import tiny_renderer_amd as T
    W, Hh = 41, 35
    for R in (1, 2, 8, 15):
        D = (R + 1) ** 4
        for (py, px) in ((17, 20), (0, 0), (Hh - 1, W - 2), (3, W - 1)):
            one = np.zeros((Hh, W, 3), np.uint8)
            one[py, px] = 255
            got = T.bloom_host(one, P(R, 100, flags=GLOW))
            ys, xs = np.mgrid[0:Hh, 0:W]
            w = np.maximum(R + 1 - np.abs(xs - px), 0) * np.maximum(R + 1 - np.abs(ys - py), 0)
            want = (255 * w + D // 2) // D
            for c in range(3):
                assert np.array_equal(got[..., c].astype(np.int64), want), (R, py, px)
            assert np.array_equal(got, rule(one, R, 100, flags=GLOW))
            assert got[py, px, 0] == (255 * (R + 1) ** 2 + D // 2) // D


def test_saturation(built):
    import tiny_renderer_amd as T
    white = np.full((19, 33, 3), 255, np.uint8)
    for R in (1, 8, 15):
        assert np.array_equal(T.bloom_host(white, P(R, 0, 1024)), white)
        assert np.array_equal(T.bloom_host(white, P(R, 254, 1024)), white)


# ------------------------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------------------------

AT = TC.DST_AT
PIPE = "phong"


def host(fb, p):
    import tiny_renderer_amd as T
    return T.bloom_host(fb, p)


def mid_threshold(fb):
    """A threshold below the frame's maximum that some drawn pixels pass and others do not."""
    m = fb.max(-1)
    lit = m[m > 0]
    assert lit.size >= 4
    thr = int(np.quantile(lit, 0.6))
    assert (m > thr).any() and ((m > 0) & (m <= thr)).any(), "the key splits nothing"
    return thr


def expectation(fb, p):
    """tr_bloom_host of the snapshot, asserted not to be vacuous: a pixel passes the key and a byte changes."""
    want = host(fb, p)
    assert (fb.max(-1) > p.threshold).any(), "no pixel passes the key"
    assert not np.array_equal(want, fb), "the expectation is the input"
    return want


def state(s):
    """Everything a call must leave alone: z, winner words."""
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


# the settings beside the radius, one further frame each: (W, H) -> (R, threshold or None for a mid value, strength, flags)
SETTINGS = {(7, 5): [(8, 0, 256, 0), (15, None, 1024, GLOW)],
            (128, 16): [(2, None, 1024, 0), (15, 0, 256, GLOW)],
            (256, 48): [(8, None, 0, GLOW), (1, 255, 256, 0)],
            (300, 50): [(15, None, 256, 0), (2, 0, 1024, GLOW)]}
# where the model stands: over the partial tile column and row of the ragged frames
PLACE = {(130, 17): np.array([[0.8, 0.8, 0.0, 0.8]], np.float32), (300, 50): np.array([[0.7, 0.7, 0.0, 0.7]], np.float32)}


def cases_for(W, Hh):
    if (W, Hh) in ((130, 17), (384, 48)):
        return [(1, None, 256, 0), (2, 0, 256, GLOW), (8, None, 1024, 0), (15, None, 256, 0), (15, 0, 256, GLOW), (8, 255, 256, 0), (2, None, 0, 0),
                (8, 255, 256, GLOW)]
    return SETTINGS[(W, Hh)]


@pytest.mark.gpu
@pytest.mark.parametrize("W,Hh", [(7, 5), (128, 16), (130, 17), (256, 48), (384, 48), (300, 50)])
def test_bloomed_frame_equals_the_host_rule(small_synthetic, W, Hh):
    """7 x 5: smaller than the radius, one partial tile, guarded; 128 x 16: one tile, every halo piece outside the grid;
    130 x 17: ragged in both axes, a two-pixel tile column and a one-row tile row; 256 x 48: tiles above and below;
    384 x 48: a tile with all eight neighbours; 300 x 50: guarded, ragged.  In place and through the getter."""
    s = scene(W, Hh, small_synthetic, PIPE, PLACE.get((W, Hh), AT), tap=True)
    drive(s)
    f, before = snap(s), state(s)
    if (W, Hh) in PLACE:
        drawn = (f["fb"].max(-1) > 0)[::-1]
        assert drawn[:, W // 128 * 128:].any() and drawn[Hh // 16 * 16:].any(), "nothing drawn in the partial tiles"
    for R, thr, strength, flags in cases_for(W, Hh):
        p = P(R, mid_threshold(f["fb"]) if thr is None else thr, strength, flags)
        if thr == 255 and flags:
            want = host(f["fb"], p)                       # (nothing keyed, the glow alone: zeros over the drawn tiles too)
            assert not want.any() and f["fb"].any()
        elif thr == 255 or (strength == 0 and not flags):
            want = host(f["fb"], p)                       # (the identity: the settings' own edge)
            assert np.array_equal(want, f["fb"])
        else:
            want = expectation(f["fb"], p)
        drive(s)                                          # a fresh frame: flags as a render leaves them
        got = s.get_bloom(p)
        assert np.array_equal(got, want), "getter, %r: %d bytes differ" % ((R, thr, strength, flags), int((got != want).sum()))
        assert np.array_equal(s.get_frame_buffer(), f["fb"]), "the getter bloomed the frame"
        drive(s)
        s.bloom(p)
        assert s.sync() == 0
        got = s.get_frame_buffer()
        assert np.array_equal(got, want), "in place, %r: %d bytes differ" % ((R, thr, strength, flags), int((got != want).sum()))
        same_state(state(s), before)
    s.close()


CORNER_AT = np.array([[0.66, 0.0, 0.0, 0.22]], np.float32)   # the model inside the right tile column of 384 x 48


def tile_kinds(fb, flags, want):
    """From the snapshot: tiles whose 3 x 3 neighbourhood is all clean, clean tiles beside a drawn one that receive glow,
    drawn tiles."""
    ty, tx = flags.shape
    lone = np.zeros_like(flags)
    for j, i in np.ndindex(ty, tx):
        lone[j, i] = flags[max(j - 1, 0):j + 2, max(i - 1, 0):i + 2].all()
    lit = tiles_any((want != 0).any(-1)[::-1])
    return lone, flags & ~lone & lit, ~flags


@pytest.mark.gpu
def test_the_three_kinds_of_tile(small_synthetic):
    W, Hh = 384, 48
    s = scene(W, Hh, small_synthetic, PIPE, CORNER_AT)
    drive(s)
    f, flags = snap(s), clean_flags(s)
    assert not (flags & tiles_any((f["fb"] != 0).any(-1)[::-1])).any()
    p = P(15, mid_threshold(f["fb"]), 1024)
    want = expectation(f["fb"], p)
    lone, spill, drawn = tile_kinds(f["fb"], flags, want)
    assert lone.sum() >= 1 and spill.sum() >= 1 and drawn.sum() >= 1, (int(lone.sum()), int(spill.sum()), int(drawn.sum()))
    for place in ("in", "out"):
        drive(s)
        assert np.array_equal(clean_flags(s), flags)
        if place == "in":
            s.bloom(p)
            got = s.get_frame_buffer()
            after = clean_flags(s)
            assert np.array_equal(after, lone), "flags: up exactly where the whole neighbourhood was clean"
            assert not (after & spill).any(), "a cleared tile that received glow kept its flag"
        else:
            got = s.get_bloom(p)
        assert np.array_equal(got, want), "%s place: %d bytes differ" % (place, int((got != want).sum()))
        for j, i in zip(*np.nonzero(spill)):
            assert got[::-1][j * 16:j * 16 + 16, i * 128:i * 128 + 128].any(), "no glow in tile (%d, %d)" % (j, i)
        for j, i in zip(*np.nonzero(lone)):
            assert not got[::-1][j * 16:j * 16 + 16, i * 128:i * 128 + 128].any()
    s.close()


@pytest.mark.gpu
def test_in_place_consumers_see_the_bloomed_frame(small_synthetic, other_synthetic):
    import tiny_renderer_amd as T
    W, Hh = 384, 48
    mk = lambda ms=None, at=None, **kw: scene(W, Hh, ms or small_synthetic, PIPE, TC._small(-0.4, 0.1) if at is None else at, **kw)
    ref = mk(tap=True)
    drive(ref)
    f = snap(ref)
    ref.close()
    p = P(8, mid_threshold(f["fb"]), 512)
    once = expectation(f["fb"], p)
    twice = host(once, p)
    assert not np.array_equal(twice, once)
    bloomed = dict(f, fb=once, win=None)
    s = mk(tap=True)
    drive(s), s.bloom(p)
    assert np.array_equal(s.resolve(2), box(once, 2))
    # the sparse read-back into a page-locked buffer: the copied flags
    out = s.pinned_frame()
    out[:] = 0x5A
    drive(s), s.bloom(p)
    s.get_frame_buffer_async(out)
    assert s.sync() == 0 and np.array_equal(out, once)
    assert not (clean_flags(s) & tiles_any(once[::-1].any(-1))).any(), "a tile with colour in it is flagged clean"
    assert np.array_equal(s.get_frame_buffer(), once)
    assert np.array_equal(bits(s.read_z_f32()), bits(f["z"])) and np.array_equal(s.read_winner_u32(), f["win"])
    # twice
    s.bloom(p)
    assert np.array_equal(s.get_frame_buffer(), twice), "blooming twice is the rule applied twice"
    assert np.array_equal(bits(s.read_z_f32()), bits(f["z"])) and np.array_equal(s.read_winner_u32(), f["win"])
    s.close()
    # composite: the bloomed scene as dst and as src
    o = mk(other_synthetic, TC._small(-0.2, 0.0, 0.2))
    drive(o, light=0.2)
    fo = snap(o)
    fo["win"] = None
    o.close()
    for role in ("dst", "src"):
        a, b = mk(), mk(other_synthetic, TC._small(-0.2, 0.0, 0.2))
        drive(a), drive(b, light=0.2)
        a.bloom(p)
        if role == "dst":
            a.composite(b)
            want, wins = TC.merge(bloomed, fo)
            got = a
        else:
            b.composite(a)
            want, wins = TC.merge(fo, bloomed)
            got = b
        assert wins.any() and not wins.all()
        TC.same(snap(got), want)
        a.close(), b.close()
    # render to texture: the bloomed frame as another scene's image
    mesh, texs = small_synthetic
    th, tw = texs[0].shape[:2]
    src = scene(tw, th, small_synthetic, PIPE, AT)
    drive(src)
    tf = src.get_frame_buffer()
    pt = P(8, mid_threshold(tf), 512)
    tex_want = expectation(tf, pt)
    drive(src), src.bloom(pt)
    dst = scene(64, 64, small_synthetic, PIPE)
    dst.set_texture_from(src, 0)
    assert np.array_equal(dst.read_texture(0), tex_want)
    src.close(), dst.close()


@pytest.mark.gpu
def test_out_of_place_targets_are_filled_and_leave_the_scene_alone(small_synthetic):
    import tiny_renderer_amd as T
    W, Hh = 384, 48
    s = scene(W, Hh, small_synthetic, PIPE, CORNER_AT, tap=True)
    drive(s)
    f, before, flags = snap(s), state(s), clean_flags(s)
    p = P(8, mid_threshold(f["fb"]), 768)
    want = expectation(f["fb"], p)
    lone, _, _ = tile_kinds(f["fb"], flags, want)
    assert lone.any(), "no tile is produced as zeros on the flags alone"
    drive(s)
    dev = device_buffer(W * Hh * 3)                       # 0xAB everywhere: a byte that is not written shows
    s.bloom(p, out=dev.data_ptr())
    assert s.sync() == 0
    assert np.array_equal(dev.cpu().numpy().reshape(Hh, W, 3), want)
    pinned = s.pinned_frame()
    pinned[:] = 0xAB
    s.bloom(p, out=pinned)
    assert s.sync() == 0 and np.array_equal(pinned, want)
    assert np.array_equal(s.get_bloom(p), want)
    assert np.array_equal(clean_flags(s), flags), "an out-of-place call changed the frame's flags"
    TC.same(snap(s), f)
    same_state(state(s), before)
    s.close()


@pytest.mark.gpu
def test_a_cleared_scene_a_selected_frame_and_a_callers_buffer(small_synthetic):
    import torch
    W, Hh = 256, 48
    s = scene(W, Hh, small_synthetic, PIPE, AT)
    drive(s)
    f = snap(s)
    p = P(8, mid_threshold(f["fb"]), 512)
    # logically cleared: zeros out of place, nothing in place
    s.clear()
    dev = device_buffer(W * Hh * 3)
    s.bloom(p, out=dev.data_ptr())
    assert s.sync() == 0 and not dev.cpu().numpy().any()
    assert not s.get_bloom(p).any()
    s.bloom(p)
    assert not s.get_frame_buffer().any() and (bits(s.read_z_f32()) == F32_MIN_BITS).all()
    s.close()
    # a kept frame chosen with select_frame: it alone is bloomed
    n = 4
    par = TC._params(n)
    kept = []
    for twin in (True, False):
        g = scene(W, Hh, small_synthetic, PIPE, AT, frames_per_launch=4)
        g.render_frames(par)
        assert g.frames_kept() >= 3
        if twin:
            for back in range(3):
                g.select_frame(back)
                kept.append(snap(g))
            pk = P(8, mid_threshold(kept[1]["fb"]), 512)
            want = expectation(kept[1]["fb"], pk)
            assert not np.array_equal(want, host(kept[0]["fb"], pk))
        else:
            g.select_frame(1)
            g.bloom(pk)
            assert np.array_equal(g.get_frame_buffer(), want)
            for back in (0, 2):
                g.select_frame(back)
                TC.same(snap(g), kept[back])
            g.select_frame(1)
            assert np.array_equal(g.get_frame_buffer(), want) and np.array_equal(bits(g.read_z_f32()), bits(kept[1]["z"]))
        g.close()
    # a caller's buffer handed over with set_frame_buffer_device: the two copies land in it, its guards stay
    guard, nb = 64, W * Hh * 3
    buf = torch.full((guard + nb + guard,), 0xAA, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    d = scene(W, Hh, small_synthetic, PIPE, AT)
    d.set_frame_buffer_device(buf.data_ptr() + guard)
    drive(d)
    d.bloom(p)
    assert d.sync() == 0
    raw = buf.cpu().numpy()
    want = expectation(f["fb"], p)
    assert np.array_equal(raw[guard:guard + nb].reshape(Hh, W, 3), want)
    assert (raw[:guard] == 0xAA).all() and (raw[guard + nb:] == 0xAA).all(), "a guard byte changed"
    assert np.array_equal(d.get_frame_buffer(), want)
    d.close()


@pytest.mark.gpu
def test_transient_depth_stays_transient(small_synthetic):
    """Without TR_OPT_STORE_DEPTH a frame's depth stays on the chip until somebody asks for it; bloom does not.  The
    observable of the transient-depth tests: the profile's k_tile launches -- one for the frame, none for the bloom calls,
    and the depth-only repeat only when z is read afterwards."""
    W, Hh = 256, 48
    ref = scene(W, Hh, small_synthetic, PIPE, AT, auto_group=False)
    drive(ref)
    f = snap(ref)
    ref.close()
    p = P(8, mid_threshold(f["fb"]), 512)
    want = expectation(f["fb"], p)
    s = scene(W, Hh, small_synthetic, PIPE, AT, auto_group=False)
    s.profile_enable(True)
    drive(s)
    assert np.array_equal(s.get_bloom(p), want)
    s.bloom(p)
    assert s.sync() == 0
    prof = s.profile_read()
    assert prof["k_tile"]["launches"] == 1, "bloom repeated the pass for its depth: %r" % (prof,)
    assert prof.get("k_bloom", {}).get("launches") == 2 and prof["k_bloom"]["total_ms"] > 0.0, prof
    assert np.array_equal(bits(s.read_z_f32()), bits(f["z"]))
    assert s.profile_read()["k_tile"]["launches"] == 2, "the depth was not transient: the case shows nothing"
    assert np.array_equal(s.get_frame_buffer(), want)
    s.close()


@pytest.mark.gpu
def test_refusals_on_the_device_queue_nothing(small_synthetic):
    import tiny_renderer_amd as T
    from tiny_renderer_amd import _lib
    L = T.load_library()
    W, Hh = 256, 48
    s = scene(W, Hh, small_synthetic, PIPE, AT, tap=True, auto_group=True)
    band = scene(W, Hh, small_synthetic, PIPE, AT, band_rows=(16, 32))
    drive(s)
    f = snap(s)
    p = P(8, mid_threshold(f["fb"]), 512)
    want = expectation(f["fb"], p)
    # frames tr_scene_render holds back are submitted first
    drive(s, cam=1.0), drive(s, cam=2.0), drive(s)
    assert np.array_equal(s.get_bloom(p), want)
    drive(s), drive(band)
    flags = clean_flags(s)
    for field, v in BAD:
        q = P(8, p.threshold, 512)
        setattr(q, field, v)
        assert L.tr_scene_bloom(s._h, C.addressof(q), None) == _lib.TR_E_INVALID and L.tr_last_error(), (field, v)
        host_out = np.zeros((Hh, W, 3), np.uint8)
        assert L.tr_scene_get_bloom(s._h, C.addressof(q), host_out.ctypes.data) == _lib.TR_E_INVALID, (field, v)
    assert L.tr_scene_bloom(s._h, None, None) == _lib.TR_E_INVALID
    assert L.tr_scene_bloom(band._h, C.addressof(p), None) == _lib.TR_E_INVALID and b"band" in L.tr_last_error()
    with pytest.raises(T.TinyRendererError):
        band.get_bloom(p)
    fb_dev = int(s.frame_buffer_device())
    for off in (0, 3 * W, W * Hh * 3 - 1):
        assert L.tr_scene_bloom(s._h, C.addressof(p), fb_dev + off) == _lib.TR_E_INVALID and b"overlaps" in L.tr_last_error()
    small = L.tr_host_alloc(W * Hh * 3 - 1)
    assert small
    assert L.tr_scene_bloom(s._h, C.addressof(p), small) == _lib.TR_E_INVALID and b"smaller" in L.tr_last_error()
    L.tr_host_free(small)
    plain = np.zeros((Hh, W, 3), np.uint8)
    assert L.tr_scene_bloom(s._h, C.addressof(p), plain.ctypes.data) == _lib.TR_E_INVALID and b"tr_host_alloc" in L.tr_last_error()
    with pytest.raises(T.TinyRendererError):
        s.bloom(p, out=plain)
    assert not plain.any()
    assert s.sync() == 0 and np.array_equal(clean_flags(s), flags)
    assert np.array_equal(s.get_frame_buffer(), f["fb"]), "a refused call changed the frame"
    TC.same(snap(s), f)
    s.close(), band.close()


@pytest.mark.gpu
def test_chain_ao_dof_bloom_resolve(small_synthetic):
    """Ambient occlusion, then depth of field, then bloom, then resolve by 2, on 256 x 48: the host rules in that order."""
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
    bp = P(8, mid_threshold(soft), 512)
    want = expectation(soft, bp)
    s = scene(W, Hh, small_synthetic, PIPE, AT)
    drive(s)
    s.ambient_occlusion(**ao)
    s.depth_of_field(dp)
    s.bloom(bp)
    assert np.array_equal(s.resolve(2), box(want, 2))
    assert np.array_equal(s.get_frame_buffer(), want)
    assert np.array_equal(bits(s.read_z_f32()), bits(f["z"]))
    s.close()


@pytest.mark.gpu
def test_cli_bloom_writes_the_host_rule_of_the_plain_run(african_head, tmp_path):
    from tiny_renderer_amd import cli
    common = ["-p", H.asset_dir("african_head"), "-s", "phong", "--width", "256", "--height", "128", "--camera-angle", "0.3",
              "--light-angle", "0.7"]
    plain, glow = (str(tmp_path / n) for n in ("plain.ppm", "bloom.ppm"))
    assert cli.main(common + ["--out", plain]) == 0
    hd = b"P6\n256 128\n255\n"
    a = np.frombuffer(open(plain, "rb").read()[len(hd):], np.uint8).reshape(128, 256, 3)
    thr = mid_threshold(a)
    assert cli.main(common + ["--bloom", "6", "--bloom-threshold", str(thr), "--bloom-strength", "512", "--out", glow]) == 0
    b = np.frombuffer(open(glow, "rb").read()[len(hd):], np.uint8).reshape(128, 256, 3)
    assert np.array_equal(b, expectation(a, P(6, thr, 512)))


@pytest.fixture(scope="module")
def other_synthetic(built):
    import tiny_renderer_amd as T
    return T.synthetic_scene(n_lat=9, n_lon=17, tex_size=128, radius=0.75)
