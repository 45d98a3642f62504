"""The depth ramp on the device: tr_scene_ramp / tr_scene_get_ramped (k_ramp) equal tr_ramp_host in every byte.

Every comparison is np.array_equal against ramp_host of what the scene itself returns (get_frame_buffer, read_z_f32);
tests/test_ramp_host.py pins ramp_host against the rule in numpy and asserts, on the oracle's frames of these very cases,
that the span of tests/ramp_cases.py puts pixels in front of the ramp, behind it and inside it, and that every size has a
tile in which nothing is drawn and one with drawn and undrawn pixels."""
import ctypes as C

import numpy as np
import pytest

from tests import ramp_cases as RC
from tests import test_composite as TC
from tests import test_grade as TG
from tests import test_outline as TO

scene, snap, clean_flags, tiles_any = TC.scene, TC.snap, TC.clean_flags, TC.tiles_any
other_synthetic = TC.other_synthetic
device_buffer, state, same_state, box = TO.device_buffer, TO.state, TO.same_state, TO.box
GUARD = 64
IDS = ["%dx%d" % s for s in RC.SIZES]


def drive(s, cam=RC.CAM, light=RC.LIGHT, clear=True):
    TC.drive(s, cam, light, clear)


def keywords(n, mode="normal", opacity=256, repeat=False, alpha=0):
    z0, scale = RC.span(n)
    return dict(z0=z0, scale=scale, mode=mode, opacity=opacity, undrawn=RC.undrawn_of(alpha), repeat=repeat)


def host(f, tab, kw):
    import tiny_renderer_amd as T
    return T.ramp_host(f["fb"], f["z"], tab, T.ramp_params(**kw))


def same(got, want, what):
    assert got.shape == want.shape and np.array_equal(got, want), "%s: %d bytes differ" % (what, int((got != want).sum()))


def combos(all_modes, n=256):
    """Keyword sets of Scene.ramp: every mode (opacity, REPEAT and the undrawn alpha in turn), or the short list."""
    if not all_modes:
        return [keywords(n, *c) for c in RC.SHORT]
    return [keywords(n, mode, (256, 200, 128, 255, 1)[i % 5], i % 2 == 1, (0, 255, 130)[i % 3]) for i, mode in enumerate(RC.MODES)]


def drawn_tiles(f):
    return tiles_any(RC.bits(f["z"]) != RC.F32_MIN_BITS)


@pytest.mark.gpu
@pytest.mark.parametrize("W,Hh", RC.SIZES, ids=IDS)
def test_ramped_frame_equals_the_host_rule_in_all_four_forms(small_synthetic, W, Hh):
    """All seven modes at 256 x 48, the short list elsewhere: through the getter, into device memory, into a
    tr_host_alloc block and in place."""
    s = scene(W, Hh, small_synthetic, "phong", RC.table(W, Hh), tap=True)
    tab = RC.random_table(np.random.default_rng(W * Hh), 256)
    s.set_ramp(tab)
    drive(s)
    f, before, flags = snap(s), state(s), clean_flags(s)
    drawn = drawn_tiles(f)
    assert (~drawn).any() and drawn.any(), "tiles with and without drawn pixels"
    pinned = s.pinned_frame()
    for kw in combos((W, Hh) == (256, 48)):
        want = host(f, tab, kw)
        assert not np.array_equal(want, f["fb"])
        same(s.get_ramped(**kw), want, "getter %r" % (kw,))
        dev = device_buffer(W * Hh * 3, 0xAB)
        pinned[...] = 0xAB
        s.ramp(out=dev.data_ptr(), **kw)
        s.ramp(out=pinned, **kw)
        assert s.sync() == 0
        same(dev.cpu().numpy().reshape(Hh, W, 3), want, "device memory %r" % (kw,))
        same(pinned, want, "tr_host_alloc %r" % (kw,))
        assert np.array_equal(clean_flags(s), flags), "an out-of-place call changed the frame's flags"
        same(s.get_frame_buffer(), f["fb"], "out of place leaves the scene's frame")
        s.ramp(**kw)
        same(s.get_frame_buffer(), want, "in place %r" % (kw,))
        same_state(state(s), before)
        drive(s)
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("W,Hh", [(256, 48), (131, 19)], ids=["words", "bytes"])
def test_out_at_an_odd_byte_offset_between_guards(small_synthetic, W, Hh):
    import torch
    s = scene(W, Hh, small_synthetic, "specular", RC.table(W, Hh))
    tab = RC.random_table(np.random.default_rng(5), 256)
    s.set_ramp(tab)
    drive(s)
    f = snap(s)
    n = W * Hh * 3
    for kw in (keywords(256, "normal", 231, False, 255), keywords(256, "screen", 256, True, 0)):
        want = host(f, tab, kw)
        for off in (1, 2, 3):
            out = torch.full((n + 2 * GUARD + off,), 0xAA, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            assert out.data_ptr() % 4 == 0
            s.ramp(out=out.data_ptr() + GUARD + off, **kw)
            assert s.sync() == 0
            raw = out.cpu().numpy()
            same(raw[GUARD + off:GUARD + off + n].reshape(Hh, W, 3), want, "out + %d" % off)
            assert (raw[:GUARD + off] == 0xAA).all() and (raw[GUARD + off + n:] == 0xAA).all(), "a guard byte changed"
        # a tensor as `out`
        out = torch.full((Hh, W, 3), 0xAA, dtype=torch.uint8, device="cuda")
        s.ramp(out=out, **kw)
        assert s.sync() == 0
        same(out.cpu().numpy(), want, "a tensor")
    same(s.get_frame_buffer(), f["fb"], "out of place leaves the scene's frame")
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [2, 3, 1024])
def test_table_sizes(small_synthetic, n):
    W, Hh = 200, 40
    s = scene(W, Hh, small_synthetic, "phong", RC.table(W, Hh))
    tab = RC.random_table(np.random.default_rng(n), n)
    s.set_ramp(tab)
    drive(s)
    f = snap(s)
    for kw in (keywords(n, "normal", 256, False, 255), keywords(n, "add", 200, True, 0), keywords(n, "lighten", 255, False, 130)):
        want = host(f, tab, kw)
        assert not np.array_equal(want, f["fb"])
        same(s.get_ramped(**kw), want, "getter, n %d" % n)
        s.ramp(**kw)
        same(s.get_frame_buffer(), want, "in place, n %d" % n)
        drive(s)
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("W,Hh", [(384, 48), (256, 48)], ids=["384x48", "256x48"])
def test_capped_walk_equals_the_host_rule(small_synthetic, W, Hh):
    """tr_scene_debug_ramp_grid at 1, 2 and 3 workgroups over 9 and 6 tiles: every workgroup walks several tiles -- empty
    ones before the table is staged, drawn ones after, flagged ones lowered behind the barrier and round again."""
    n_tiles = ((W + 127) // 128) * ((Hh + 15) // 16)
    s = scene(W, Hh, small_synthetic, "phong", RC.table(W, Hh), tap=True)
    assert s.debug_ramp_grid(0) == 0, "no k_ramp launch yet"
    drive(s)
    f, before, flags = snap(s), state(s), clean_flags(s)
    assert flags.any() and not flags.all()
    for cap in (1, 2, 3):
        for j, kw in enumerate((keywords(256, "normal", 256, False, 255), keywords(256, "screen", 180, True, 0))):
            tab = RC.random_table(np.random.default_rng(10 * cap + j), 256)   # another table for every launch pair
            s.set_ramp(tab)
            s.debug_ramp_grid(cap)
            want = host(f, tab, kw)
            assert not np.array_equal(host(dict(f, fb=want), tab, kw), want), "ramping twice must not be ramping once"
            drive(s)
            dev = device_buffer(W * Hh * 3, 0xAB)
            s.ramp(out=dev.data_ptr(), **kw)
            assert s.sync() == 0
            assert s.debug_ramp_grid(cap) == min(cap, n_tiles)
            same(dev.cpu().numpy().reshape(Hh, W, 3), want, "out of place, cap %d" % cap)
            assert np.array_equal(clean_flags(s), flags)
            s.ramp(**kw)
            assert s.sync() == 0
            assert s.debug_ramp_grid(cap) == min(cap, n_tiles)
            same(s.get_frame_buffer(), want, "in place, cap %d" % cap)
            same_state(state(s), before)
    s.debug_ramp_grid(0)
    drive(s)
    s.ramp(**kw)
    assert s.sync() == 0 and s.debug_ramp_grid(0) == n_tiles, "without a cap: one workgroup a tile on a frame this small"
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("pipe", ["phong", "shadow"])
def test_what_stays_and_which_flags_come_down(small_synthetic, other_synthetic, pipe):
    import tiny_renderer_amd as T
    W, Hh = 384, 48
    s = scene(W, Hh, small_synthetic, pipe, RC.table(W, Hh), tap=True)
    tab = RC.random_table(np.random.default_rng(3), 256)
    s.set_ramp(tab)
    drive(s)
    f, before, flags = snap(s), state(s), clean_flags(s)
    empty = ~drawn_tiles(f)
    assert empty.any() and (flags & empty).any() and not (flags & ~empty).any(), "flagged tiles are tiles with nothing drawn"
    drive(s)                          # (reading z back made it real: the z flags are up again after a render)
    # undrawn alpha 0: a tile with nothing drawn is left behind its flag, whatever the mode
    for mode in ("normal", "add", "multiply"):
        kw = keywords(256, mode, 256, False, 0)
        s.ramp(**kw)
        assert np.array_equal(clean_flags(s), flags), mode
        same(s.get_frame_buffer(), host(f, tab, kw), mode)
        same_state(state(s), before)
        drive(s)
    # MULTIPLY and DARKEN keep a flagged tile black behind its flag, with an opaque `undrawn` too
    for mode in ("multiply", "darken"):
        kw = keywords(256, mode, 256, False, 255)
        s.ramp(**kw)
        assert np.array_equal(clean_flags(s), flags), mode
        want = host(f, tab, kw)
        assert not want[np.kron(empty, np.ones((16, 128), bool))[:Hh, :W][::-1]].any(), "black stays black under " + mode
        same(s.get_frame_buffer(), want, mode)
        drive(s)
    # undrawn alpha 255 under NORMAL: flagged tiles are stored whole and their flags come down; every consumer sees it
    kw = keywords(256, "normal", 256, False, 255)
    want = host(f, tab, kw)
    s.ramp(**kw)
    assert not clean_flags(s).any(), "a tile that holds the fog is still flagged clean"
    same(s.get_frame_buffer(), want, "get_frame_buffer")
    out = s.pinned_frame()
    out[...] = 0x5A
    s.get_frame_buffer_async(out)
    assert s.sync() == 0
    same(out, want, "the sparse read-back")
    same(s.resolve(2), box(want, 2), "resolve")
    for got, ref in zip(s.to_yuv("i420"), T.yuv_host(want, "i420")):
        assert np.array_equal(got, ref), "to_yuv"
    other = scene(200, 40, other_synthetic, "phong", RC.table(200, 40))
    drive(other, cam=1.1)
    g = snap(other)
    other.layer_from(s, 7, -3, "add", 200)
    same(other.get_frame_buffer(), T.layer_host(g["fb"], want, 7, -3, "add", 200), "layer_from")
    other.close()
    same_state(state(s), before)
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("store_depth", [False, True], ids=["transient", "stored"])
def test_depth_left_on_the_chip_a_composite_and_a_backdrop(small_synthetic, other_synthetic, store_depth):
    import tiny_renderer_amd as T
    W, Hh = 256, 48
    s = scene(W, Hh, small_synthetic, "phong", RC.table(W, Hh), store_depth=store_depth, auto_group=False)
    tab = RC.random_table(np.random.default_rng(9), 256)
    s.set_ramp(tab)
    kw = keywords(256, "normal", 220, False, 0)
    s.profile_enable(True)
    drive(s)
    s.ramp(**kw)                      # the first consumer of the frame's depth
    assert s.sync() == 0
    prof = s.profile_read()
    assert prof.get("k_ramp", {}).get("launches") == 1 and prof["k_ramp"]["total_ms"] > 0.0, prof
    got = s.get_frame_buffer()
    drive(s)
    f = snap(s)
    same(got, host(f, tab, kw), "the ramp made the depth real itself")
    # a composited frame with merged depth
    src = scene(W, Hh, other_synthetic, "phong", store_depth=store_depth)
    drive(src, cam=1.1)
    s.composite(src)
    m = snap(s)
    assert not np.array_equal(RC.bits(m["z"]), RC.bits(f["z"])), "the merge changed no depth"
    s.ramp(**kw)
    same(s.get_frame_buffer(), host(m, tab, kw), "after a composite")
    src.close()
    # a WHERE_UNDRAWN backdrop, then a ramp with undrawn alpha 0: the backdrop stays
    drive(s)
    back = np.random.default_rng(2).integers(0, 256, (Hh, W, 3), dtype=np.uint8)
    import torch
    s.layer(torch.from_numpy(back).cuda(), where="undrawn")
    step = T.layer_host(f["fb"], back, where="undrawn", z=f["z"])
    s.ramp(**kw)
    got = s.get_frame_buffer()
    same(got, host(dict(f, fb=step), tab, kw), "backdrop then ramp")
    undrawn = (RC.bits(f["z"]) == RC.F32_MIN_BITS)[::-1]
    assert np.array_equal(got[undrawn], back[undrawn]), "the ramp touched the backdrop"
    s.close()


@pytest.mark.gpu
def test_ramp_then_depth_of_field_then_grade_equals_the_host_chain(small_synthetic):
    import tiny_renderer_amd as T
    W, Hh = 200, 40
    s = scene(W, Hh, small_synthetic, "phong", RC.table(W, Hh))
    tab = T.ramp_fog(RC.FOG, 256, "exp", 3.0)
    lut = TG.random_lut(9, 4)
    s.set_ramp(tab), s.set_lut(lut)
    drive(s)
    f = snap(s)
    kw = keywords(256, "normal", 256, False, 255)
    dof = T.dof_params(focus=70.0, scale=0.2, max_radius=4, background_radius=2)
    s.ramp(**kw)
    s.depth_of_field(dof)
    s.grade()
    a = host(f, tab, kw)
    b = T.depth_of_field_host(f["z"], a, dof)
    assert not np.array_equal(a, f["fb"]) and not np.array_equal(b, a)
    same(s.get_frame_buffer(), T.grade_host(b, lut), "ramp, depth of field, grade")
    s.close()


@pytest.mark.gpu
def test_a_cleared_scene_table_swaps_and_dropping_the_table(small_synthetic):
    import tiny_renderer_amd as T
    from tiny_renderer_amd import _lib
    L = T.load_library()
    W, Hh = 200, 40
    s = scene(W, Hh, small_synthetic, "phong", RC.table(W, Hh))
    tab = RC.random_table(np.random.default_rng(8), 256)
    s.set_ramp(tab)
    s.profile_enable(True)
    black = dict(fb=np.zeros((Hh, W, 3), np.uint8), z=np.full((Hh, W), RC.F32_MIN, np.float32))
    # both shortcuts: `undrawn` over black is black -- alpha 0; MULTIPLY; a black undrawn colour
    stays = (keywords(256, "normal", 256, False, 0), keywords(256, "multiply", 256, False, 255), dict(keywords(256, "add", 200), undrawn=(0, 0, 0, 255)))
    for kw in stays:
        assert not host(black, tab, kw).any()
        s.clear()
        assert not s.get_ramped(**kw).any()
        s.clear()
        out = device_buffer(W * Hh * 3)
        s.ramp(out=out.data_ptr(), **kw)
        assert s.sync() == 0
        assert not out.cpu().numpy().any(), "zeros out of place"
        s.clear()
        s.ramp(**kw)
        assert not s.get_frame_buffer().any()
    assert "k_ramp" not in s.profile_read(), "a shortcut launched the kernel"
    # the non-black undrawn: the clear is made real and the kernel runs on raised flags
    for kw in (keywords(256, "normal", 256, False, 255), keywords(256, "screen", 100, True, 130)):
        want = host(black, tab, kw)
        assert want.any() and (want == want[0, 0]).all()
        s.clear()
        same(s.get_ramped(**kw), want, "cleared, getter")
        s.clear()
        out = device_buffer(W * Hh * 3)
        s.ramp(out=out.data_ptr(), **kw)
        assert s.sync() == 0
        same(out.cpu().numpy().reshape(Hh, W, 3), want, "cleared, out of place")
        assert not s.get_frame_buffer().any(), "the cleared scene stays cleared out of place"
        s.clear()
        s.ramp(**kw)
        same(s.get_frame_buffer(), want, "cleared, in place")
        assert not clean_flags(s).any()
    assert s.profile_read()["k_ramp"]["launches"] == 6
    # a table swapped between two calls: each call uses the table it was issued under
    drive(s)
    f = snap(s)
    kw = keywords(256, "normal", 256, False, 255)
    other = RC.random_table(np.random.default_rng(80), 256)
    a, b = device_buffer(W * Hh * 3), device_buffer(W * Hh * 3)
    s.ramp(out=a.data_ptr(), **kw)
    s.set_ramp(other)
    s.ramp(out=b.data_ptr(), **kw)
    assert s.sync() == 0
    same(a.cpu().numpy().reshape(Hh, W, 3), host(f, tab, kw), "the table the call was issued under")
    same(b.cpu().numpy().reshape(Hh, W, 3), host(f, other, kw), "the new table")
    assert not np.array_equal(host(f, tab, kw), host(f, other, kw))
    # a table of another size
    small = RC.random_table(np.random.default_rng(81), 5)
    s.set_ramp(small)
    same(s.get_ramped(**keywords(5, "normal", 256, False, 255)), host(f, small, keywords(5, "normal", 256, False, 255)), "n = 5 after n = 256")
    # dropped: a refusal
    s.set_ramp(None)
    p = T.ramp_params(**kw)
    assert L.tr_scene_ramp(s._h, C.addressof(p), None) == _lib.TR_E_INVALID
    assert L.tr_last_error().decode() == "tr_scene_ramp: the scene has no ramp table (tr_scene_set_ramp)"
    with pytest.raises(T.TinyRendererError):
        s.ramp(**kw)
    same(s.get_frame_buffer(), f["fb"], "a refused call changed the frame")
    s.close()


@pytest.mark.gpu
def test_refusals_queue_nothing(small_synthetic):
    import tiny_renderer_amd as T
    from tiny_renderer_amd import _lib
    L = T.load_library()
    W, Hh = 256, 48
    s = scene(W, Hh, small_synthetic, "phong", RC.table(W, Hh), tap=True)
    band = scene(W, Hh, small_synthetic, "phong", RC.table(W, Hh), band_rows=(16, 32))
    bare = scene(W, Hh, small_synthetic, "phong", RC.table(W, Hh))
    tab = RC.random_table(np.random.default_rng(4), 256)
    s.set_ramp(tab), band.set_ramp(tab)
    drive(s), drive(band), drive(bare)
    f, before, flags = snap(s), state(s), clean_flags(s)
    host_out = np.full((Hh, W, 3), 0xAA, np.uint8)
    dev = device_buffer(W * Hh * 3)

    def text():
        return L.tr_last_error().decode()

    def params(**kw):
        fields = dict(z0=82.0, scale=-1632.0, mode=0, opacity=256, undrawn=0xFF102030, flags=0, r0=0, r1=0)
        fields.update(kw)
        return T.RampParams(fields["z0"], fields["scale"], fields["mode"], fields["opacity"], fields["undrawn"], fields["flags"],
                            (C.c_uint32 * 2)(fields["r0"], fields["r1"]))

    good = params()
    q = C.addressof(good)
    s.profile_enable(True), band.profile_enable(True), bare.profile_enable(True)
    bad = ((dict(z0=float("nan")), ": z0 must be finite"), (dict(scale=0.0), ": scale must be finite and not 0"),
           (dict(scale=float("inf")), ": scale must be finite and not 0"), (dict(mode=7), ": mode must be TR_LAYER_NORMAL .. TR_LAYER_DIFFERENCE"),
           (dict(opacity=257), ": opacity must be 0..256"), (dict(flags=2), ": unknown flags"), (dict(r1=1), ": reserved must be 0"))
    for who, call in (("tr_scene_ramp", lambda sc, pp: L.tr_scene_ramp(sc, pp, None)),
                      ("tr_scene_get_ramped", lambda sc, pp: L.tr_scene_get_ramped(sc, pp, host_out.ctypes.data))):
        for kw, why in bad:
            p = params(**kw)
            assert call(s._h, C.addressof(p)) == _lib.TR_E_INVALID and text() == who + why, kw
            # parameters first, then the scene
            assert call(bare._h, C.addressof(p)) == _lib.TR_E_INVALID and text() == who + why, kw
        assert call(s._h, None) == _lib.TR_E_INVALID and text() == who + ": null argument"
        assert call(bare._h, q) == _lib.TR_E_INVALID and text() == who + ": the scene has no ramp table (tr_scene_set_ramp)"
        assert call(band._h, q) == _lib.TR_E_INVALID and text() == who + ": a band scene (tr_options.band_row0/1) cannot be ramped"
    assert L.tr_scene_get_ramped(s._h, q, None) == _lib.TR_E_INVALID and text() == "tr_scene_get_ramped: null argument"
    assert L.tr_scene_ramp(s._h, q, host_out.ctypes.data) == _lib.TR_E_INVALID
    assert text() == "tr_scene_ramp: `out` is neither device memory nor from tr_host_alloc (tr_scene_get_ramped takes any host memory)"
    assert L.tr_scene_ramp(s._h, q, int(s.band_tiles().frame_buffer_device) + 3) == _lib.TR_E_INVALID
    assert text() == "tr_scene_ramp: `out` overlaps a frame buffer of the scene (out == NULL ramps in place)"
    small = s.pinned_layer(4, 4)
    assert L.tr_scene_ramp(s._h, q, small.ctypes.data) == _lib.TR_E_INVALID and text() == "tr_scene_ramp: the host buffer is smaller than the frame"
    for n, rgba, why in ((1, tab.ctypes.data, ": the table's length n must be 2..TR_RAMP_MAX_N"), (1025, tab.ctypes.data, ": the table's length n must be 2..TR_RAMP_MAX_N"),
                         (4, None, ": null table")):
        assert L.tr_scene_set_ramp(s._h, n, rgba) == _lib.TR_E_INVALID and text() == "tr_scene_set_ramp" + why
    assert (host_out == 0xAA).all() and (dev.cpu().numpy() == 0x5A).all(), "a refused call wrote `out`"
    assert s.sync() == 0
    for sc in (s, band, bare):
        assert "k_ramp" not in sc.profile_read(), "a refused call queued a kernel"
    assert np.array_equal(clean_flags(s), flags)
    same(s.get_frame_buffer(), f["fb"], "a refused call changed the frame")
    same_state(state(s), before)
    # the table is still the one set before the refused tr_scene_set_ramp calls
    kw = keywords(256, "normal", 256, False, 255)
    same(s.get_ramped(**kw), host(f, tab, kw), "the table after refused swaps")
    with pytest.raises(ValueError):
        s.ramp(82.0, -1632.0, out=np.zeros((Hh, W, 3), np.float32))
    with pytest.raises(ValueError):
        s.ramp(82.0, 0.0)
    s.close(), band.close(), bare.close()


@pytest.mark.gpu
def test_span_auto_and_the_cli_in_a_child_process(built, tmp_path):
    """ramp_span_auto takes the span from the device's own depth range; --fog, --fog-background, --depth-view and
    --depth-contours write what ramp_host gives on the plain render; each run is a fresh process."""
    import os
    import subprocess
    import sys
    import tiny_renderer_amd as T
    REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    W, Hh = 200, 120
    mesh, texs = T.synthetic_scene()
    s = T.Scene(W, Hh, mesh, texs, "phong")
    drive(s, 0.3, 0.7)
    f = snap(s)
    zz = f["z"][RC.bits(f["z"]) != RC.F32_MIN_BITS]
    z0, scale = T.ramp_span_auto(s, 256)
    assert (z0, scale) == T.ramp_span(zz.max(), zz.min(), 256)
    s.close()
    common = [sys.executable, "-m", "tiny_renderer_amd.cli", "--synthetic", "-s", "phong", "--width", str(W), "--height", str(Hh), "--camera-angle", "0.3",
              "--light-angle", "0.7"]
    runs = {"plain": [], "fog": ["--fog", "200,210,230", "--fog-span", "80,30"], "fog-auto": ["--fog", "200,210,230", "--fog-kind", "exp", "--fog-density", "3", "--fog-background"],
            "grey": ["--depth-view", "grey"], "colour": ["--depth-view", "colour", "--fog-span", "auto"], "contours": ["--depth-contours", "8"]}
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    hd = b"P6\n%d %d\n255\n" % (W, Hh)
    got = {}
    for name, extra in runs.items():
        path = str(tmp_path / (name + ".ppm"))
        done = subprocess.run(common + extra + ["--out", path], capture_output=True, text=True, cwd=REPO, env=env, timeout=120)
        assert done.returncode == 0, done.stdout + done.stderr
        got[name] = np.frombuffer(open(path, "rb").read()[len(hd):], np.uint8).reshape(Hh, W, 3)
    same(got["plain"], f["fb"], "the child's plain render")
    auto = T.ramp_span(zz.max(), zz.min(), 256)
    same(got["fog"], T.ramp_host(f["fb"], f["z"], T.ramp_fog(RC.FOG), T.ramp_params(*T.ramp_span(80.0, 30.0, 256))), "--fog with a span")
    same(got["fog-auto"], T.ramp_host(f["fb"], f["z"], T.ramp_fog(RC.FOG, 256, "exp", 3.0), T.ramp_params(*auto, undrawn=RC.FOG + (255,))), "--fog-background, auto span")
    same(got["grey"], T.ramp_host(f["fb"], f["z"], T.ramp_grey(256)[::-1].copy(), T.ramp_params(*auto)), "--depth-view grey")
    same(got["colour"], T.ramp_host(f["fb"], f["z"], T.ramp_false_colour(256), T.ramp_params(*auto)), "--depth-view colour")
    same(got["contours"], T.ramp_host(f["fb"], f["z"], T.ramp_contours(256, 32), T.ramp_params(*auto)), "--depth-contours")
    bad = subprocess.run(common + ["--fog-kind", "exp"], capture_output=True, text=True, cwd=REPO, env=env, timeout=120)
    assert bad.returncode != 0 and "--fog" in bad.stderr
