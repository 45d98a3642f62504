"""Layers on the device: tr_scene_layer / tr_scene_layer_from_scene / tr_scene_get_layered (k_layer) equal tr_layer_host
in every byte.

Every comparison is np.array_equal against layer_host of what the scene itself returns (get_frame_buffer, read_z_f32);
tests/test_layer_host.py pins layer_host against the rule in numpy.  The sizes and placements are tests/layer_cases.py's."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import dense_cases as DC
from tests import layer_cases as LC
from tests import outline_cases as OC
from tests import test_composite as TC
from tests import test_outline as TO
from tests import test_resolve as TR

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
scene, snap, clean_flags = TC.scene, TC.snap, TC.clean_flags
other_synthetic = TC.other_synthetic
device_buffer, state, same_state, box = TO.device_buffer, TO.state, TO.same_state, TO.box
PIPELINES = TR.PIPELINES
GUARD = 64


def drive(s, cam=OC.CAM, light=OC.LIGHT, clear=True):
    TC.drive(s, cam, light, clear)


def host(f, img, **kw):
    import tiny_renderer_amd as T
    return T.layer_host(f["fb"], img, z=f["z"] if kw.get("where") else None, **kw)


def on_device(img):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(img)).cuda()
    torch.cuda.synchronize()
    return t


def same(got, want, what):
    assert got.shape == want.shape and np.array_equal(got, want), "%s: %d bytes differ" % (what, int((got != want).sum()))


def combos(all_modes):
    """Keyword sets of Scene.layer: every mode x format (opacities in turn), or the short list; then the flags."""
    out = []
    if all_modes:
        for i, mode in enumerate(LC.MODES):
            for j, fmt in enumerate(LC.FORMATS):
                out.append((fmt, dict(mode=mode, opacity=(256, 200, 128, 255, 1)[(i + 2 * j) % 5])))
    else:
        out += [(fmt, dict(mode=mode, opacity=op)) for mode, fmt, op in LC.SHORT]
    out.append(("rgb8", dict(mode="normal", where="undrawn")))
    out.append(("rgba8", dict(mode="screen", opacity=180, where="drawn", key=LC.KEY)))
    out.append(("rgb8", dict(mode="lighten", key=LC.KEY)))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("W,Hh", LC.SIZES, ids=["%dx%d" % s for s in LC.SIZES])
def test_layered_frame_equals_the_host_rule(small_synthetic, W, Hh):
    """Every placement x (all modes x formats at 256 x 48, a short list elsewhere) through the getter, out of place;
    the short list in place as well."""
    rng = np.random.default_rng(W * Hh)
    s = scene(W, Hh, small_synthetic, "phong", OC.table(W, Hh))
    drive(s)
    f, before = snap(s), state(s)
    drawn = LC.bits(f["z"]) != LC.F32_MIN_BITS
    assert drawn.any() and not drawn.all()
    for name, x, y, w, h in LC.placements(W, Hh):
        for fmt, kw in combos((W, Hh) == (256, 48)):
            img = LC.random_layer(rng, w, h, 4 if fmt == "rgba8" else 3, kw.get("key"))
            want = host(f, img, x=x, y=y, **kw)
            if name == "miss":
                assert np.array_equal(want, f["fb"])
            same(s.get_layered(on_device(img), x, y, **kw), want, "%s %r getter" % (name, kw))
    same(s.get_frame_buffer(), f["fb"], "the getter left the frame alone")
    for name, x, y, w, h in LC.placements(W, Hh):
        for fmt, kw in combos(False):
            img = LC.random_layer(rng, w, h, 4 if fmt == "rgba8" else 3, kw.get("key"))
            dev = on_device(img)
            drive(s)
            s.layer(dev, x, y, **kw)
            same(s.get_frame_buffer(), host(f, img, x=x, y=y, **kw), "%s %r in place" % (name, kw))
        same_state(state(s), before)
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("W,Hh", [(256, 48), (131, 19)], ids=["words", "bytes"])
def test_any_layer_alignment_and_stride_between_guards(small_synthetic, W, Hh):
    """The layer carved out of a larger 0xAA tensor at byte offsets 0..3 with a padded stride, `out` between guards:
    the same result at every offset, no guard byte changed, the layer's tensor unchanged."""
    import torch
    s = scene(W, Hh, small_synthetic, "specular", OC.table(W, Hh))
    drive(s)
    f = snap(s)
    rng = np.random.default_rng(5)
    n = W * Hh * 3
    for ch in (3, 4):
        w, h, x, y = 77, 13, 9, 3
        img = LC.random_layer(rng, w, h, ch)
        stride = w * ch + 7
        want = host(f, img, x=x, y=y, mode="add", opacity=231)
        for off in (0, 1, 2, 3):
            # the layer's last byte lies 29 bytes before the tensor's end: a word read behind it cannot fault
            total = stride * (h - 1) + w * ch
            block = torch.full((GUARD + off + total + 29,), 0xAA, dtype=torch.uint8, device="cuda")
            rows = torch.as_strided(block, (h, w, ch), (stride, ch, 1), GUARD + off)
            rows.copy_(torch.from_numpy(img).cuda())
            torch.cuda.synchronize()
            assert block.data_ptr() % 4 == 0 and rows.data_ptr() % 4 == (GUARD + off) % 4
            keep = block.cpu().numpy().copy()
            out = torch.full((n + 2 * GUARD,), 0xAA, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            s.layer(rows, x, y, "add", 231, out=out.data_ptr() + GUARD)
            assert s.sync() == 0
            raw = out.cpu().numpy()
            same(raw[GUARD:GUARD + n].reshape(Hh, W, 3), want, "%d channels at offset %d" % (ch, off))
            assert (raw[:GUARD] == 0xAA).all() and (raw[GUARD + n:] == 0xAA).all(), "a guard byte changed"
            assert np.array_equal(block.cpu().numpy(), keep), "the layer's memory changed"
            same(s.get_layered(rows, x, y, "add", 231), want, "getter at offset %d" % off)
        # `out` off by one byte takes the byte form
        out = torch.full((n + 2 * GUARD + 1,), 0xAA, dtype=torch.uint8, device="cuda")
        s.layer(on_device(img), x, y, "add", 231, out=out.data_ptr() + GUARD + 1)
        assert s.sync() == 0
        raw = out.cpu().numpy()
        same(raw[GUARD + 1:GUARD + 1 + n].reshape(Hh, W, 3), want, "out + 1")
        assert (raw[:GUARD + 1] == 0xAA).all() and (raw[GUARD + 1 + n:] == 0xAA).all()
        # a page-locked block as the layer and as `out`
        pinned, target = s.pinned_layer(w, h, ch), s.pinned_frame()
        pinned[...] = img
        target[...] = 0xAA
        s.layer(pinned, x, y, "add", 231, out=target)
        assert s.sync() == 0
        same(target, want, "tr_host_alloc layer and out")
    same(s.get_frame_buffer(), f["fb"], "out of place leaves the scene's frame")
    s.close()


@pytest.mark.gpu
def test_flagged_tiles_in_place_and_what_later_consumers_see(small_synthetic):
    W, Hh = 384, 48
    s = scene(W, Hh, small_synthetic, "phong", OC.table(W, Hh))
    drive(s)
    f, flags = snap(s), clean_flags(s)
    assert flags.any() and not flags.all(), "flagged and unflagged tiles"
    rng = np.random.default_rng(3)
    # a layer that misses the frame changes nothing, flags included
    s.layer(on_device(LC.random_layer(rng, 9, 9, 3)), W, 0)
    s.layer(on_device(LC.random_layer(rng, 9, 9, 3)), 5, -9)
    s.layer(on_device(LC.random_layer(rng, 9, 9, 3)), 5, 5, opacity=0)
    assert np.array_equal(clean_flags(s), flags)
    same(s.get_frame_buffer(), f["fb"], "a miss")
    # MULTIPLY and DARKEN in place leave the flags of untouched and black tiles up
    img = LC.random_layer(rng, W - 20, Hh - 10, 3)
    for mode in ("multiply", "darken"):
        drive(s)
        s.layer(on_device(img), 10, 5, mode)
        assert np.array_equal(clean_flags(s), flags), mode
        same(s.get_frame_buffer(), host(f, img, x=10, y=5, mode=mode), mode)
    # WHERE_DRAWN leaves tiles in which nothing is drawn alone, flag and all
    drive(s)
    s.layer(on_device(img), 10, 5, where="drawn")
    assert np.array_equal(clean_flags(s), flags)
    same(s.get_frame_buffer(), host(f, img, x=10, y=5, where="drawn"), "where drawn")
    # NORMAL into flagged tiles: an inset that ends inside the middle tile column and touches flagged tiles
    inset = LC.random_layer(rng, 150, 30, 4)
    drive(s)
    s.layer(on_device(inset), 100, 9, opacity=220)
    after = clean_flags(s)
    want = host(f, inset, x=100, y=9, opacity=220)
    touched = TC.tiles_any(np.pad(np.ones((30, 150), bool), ((9, Hh - 39), (100, W - 250)))[::-1])
    assert (flags & touched).any(), "the inset reaches a flagged tile"
    assert not (after & touched).any() and np.array_equal(after & ~touched, flags & ~touched), "flags: lowered where written, kept elsewhere"
    same(s.get_frame_buffer(), want, "get_frame_buffer")
    out = s.pinned_frame()
    out[...] = 0x5A
    s.get_frame_buffer_async(out)
    assert s.sync() == 0
    same(out, want, "the sparse read-back")
    same(s.resolve(2), box(want, 2), "resolve")
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("W,Hh", DC.SIZES)
def test_where_undrawn_is_the_dense_frames_paste_and_where_drawn_its_complement(small_synthetic, W, Hh):
    s = scene(W, Hh, small_synthetic, DC.PIPE, DC.table(W, Hh))
    TC.drive(s, DC.CAM, DC.LIGHT)
    f = snap(s)
    back = DC.backdrop("noise", W, Hh)
    dev = on_device(back)
    same(s.get_layered(dev, where="undrawn"), DC.paste(back, f["fb"], f["z"]), "a backdrop is the dense frame")
    same(s.get_layered(dev, where="drawn"), DC.paste(f["fb"], back, f["z"]), "the complement")
    s.layer(dev, where="undrawn")
    same(s.get_frame_buffer(), DC.paste(back, f["fb"], f["z"]), "in place")
    assert not clean_flags(s).any(), "every tile holds the backdrop now"
    assert np.array_equal(LC.bits(s.read_z_f32()), LC.bits(f["z"])), "a backdrop pixel is still not drawn"
    s.close()


@pytest.mark.gpu
def test_transient_depth_stays_transient_without_a_where_flag(small_synthetic):
    W, Hh = 256, 48
    s = scene(W, Hh, small_synthetic, "phong", OC.table(W, Hh), auto_group=False)
    img = on_device(LC.random_layer(np.random.default_rng(1), 90, 20, 4))
    out = device_buffer(W * Hh * 3)
    s.profile_enable(True)
    drive(s)
    s.layer(img, 20, 10, out=out.data_ptr())
    s.layer(img, 20, 10, "screen")
    assert s.sync() == 0
    prof = s.profile_read()
    assert prof["k_tile"]["launches"] == 1 and prof.get("k_tile_depth", {}).get("launches", 0) == 0, "a layer repeated the pass for its depth: %r" % (prof,)
    assert prof.get("k_layer", {}).get("launches") == 2 and prof["k_layer"]["total_ms"] > 0.0, prof
    s.layer(img, 20, 10, where="drawn")
    assert s.sync() == 0
    prof = s.profile_read()
    tiles = prof["k_tile"]["launches"] + prof.get("k_tile_depth", {}).get("launches", 0)
    assert tiles == 2, "the depth was not transient: the case shows nothing (%r)" % (prof,)
    s.close()


@pytest.mark.gpu
def test_layer_from_another_scene_of_another_size(small_synthetic, other_synthetic):
    import tiny_renderer_amd as T
    from tiny_renderer_amd import _lib
    L = T.load_library()
    W, Hh = 256, 48
    dst = scene(W, Hh, small_synthetic, "phong", OC.table(W, Hh))
    src = scene(200, 40, other_synthetic, "phong", OC.table(200, 40))
    drive(dst), drive(src, cam=1.1)
    f, g = snap(dst), snap(src)
    src_flags, src_state = clean_flags(src), state(src)
    assert src_flags.any() and not src_flags.all(), "flagged and unflagged source tiles"
    for x, y, kw in ((31, 5, dict()), (-50, -7, dict(mode="add", opacity=200)), (130, 20, dict(mode="difference", key=(0, 0, 0))),
                     (57, 3, dict(where="undrawn")), (W, 0, dict())):
        dst.layer_from(src, x, y, **kw)
        same(dst.get_frame_buffer(), host(f, g["fb"], x=x, y=y, **kw), "layer_from %r" % ((x, y, kw),))
        drive(dst)
    out = device_buffer(W * Hh * 3)
    dst.layer_from(src, 31, 5, "screen", out=out.data_ptr())
    assert dst.sync() == 0
    same(out.cpu().numpy().reshape(Hh, W, 3), host(f, g["fb"], x=31, y=5, mode="screen"), "out of place")
    same(dst.get_frame_buffer(), f["fb"], "dst's frame stays out of place")
    # a logically cleared source is a layer of zeros
    src.clear()
    dst.layer_from(src, 31, 5)
    same(dst.get_frame_buffer(), host(f, np.zeros_like(g["fb"]), x=31, y=5), "a cleared source")
    drive(src, cam=1.1), drive(dst)
    same(src.get_frame_buffer(), g["fb"], "src renders as before")
    assert np.array_equal(clean_flags(src), src_flags)
    same_state(state(src), src_state)
    # refusals
    def text():
        return L.tr_last_error().decode()
    p = T.layer_params(0, 0)
    q = C.addressof(p)
    assert L.tr_scene_layer_from_scene(dst._h, q, dst._h, None) == _lib.TR_E_INVALID and text() == "tr_scene_layer_from_scene: dst and src are the same scene"
    band = scene(W, Hh, small_synthetic, "phong", OC.table(W, Hh), band_rows=(16, 32))
    drive(band)
    assert L.tr_scene_layer_from_scene(band._h, q, src._h, None) == _lib.TR_E_INVALID and text().startswith("tr_scene_layer_from_scene: a band scene")
    assert L.tr_scene_layer_from_scene(dst._h, q, band._h, None) == _lib.TR_E_INVALID and text().startswith("tr_scene_layer_from_scene: src is a band scene")
    sized = T.layer_params(4, 4)
    assert L.tr_scene_layer_from_scene(dst._h, C.addressof(sized), src._h, None) == _lib.TR_E_INVALID
    assert text() == "tr_scene_layer_from_scene: width, height and stride must be 0 (they are taken from src)"
    same(dst.get_frame_buffer(), f["fb"], "a refused call changed nothing")
    dst.close(), src.close(), band.close()


@pytest.mark.gpu
def test_in_place_twice_out_of_place_and_a_cleared_scene(small_synthetic):
    W, Hh = 200, 40
    rng = np.random.default_rng(8)
    img = LC.random_layer(rng, 120, 25, 4)
    dev = on_device(img)
    kw = dict(x=33, y=7, mode="screen", opacity=150)
    s = scene(W, Hh, small_synthetic, "phong", OC.table(W, Hh), auto_group=True)
    drive(s, cam=1.0), drive(s, cam=2.0), drive(s)        # (held-back frames are submitted first)
    ref = scene(W, Hh, small_synthetic, "phong", OC.table(W, Hh))
    drive(ref)
    f = snap(ref)
    ref.close()
    once = host(f, img, **kw)
    twice = host(dict(f, fb=once), img, **kw)
    assert not np.array_equal(once, f["fb"]) and not np.array_equal(twice, once)
    s.layer(dev, **kw)
    same(s.get_frame_buffer(), once, "once")
    s.layer(dev, **kw)
    same(s.get_frame_buffer(), twice, "twice")
    # a cleared scene: out of place the layer over black, through every target; in place the kernel runs on the flags
    black = dict(fb=np.zeros((Hh, W, 3), np.uint8), z=np.full((Hh, W), LC.F32_MIN, np.float32))
    for kw2 in (dict(x=33, y=7), dict(x=33, y=7, mode="multiply"), dict(x=-5, y=30, mode="add", opacity=99), dict(x=33, y=7, where="undrawn"),
                dict(x=33, y=7, where="drawn"), dict(x=W, y=0)):
        want = host(black, img, **kw2)
        s.clear()
        same(s.get_layered(dev, **kw2), want, "cleared, getter %r" % (kw2,))
        s.clear()
        out = device_buffer(W * Hh * 3)
        s.layer(dev, out=out.data_ptr(), **kw2)
        assert s.sync() == 0
        same(out.cpu().numpy().reshape(Hh, W, 3), want, "cleared, out of place %r" % (kw2,))
        assert not s.get_frame_buffer().any(), "the cleared scene stays cleared out of place"
        s.clear()
        s.layer(dev, **kw2)
        same(s.get_frame_buffer(), want, "cleared, in place %r" % (kw2,))
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("pipe", PIPELINES)
def test_every_pipeline(small_synthetic, pipe):
    W, Hh = 256, 48
    s = scene(W, Hh, small_synthetic, pipe, OC.table(W, Hh), tap=True)
    drive(s)
    f, before = snap(s), state(s)
    img = LC.random_layer(np.random.default_rng(2), 140, 31, 4, LC.KEY)
    kw = dict(x=61, y=-3, mode="add", opacity=210, key=LC.KEY, where="drawn")
    same(s.get_layered(on_device(img), **kw), host(f, img, **kw), pipe)
    s.layer(on_device(img), **kw)
    same(s.get_frame_buffer(), host(f, img, **kw), pipe + " in place")
    same_state(state(s), before)
    s.close()


@pytest.mark.gpu
def test_refusals_queue_nothing(small_synthetic):
    import tiny_renderer_amd as T
    from tiny_renderer_amd import _lib
    L = T.load_library()
    W, Hh = 256, 48
    s = scene(W, Hh, small_synthetic, "phong", OC.table(W, Hh))
    band = scene(W, Hh, small_synthetic, "phong", OC.table(W, Hh), band_rows=(16, 32))
    drive(s), drive(band)
    before, flags = snap(s), clean_flags(s)
    img = on_device(LC.random_layer(np.random.default_rng(4), 16, 8, 3))
    host_img, host_out = np.zeros((8, 16, 3), np.uint8), np.full((Hh, W, 3), 0xAA, np.uint8)
    dev = device_buffer(W * Hh * 3)

    def text():
        return L.tr_last_error().decode()

    p = T.layer_params(16, 8)
    q = C.addressof(p)
    s.profile_enable(True), band.profile_enable(True)
    for who, call in (("tr_scene_layer", lambda sc, pp, im: L.tr_scene_layer(sc, pp, im, None)),
                      ("tr_scene_get_layered", lambda sc, pp, im: L.tr_scene_get_layered(sc, pp, im, host_out.ctypes.data))):
        for fields, why in (((7, 0, 0, 256), ": mode must be TR_LAYER_NORMAL .. TR_LAYER_DIFFERENCE"), ((0, 2, 0, 256), ": format must be TR_LAYER_RGB8 or TR_LAYER_RGBA8"),
                            ((0, 0, 8, 256), ": unknown flags"), ((0, 0, 6, 256), ": TR_LAYER_WHERE_DRAWN and TR_LAYER_WHERE_UNDRAWN exclude each other"),
                            ((0, 0, 0, 257), ": opacity must be 0..256")):
            bad = T.LayerParams(*fields, 0, 0, 16, 8, 0, (C.c_uint8 * 4)())
            assert call(s._h, C.addressof(bad), img.data_ptr()) == _lib.TR_E_INVALID and text() == who + why
        for size, why in (((0, 8, 0), ": width and height must be 1..8192"), ((16, 8193, 0), ": width and height must be 1..8192"),
                          ((16, 8, 47), ": stride must be 0 or at least the bytes of a row")):
            bad = T.LayerParams(0, 0, 0, 256, 0, 0, size[0], size[1], size[2], (C.c_uint8 * 4)())
            assert call(s._h, C.addressof(bad), img.data_ptr()) == _lib.TR_E_INVALID and text() == who + why
        assert call(s._h, None, img.data_ptr()) == _lib.TR_E_INVALID and text() == who + ": null argument"
        assert call(s._h, q, None) == _lib.TR_E_INVALID and text() == who + ": null argument"
        assert call(band._h, q, img.data_ptr()) == _lib.TR_E_INVALID and text().startswith(who + ": a band scene (tr_options.band_row0/1) cannot be layered")
        assert call(s._h, q, host_img.ctypes.data) == _lib.TR_E_INVALID
        assert text() == who + ": `image` is neither device memory nor from tr_host_alloc (tr_layer_host takes any host memory)"
        t = s.band_tiles()
        assert call(s._h, q, int(t.frame_buffer_device) + 5) == _lib.TR_E_INVALID and text() == who + ": `image` overlaps a frame buffer of the scene"
    small = s.pinned_layer(4, 4)
    assert L.tr_scene_layer(s._h, q, small.ctypes.data, None) == _lib.TR_E_INVALID and text() == "tr_scene_layer: the host buffer `image` is smaller than the layer"
    assert L.tr_scene_layer(s._h, q, img.data_ptr(), host_out.ctypes.data) == _lib.TR_E_INVALID
    assert text() == "tr_scene_layer: `out` is neither device memory nor from tr_host_alloc (tr_scene_get_layered takes any host memory)"
    assert L.tr_scene_layer(s._h, q, img.data_ptr(), int(s.band_tiles().frame_buffer_device) + 3) == _lib.TR_E_INVALID
    assert text() == "tr_scene_layer: `out` overlaps a frame buffer of the scene (out == NULL layers in place)"
    big = T.layer_params(W, Hh)
    assert L.tr_scene_layer(s._h, C.addressof(big), dev.data_ptr(), dev.data_ptr() + 9) == _lib.TR_E_INVALID and text() == "tr_scene_layer: `image` overlaps `out`"
    assert (host_out == 0xAA).all() and (dev.cpu().numpy() == 0x5A).all(), "a refused call wrote `out`"
    for q_, f_ in ((s, before),):
        assert q_.sync() == 0
        assert "k_layer" not in q_.profile_read(), "a refused call queued a kernel"
        assert np.array_equal(clean_flags(q_), flags)
        same(q_.get_frame_buffer(), f_["fb"], "a refused call changed the frame")
    assert "k_layer" not in band.profile_read()
    with pytest.raises(ValueError):
        s.layer(123456, 0, 0)                    # a device address needs its sizes
    with pytest.raises(ValueError):
        s.layer(img.to(dtype=__import__("torch").float32), 0, 0)
    s.close(), band.close()


@pytest.mark.gpu
def test_cli_backdrop_overlay_and_vignette_in_a_child_process(built, tmp_path):
    """--backdrop, --overlay and --vignette write what layer_host gives on the plain render; each run is a fresh process."""
    import tiny_renderer_amd as T
    W, Hh = 200, 120
    common = [sys.executable, "-m", "tiny_renderer_amd.cli", "--synthetic", "-s", "phong", "--width", str(W), "--height", str(Hh), "--camera-angle", "0.3",
              "--light-angle", "0.7"]
    rng = np.random.default_rng(6)
    back, mark = LC.random_layer(rng, W, Hh, 3), LC.random_layer(rng, 50, 30, 3)
    back_tga, mark_tga = str(tmp_path / "back.tga"), str(tmp_path / "mark.tga")
    T.save_tga(back_tga, back), T.save_tga(mark_tga, mark)
    assert np.array_equal(T.load_tga(back_tga), back)
    runs = {"plain": [], "backdrop": ["--backdrop", back_tga], "sky": ["--backdrop", "10,20,200:250,240,230"],
            "overlay": ["--overlay", mark_tga, "--overlay-at=-7,100", "--overlay-opacity", "180", "--overlay-mode", "screen"], "vignette": ["--vignette", "160"],
            "all": ["--backdrop", back_tga, "--overlay", mark_tga, "--overlay-at", "33,9", "--vignette", "90"]}
    got = {}
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    hd = b"P6\n%d %d\n255\n" % (W, Hh)
    for name, extra in runs.items():
        path = str(tmp_path / (name + ".ppm"))
        done = subprocess.run(common + extra + ["--out", path], capture_output=True, text=True, cwd=REPO, env=env, timeout=120)
        assert done.returncode == 0, done.stdout + done.stderr
        got[name] = np.frombuffer(open(path, "rb").read()[len(hd):], np.uint8).reshape(Hh, W, 3)
    # the same frame here, for its depth
    mesh, texs = T.synthetic_scene()
    s = T.Scene(W, Hh, mesh, texs, "phong")
    drive(s, 0.3, 0.7)
    f = snap(s)
    s.close()
    same(got["plain"], f["fb"], "the child's plain render")
    same(got["backdrop"], T.layer_host(f["fb"], back, where="undrawn", z=f["z"]), "--backdrop FILE")
    same(got["sky"], T.layer_host(f["fb"], T.layer_gradient(W, Hh, (10, 20, 200), (250, 240, 230)), where="undrawn", z=f["z"]), "--backdrop colours")
    same(got["overlay"], T.layer_host(f["fb"], mark, -7, 100, "screen", 180), "--overlay")
    same(got["vignette"], T.layer_host(f["fb"], T.layer_vignette(W, Hh, 160), mode="multiply"), "--vignette")
    step = T.layer_host(T.layer_host(f["fb"], back, where="undrawn", z=f["z"]), mark, 33, 9)
    same(got["all"], T.layer_host(step, T.layer_vignette(W, Hh, 90), mode="multiply"), "all three in their order")
    bad = subprocess.run(common + ["--overlay-opacity", "100"], capture_output=True, text=True, cwd=REPO, env=env, timeout=120)
    assert bad.returncode != 0 and "--overlay" in bad.stderr
