"""Outlines on the device: tr_scene_outline / tr_scene_get_outlined (k_outline) equal tr_outline_host in every byte.

The expectation is the host rule applied to a snapshot of colour and z of the very frame that is then rendered again and
outlined (the pattern of tests/test_ambient_occlusion.py): reading a scene makes its depth real and lowers flags, so the
frame that is outlined is a fresh one.  tests/test_outline_host.py pins the host rule and shows on the CPU that the cases
here are not vacuous; sizes, placement and thresholds are shared through tests/outline_cases.py."""
import ctypes as C

import numpy as np
import pytest

from tests import outline_cases as OC
from tests import test_composite as TC

F32_MIN_BITS = OC.F32_MIN_BITS
bits, scene, snap, clean_flags, tiles_any = TC.bits, TC.scene, TC.snap, TC.clean_flags, TC.tiles_any
SPREADS = TC._small(-0.4, -0.28, 0.0, 0.3)   # on 512 x 64: rows 18..30 of tile row 1, so ink of radius 3 reaches empty tile row 0


def drive(s, cam=OC.CAM, light=OC.LIGHT, clear=True):
    TC.drive(s, cam, light, clear)


def params(**kw):
    import tiny_renderer_amd as T
    return T.outline_params(**kw)


def host(f, **kw):
    import tiny_renderer_amd as T
    return T.outline_host(f["z"], f["fb"], params(**kw))


def device_buffer(n, fill=0x5A):
    import torch
    buf = torch.full((n,), fill, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return buf


def state(s):
    """Everything a call must leave alone: z, winner words, shadow buffer."""
    out = {"z": bits(s.read_z_f32()), "win": s.read_winner_u32() if getattr(s, "_tap", False) else None}
    out["shadow"] = bits(s.read_shadow_f32()) if s.pipeline in ("shadow", "occlusion") else None
    return out


def same_state(a, b):
    for k in a:
        assert (a[k] is None and b[k] is None) or np.array_equal(a[k], b[k]), k + " changed"


def box(img, f):
    """Scene.resolve's contract: the rounded mean of every f x f block."""
    Hh, W, _ = img.shape
    return ((img.reshape(Hh // f, f, W // f, f, 3).astype(np.uint32).sum((1, 3)) + f * f // 2) // (f * f)).astype(np.uint8)


@pytest.mark.gpu
@pytest.mark.parametrize("store_depth", [False, True], ids=["transient", "stored"])
@pytest.mark.parametrize("pipe", ["phong", "shadow"])
@pytest.mark.parametrize("W,Hh", OC.SIZES)
def test_outlined_frame_equals_the_host_rule_in_all_four_forms(small_synthetic, W, Hh, pipe, store_depth):
    """Radius 0, 1 and 3, creases off and on, ONLY with black and with another paper, opacity 256 and 100; into device
    memory, into tr_host_alloc memory, through the getter and in place."""
    import torch
    s = scene(W, Hh, small_synthetic, pipe, OC.table(W, Hh), tap=True, store_depth=store_depth)
    drive(s)
    f, before = snap(s), state(s)
    assert (bits(f["z"]) != F32_MIN_BITS).any() and (bits(f["z"]) == F32_MIN_BITS).any()
    dev, pinned = device_buffer(W * Hh * 3), s.pinned_frame()
    changed = 0
    for kw in OC.gpu_params():
        want = host(f, **kw)
        changed += int((want != f["fb"]).any(-1).sum())
        p = params(**kw)
        drive(s)                                          # a fresh frame: depth and flags as a render leaves them
        dev[:] = 0x5A
        torch.cuda.synchronize()                          # (torch fills on its own stream: not behind the scene's kernel)
        s.outline(p, out=dev.data_ptr())
        assert s.sync() == 0
        got = dev.cpu().numpy().reshape(Hh, W, 3)
        assert np.array_equal(got, want), "device %r: %d bytes differ" % (kw, int((got != want).sum()))
        pinned[:] = 0xA5
        s.outline(p, out=pinned)
        assert s.sync() == 0 and np.array_equal(pinned, want), "pinned %r" % (kw,)
        assert np.array_equal(s.get_outlined(p), want), "getter %r" % (kw,)
        assert np.array_equal(s.get_frame_buffer(), f["fb"]), "out of place wrote the frame"
        drive(s)
        s.outline(p)
        assert s.sync() == 0
        got = s.get_frame_buffer()
        assert np.array_equal(got, want), "in place %r: %d bytes differ" % (kw, int((got != want).sum()))
        same_state(state(s), before)
    assert changed > 0
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("only", [None, (0, 0, 0), OC.PAPER], ids=["frame", "black", "paper"])
def test_flags_after_an_in_place_call_and_what_their_consumers_read(small_synthetic, only):
    """512 x 64 is 4 x 4 tiles and the model leaves most of them empty; ink of radius 3 spreads from its top rows into an
    empty tile row.  A flag that stays up must still mean zeros nobody reads, so: down where ink (or paper) was written,
    up elsewhere -- and get_frame_buffer, resolve(2) and the sparse read-back all return the host rule's frame."""
    W, Hh = 512, 64
    kw = dict(radius=3, depth_step=OC.DEPTH_STEP, crease=OC.CREASE_T, ink=OC.INK)
    if only is not None:
        kw.update(only=True, paper=only)
    s = scene(W, Hh, small_synthetic, "phong", SPREADS)
    drive(s)
    f, flags = snap(s), clean_flags(s)
    drawn_tiles = tiles_any(bits(f["z"]) != F32_MIN_BITS)
    assert np.array_equal(flags, ~drawn_tiles)
    inked_tiles = tiles_any(OC.inked_np(OC.kinds_np(f["z"], OC.DEPTH_STEP, OC.CREASE_T), 3))
    assert (inked_tiles & flags).any(), "no ink spreads into a flagged tile: the case shows nothing"
    assert (~inked_tiles & flags).any(), "every flagged tile receives ink"
    want = host(f, **kw)
    assert np.array_equal(want, OC.rule_np(f["z"], f["fb"], **kw))
    if only is None:
        expect = flags & ~inked_tiles
    elif only == (0, 0, 0):
        expect = flags & ~inked_tiles
    else:
        expect = np.zeros_like(flags)
    p = params(**kw)
    drive(s), s.outline(p)
    assert np.array_equal(clean_flags(s), expect), "flags: down where the kernel wrote a flagged tile, up where it did not"
    assert np.array_equal(s.get_frame_buffer(), want)
    drive(s), s.outline(p)
    assert np.array_equal(s.resolve(2), box(want, 2)), "a consumer that skips clean tiles lost ink"
    out = s.pinned_frame()
    out[:] = 0x5A
    drive(s), s.outline(p)
    s.get_frame_buffer_async(out)
    assert s.sync() == 0 and np.array_equal(out, want), "the sparse read-back"
    assert np.array_equal(bits(s.read_z_f32()), bits(f["z"]))
    # out of place over the same flags: every byte, the scene's flags as they were
    drive(s)
    dev = device_buffer(W * Hh * 3)
    s.outline(p, out=dev.data_ptr())
    assert np.array_equal(clean_flags(s), flags)
    assert np.array_equal(dev.cpu().numpy().reshape(Hh, W, 3), want)
    s.close()


@pytest.mark.gpu
def test_in_place_twice_is_the_rule_twice_and_held_back_frames_are_submitted(small_synthetic):
    W, Hh = 256, 48
    kw = dict(radius=1, depth_step=OC.DEPTH_STEP, crease=OC.CREASE_T, ink=OC.INK, opacity=100)
    ref = scene(W, Hh, small_synthetic, "phong", OC.table(W, Hh))
    drive(ref)
    f = snap(ref)
    once = host(f, **kw)
    twice = host(dict(f, fb=once), **kw)
    assert not np.array_equal(once, f["fb"]) and not np.array_equal(twice, once)
    ref.close()
    s = scene(W, Hh, small_synthetic, "phong", OC.table(W, Hh), auto_group=True)
    drive(s, cam=1.0), drive(s, cam=2.0), drive(s)
    s.outline(params(**kw))
    assert np.array_equal(s.get_frame_buffer(), once)
    s.outline(params(**kw))
    assert np.array_equal(s.get_frame_buffer(), twice), "outlining twice is the rule applied twice"
    assert np.array_equal(bits(s.read_z_f32()), bits(f["z"]))
    s.close()


@pytest.mark.gpu
def test_a_kept_frame_chosen_by_select_frame(small_synthetic):
    W, Hh, n = 200, 40, 5
    kw = dict(radius=1, depth_step=OC.DEPTH_STEP, crease=OC.CREASE_T, ink=OC.INK)
    p = TC._params(n)
    want = kept = None
    for twin in (True, False):
        s = scene(W, Hh, small_synthetic, "phong", OC.table(W, Hh), frames_per_launch=4)
        s.render_frames(p)
        assert s.frames_kept() >= 3
        if twin:
            kept = []
            for back in range(3):
                s.select_frame(back)
                kept.append(snap(s))
            want = host(kept[1], **kw)
            assert not np.array_equal(want, kept[1]["fb"]) and not np.array_equal(want, host(kept[0], **kw))
        else:
            s.select_frame(1)
            assert np.array_equal(s.get_outlined(params(**kw)), want)
            s.outline(params(**kw))
            assert np.array_equal(s.get_frame_buffer(), want)
            for back in (0, 2):
                s.select_frame(back)
                TC.same(snap(s), kept[back])
            s.select_frame(1)
            assert np.array_equal(s.get_frame_buffer(), want) and np.array_equal(bits(s.read_z_f32()), bits(kept[1]["z"]))
        s.close()


@pytest.mark.gpu
def test_a_composited_frame_carries_ink_on_the_step_between_the_models(small_synthetic):
    import tiny_renderer_amd as T
    W, Hh = 256, 48
    kw = dict(radius=1, depth_step=OC.DEPTH_STEP, ink=OC.INK)
    other = T.synthetic_scene(n_lat=9, n_lon=17, tex_size=128, radius=0.75)
    mk_a = lambda: scene(W, Hh, small_synthetic, "phong", TC.DST_AT)
    mk_b = lambda: scene(W, Hh, other, "phong", TC.SRC_AT)
    a, b = mk_a(), mk_b()
    drive(a), drive(b, light=0.2)
    fa, fb_ = snap(a), snap(b)
    merged, wins = TC.merge(fa, fb_)
    assert wins.any() and not wins.all()
    # the step between the models: a STEP pixel of one model with a drawn 4-neighbour that belongs to the other
    k = T.outline_kinds(merged["z"], params(**kw))
    drawn = bits(merged["z"]) != F32_MIN_BITS
    step = (k & OC.STEP) != 0
    other_side = np.zeros_like(step)
    for axis, sh in ((0, 1), (0, -1), (1, 1), (1, -1)):
        nb_wins, nb_drawn = np.roll(wins, sh, axis), np.roll(drawn, sh, axis)
        other_side |= nb_drawn & (nb_wins != wins)
    assert (step & other_side).sum() >= 8, "no ink on the step between the two models"
    want = host(merged, **kw)
    drive(a), drive(b, light=0.2)
    a.composite(b)
    a.outline(params(**kw))
    got = snap(a)
    assert np.array_equal(got["fb"], want), "%d bytes differ" % int((got["fb"] != want).sum())
    assert np.array_equal(bits(got["z"]), bits(merged["z"]))
    a.close(), b.close()


@pytest.mark.gpu
def test_a_cleared_scene_in_all_four_forms(small_synthetic):
    W, Hh = 200, 40
    s = scene(W, Hh, small_synthetic, "phong", OC.table(W, Hh))
    drive(s)
    assert s.sync() == 0
    plain = params(radius=3, depth_step=OC.DEPTH_STEP, ink=OC.INK)
    paper = params(radius=3, depth_step=OC.DEPTH_STEP, ink=OC.INK, only=True, paper=OC.PAPER)
    for p, colour in ((plain, (0, 0, 0)), (paper, OC.PAPER)):
        want = np.broadcast_to(np.array(colour, np.uint8), (Hh, W, 3))
        s.clear()
        dev, pinned = device_buffer(W * Hh * 3), s.pinned_frame()
        pinned[:] = 0xA5
        s.outline(p, out=dev.data_ptr())
        assert s.sync() == 0 and np.array_equal(dev.cpu().numpy().reshape(Hh, W, 3), want)
        s.clear()
        s.outline(p, out=pinned)
        assert s.sync() == 0 and np.array_equal(pinned, want)
        s.clear()
        assert np.array_equal(s.get_outlined(p), want)
        s.clear()
        s.outline(p)                                      # in place: TR_OK and nothing happens
        assert not s.get_frame_buffer().any() and (bits(s.read_z_f32()) == F32_MIN_BITS).all()
    # and the scene renders as ever afterwards
    drive(s)
    f = snap(s)
    assert np.array_equal(s.get_outlined(plain), host(f, radius=3, depth_step=OC.DEPTH_STEP, ink=OC.INK))
    s.close()


@pytest.mark.gpu
def test_refusals_leave_the_scene_alone(small_synthetic):
    import tiny_renderer_amd as T
    from tiny_renderer_amd import _lib
    L = T.load_library()
    W, Hh = 256, 48
    s = scene(W, Hh, small_synthetic, "phong", OC.table(W, Hh), tap=True)
    band = scene(W, Hh, small_synthetic, "phong", OC.table(W, Hh), band_rows=(16, 32))
    drive(s), drive(band)
    before, flags = snap(s), clean_flags(s)
    before_band, flags_band = snap(band), clean_flags(band)
    p = params(radius=1, depth_step=OC.DEPTH_STEP, ink=OC.INK)
    q = C.addressof(p)
    host_out = np.zeros((Hh, W, 3), np.uint8)
    text = lambda: L.tr_last_error().decode()
    band_text = ": a band scene (tr_options.band_row0/1) cannot be outlined: its border neighbours lie in another rank's rows"
    assert L.tr_scene_outline(band._h, q, None) == _lib.TR_E_INVALID and text() == "tr_scene_outline" + band_text
    assert L.tr_scene_get_outlined(band._h, q, host_out.ctypes.data) == _lib.TR_E_INVALID and text() == "tr_scene_get_outlined" + band_text
    with pytest.raises(T.TinyRendererError):
        band.outline(p)
    assert L.tr_scene_outline(s._h, None, None) == _lib.TR_E_INVALID and text() == "tr_scene_outline: null argument"
    assert L.tr_scene_get_outlined(s._h, q, None) == _lib.TR_E_INVALID and text() == "tr_scene_get_outlined: null argument"
    for field, v, why in (("struct_size", 28, "struct_size is not sizeof(tr_outline_params)"), ("radius", 4, "radius must be 0..TR_OUTLINE_MAX_RADIUS"),
                          ("flags", 4, "unknown flags"), ("opacity", 257, "opacity must be 0..256"),
                          ("depth_step", float("nan"), "depth_step must be finite and >= 0"), ("crease", -1.0, "crease must be finite and >= 0")):
        bad = params(radius=1, depth_step=OC.DEPTH_STEP)
        setattr(bad, field, v)
        assert L.tr_scene_outline(s._h, C.addressof(bad), None) == _lib.TR_E_INVALID and text() == "tr_scene_outline: " + why
        assert L.tr_scene_get_outlined(s._h, C.addressof(bad), host_out.ctypes.data) == _lib.TR_E_INVALID and text() == "tr_scene_get_outlined: " + why
    bad = params()
    bad.ink[3] = 9
    assert L.tr_scene_outline(s._h, C.addressof(bad), None) == _lib.TR_E_INVALID
    assert text() == "tr_scene_outline: the fourth byte of ink and of paper must be 0"
    # `out`: ordinary host memory, a pinned buffer that is too small, the scene's own frame buffer at its start and inside
    assert L.tr_scene_outline(s._h, q, host_out.ctypes.data) == _lib.TR_E_INVALID
    assert text() == "tr_scene_outline: `out` is neither device memory nor from tr_host_alloc (tr_scene_get_outlined takes any host memory)"
    small = L.tr_host_alloc(W * Hh * 3 - 1)
    assert small
    assert L.tr_scene_outline(s._h, q, small) == _lib.TR_E_INVALID and text() == "tr_scene_outline: the host buffer is smaller than the frame"
    L.tr_host_free(small)
    fb_dev = int(s.frame_buffer_device())
    for off in (0, 3 * W, W * Hh * 3 - 1):
        assert L.tr_scene_outline(s._h, q, fb_dev + off) == _lib.TR_E_INVALID
        assert text() == "tr_scene_outline: `out` overlaps a frame buffer of the scene (out == NULL outlines in place)"
    for q_, f_, fl_, rows in ((s, before, flags, None), (band, before_band, flags_band, (16, 32))):
        assert q_.sync() == 0
        assert np.array_equal(clean_flags(q_), fl_)
        TC.same(snap(q_), f_, rows)
    s.close(), band.close()


@pytest.mark.gpu
def test_profile_shows_one_launch_per_call(small_synthetic):
    s = scene(256, 48, small_synthetic, "phong", OC.table(256, 48))
    s.profile_enable(True)
    drive(s)
    s.outline(params(radius=0, depth_step=OC.DEPTH_STEP))
    s.get_outlined(params(radius=3, depth_step=OC.DEPTH_STEP, crease=OC.CREASE_T, only=True))
    assert s.sync() == 0
    prof = s.profile_read()
    assert prof.get("k_outline", {}).get("launches") == 2 and prof["k_outline"]["total_ms"] > 0.0, prof
    s.close()


@pytest.mark.gpu
def test_cli_outline_runs_after_the_grade_and_writes_the_host_rule(african_head, tmp_path):
    import tiny_renderer_amd as T
    from tests import helpers as H
    from tiny_renderer_amd import cli
    common = ["-p", H.asset_dir("african_head"), "-s", "phong", "--width", "256", "--height", "128", "--camera-angle", "0.3",
              "--light-angle", "0.7", "--gamma", "2.2"]
    graded, inked = (str(tmp_path / n) for n in ("graded.ppm", "inked.ppm"))
    assert cli.main(common + ["--out", graded]) == 0
    assert cli.main(common + ["--outline", "1", "--outline-depth", "3", "--outline-crease", "1.5", "--outline-colour", "200,10,10",
                              "--outline-opacity", "200", "--out", inked]) == 0
    hd = b"P6\n256 128\n255\n"
    a, b = (np.frombuffer(open(p, "rb").read()[len(hd):], np.uint8).reshape(128, 256, 3) for p in (graded, inked))
    mesh, texs = african_head
    s = scene(256, 128, (mesh, texs), "phong")
    TC.drive(s)
    z = s.read_z_f32()
    s.close()
    want = T.outline_host(z, a, params(radius=1, depth_step=3.0, crease=1.5, ink=(200, 10, 10), opacity=200))
    assert not np.array_equal(a, b) and np.array_equal(b, want), "the ink goes over the graded picture, untouched by the table"
