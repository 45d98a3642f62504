"""Edge anti-aliasing on the device: tr_scene_antialias / tr_scene_get_antialiased (k_aa) equal tr_aa_host in every byte.

The expectation is the host rule applied to a snapshot of the very frame that is then rendered again and filtered (the
pattern of tests/test_outline.py): reading a scene lowers flags, so the frame that is filtered is a fresh one.
tests/test_aa_host.py pins the host rule and shows on the CPU that the cases here are not vacuous; sizes, placement and
parameter sets are shared through tests/aa_cases.py."""
import ctypes as C

import numpy as np
import pytest

from tests import aa_cases as AC
from tests import outline_cases as OC
from tests import test_composite as TC
from tests import test_outline as TO

bits, scene, snap, clean_flags, tiles_any = TC.bits, TC.scene, TC.snap, TC.clean_flags, TC.tiles_any
device_buffer, state, same_state, box = TO.device_buffer, TO.state, TO.same_state, TO.box


def drive(s, cam=AC.CAM, light=AC.LIGHT, clear=True):
    TC.drive(s, cam, light, clear)


def params(**kw):
    import tiny_renderer_amd as T
    return T.aa_params(**kw)


def host(fb, **kw):
    import tiny_renderer_amd as T
    return T.aa_host(fb, params(**kw))


def four_forms(s, f, before, kws):
    """Every parameter set of kws into device memory, into tr_host_alloc memory, through the getter and in place, each on
    a fresh render of the frame f was taken from.  Returns the number of pixels the host rule changes."""
    import torch
    W, Hh = s.width, s.height
    dev, pinned = device_buffer(W * Hh * 3), s.pinned_frame()
    changed = 0
    for kw in kws:
        want = host(f["fb"], **kw)
        changed += int((want != f["fb"]).any(-1).sum())
        p = params(**kw)
        drive(s)
        dev[:] = 0x5A
        torch.cuda.synchronize()                          # (torch fills on its own stream: not behind the scene's kernel)
        s.antialias(p, out=dev.data_ptr())
        assert s.sync() == 0
        got = dev.cpu().numpy().reshape(Hh, W, 3)
        assert np.array_equal(got, want), "device %r: %d bytes differ" % (kw, int((got != want).sum()))
        pinned[:] = 0xA5
        s.antialias(p, out=pinned)
        assert s.sync() == 0 and np.array_equal(pinned, want), "pinned %r" % (kw,)
        assert np.array_equal(s.get_antialiased(p), want), "getter %r" % (kw,)
        assert np.array_equal(s.get_frame_buffer(), f["fb"]), "out of place wrote the frame"
        drive(s)
        s.antialias(p)
        assert s.sync() == 0
        got = s.get_frame_buffer()
        assert np.array_equal(got, want), "in place %r: %d bytes differ" % (kw, int((got != want).sum()))
        same_state(state(s), before)
    return changed


@pytest.mark.gpu
@pytest.mark.parametrize("store_depth", [False, True], ids=["transient", "stored"])
@pytest.mark.parametrize("pipe", ["phong", "shadow"])
@pytest.mark.parametrize("W,Hh", AC.SIZES)
def test_filtered_frame_equals_the_host_rule_in_all_four_forms(small_synthetic, W, Hh, pipe, store_depth):
    s = scene(W, Hh, small_synthetic, pipe, tap=True, store_depth=store_depth, instance_transforms=AC.table(W, Hh))
    drive(s)
    f, before = snap(s), state(s)
    assert four_forms(s, f, before, AC.gpu_params()) > 0
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("W,Hh", AC.SIZES)
def test_the_ends_of_the_parameter_ranges(small_synthetic, W, Hh):
    """search 1 and 8, subpixel 0 and 256, both thresholds 0 (every pixel that is not flat is filtered) and both at their
    largest."""
    s = scene(W, Hh, small_synthetic, "phong", tap=True, instance_transforms=AC.table(W, Hh))
    drive(s)
    f, before = snap(s), state(s)
    assert four_forms(s, f, before, AC.edge_params()) > 0
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("show_blend", [False, True], ids=["picture", "blend"])
def test_flags_after_an_in_place_call_and_what_their_consumers_read(small_synthetic, show_blend):
    """512 x 64 is 4 x 4 tiles and the model leaves most of them empty; its top row is the last row of its tiles, so the
    black row above, in a flagged tile, takes colour.  A flag that stays up must still mean zeros, so: down exactly
    where a flagged tile received colour, up elsewhere -- and get_frame_buffer, resolve(2) and the sparse read-back
    all return the host rule's frame."""
    W, Hh = 512, 64
    kw = dict(show_blend=show_blend)
    s = scene(W, Hh, small_synthetic, "phong", AC.FLAGS_AT)
    drive(s)
    f, flags = snap(s), clean_flags(s)
    assert np.array_equal(flags, ~tiles_any(bits(f["z"]) != OC.F32_MIN_BITS))
    want = host(f["fb"], **kw)
    assert np.array_equal(want, AC.rule_np(f["fb"], **kw)["out"])
    lit = tiles_any(want.any(-1)[::-1])
    assert (lit & flags).any(), "no flagged tile receives colour: the case shows nothing"
    assert (~lit & flags).any(), "every flagged tile receives colour"
    expect = flags & ~lit
    p = params(**kw)
    drive(s), s.antialias(p)
    assert np.array_equal(clean_flags(s), expect), "flags: down where a flagged tile received colour, up elsewhere"
    assert np.array_equal(s.get_frame_buffer(), want)
    drive(s), s.antialias(p)
    assert np.array_equal(s.resolve(2), box(want, 2)), "a consumer that skips clean tiles lost colour"
    out = s.pinned_frame()
    out[:] = 0x5A
    drive(s), s.antialias(p)
    s.get_frame_buffer_async(out)
    assert s.sync() == 0 and np.array_equal(out, want), "the sparse read-back"
    assert np.array_equal(bits(s.read_z_f32()), bits(f["z"]))
    # out of place over the same flags: every byte, the scene's flags as they were
    drive(s)
    dev = device_buffer(W * Hh * 3)
    s.antialias(p, out=dev.data_ptr())
    assert np.array_equal(clean_flags(s), flags)
    assert np.array_equal(dev.cpu().numpy().reshape(Hh, W, 3), want)
    s.close()


@pytest.mark.gpu
def test_no_depth_pass_is_provoked_and_the_profile_counts_the_launches(small_synthetic):
    """With transient depth the frame's depth stays on the chip: k_tile runs once for the render and not again for the
    filter, and no depth-only pass runs at all."""
    W, Hh = 256, 48
    s = scene(W, Hh, small_synthetic, "phong", instance_transforms=AC.table(W, Hh))
    s.profile_enable(True)
    drive(s)
    assert s.sync() == 0
    tiles = dict(s.profile_read())
    s.antialias(params())
    s.antialias(params(search=4), out=device_buffer(W * Hh * 3).data_ptr())
    s.get_antialiased(params(show_blend=True))
    assert s.sync() == 0
    prof = s.profile_read()
    assert prof.get("k_aa", {}).get("launches") == 3 and prof["k_aa"]["total_ms"] > 0.0, prof
    for k in ("k_tile", "k_tile_depth"):
        assert prof.get(k, {}).get("launches", 0) == tiles.get(k, {}).get("launches", 0), (k, tiles, prof)
    assert prof["k_tile"]["launches"] >= 1
    s.close()


@pytest.mark.gpu
def test_a_cleared_scene_in_all_four_forms(small_synthetic):
    W, Hh = 200, 40
    s = scene(W, Hh, small_synthetic, "phong", instance_transforms=AC.table(W, Hh))
    drive(s)
    assert s.sync() == 0
    p = params()
    want = np.zeros((Hh, W, 3), np.uint8)
    s.profile_enable(True)
    s.clear()
    dev, pinned = device_buffer(W * Hh * 3), s.pinned_frame()
    pinned[:] = 0xA5
    s.antialias(p, out=dev.data_ptr())
    assert s.sync() == 0 and np.array_equal(dev.cpu().numpy().reshape(Hh, W, 3), want)
    s.clear()
    s.antialias(p, out=pinned)
    assert s.sync() == 0 and np.array_equal(pinned, want)
    s.clear()
    assert np.array_equal(s.get_antialiased(p), want)
    s.clear()
    s.antialias(p)                                        # in place: TR_OK and nothing happens
    assert s.sync() == 0 and "k_aa" not in s.profile_read(), "a cleared scene launches nothing"
    assert not s.get_frame_buffer().any() and (bits(s.read_z_f32()) == OC.F32_MIN_BITS).all()
    # and the scene renders as ever afterwards
    drive(s)
    f = snap(s)
    assert np.array_equal(s.get_antialiased(p), host(f["fb"]))
    s.close()


@pytest.mark.gpu
def test_refusals_leave_the_scene_alone(small_synthetic):
    import tiny_renderer_amd as T
    from tiny_renderer_amd import _lib
    L = T.load_library()
    W, Hh = 256, 48
    s = scene(W, Hh, small_synthetic, "phong", tap=True, instance_transforms=AC.table(W, Hh))
    band = scene(W, Hh, small_synthetic, "phong", band_rows=(16, 32), instance_transforms=AC.table(W, Hh))
    drive(s), drive(band)
    before, flags = snap(s), clean_flags(s)
    before_band, flags_band = snap(band), clean_flags(band)
    p = params()
    q = C.addressof(p)
    host_out = np.zeros((Hh, W, 3), np.uint8)
    text = lambda: L.tr_last_error().decode()
    band_text = ": a band scene (tr_options.band_row0/1) cannot be anti-aliased: its border taps lie in another rank's rows"
    assert L.tr_scene_antialias(band._h, q, None) == _lib.TR_E_INVALID and text() == "tr_scene_antialias" + band_text
    assert L.tr_scene_get_antialiased(band._h, q, host_out.ctypes.data) == _lib.TR_E_INVALID and text() == "tr_scene_get_antialiased" + band_text
    with pytest.raises(T.TinyRendererError):
        band.antialias(p)
    assert L.tr_scene_antialias(s._h, None, None) == _lib.TR_E_INVALID and text() == "tr_scene_antialias: null argument"
    assert L.tr_scene_get_antialiased(s._h, q, None) == _lib.TR_E_INVALID and text() == "tr_scene_get_antialiased: null argument"
    for field, v, why in (("struct_size", 20, "struct_size is not sizeof(tr_aa_params)"), ("contrast_min", 256, "contrast_min must be 0..255"),
                          ("contrast_rel", 257, "contrast_rel must be 0..256"), ("search", 0, "search must be 1..TR_AA_MAX_SEARCH"),
                          ("search", 9, "search must be 1..TR_AA_MAX_SEARCH"), ("subpixel", 257, "subpixel must be 0..256"),
                          ("flags", 2, "unknown flags")):
        bad = params()
        setattr(bad, field, v)
        assert L.tr_scene_antialias(s._h, C.addressof(bad), None) == _lib.TR_E_INVALID and text() == "tr_scene_antialias: " + why
        assert L.tr_scene_get_antialiased(s._h, C.addressof(bad), host_out.ctypes.data) == _lib.TR_E_INVALID and text() == "tr_scene_get_antialiased: " + why
    # `out`: ordinary host memory, a pinned buffer that is too small, the scene's own frame buffer at its start and inside
    assert L.tr_scene_antialias(s._h, q, host_out.ctypes.data) == _lib.TR_E_INVALID
    assert text() == "tr_scene_antialias: `out` is neither device memory nor from tr_host_alloc (tr_scene_get_antialiased takes any host memory)"
    small = L.tr_host_alloc(W * Hh * 3 - 1)
    assert small
    assert L.tr_scene_antialias(s._h, q, small) == _lib.TR_E_INVALID and text() == "tr_scene_antialias: the host buffer is smaller than the frame"
    L.tr_host_free(small)
    fb_dev = int(s.frame_buffer_device())
    for off in (0, 3 * W, W * Hh * 3 - 1):
        assert L.tr_scene_antialias(s._h, q, fb_dev + off) == _lib.TR_E_INVALID
        assert text() == "tr_scene_antialias: `out` overlaps a frame buffer of the scene (out == NULL filters in place)"
    for q_, f_, fl_, rows in ((s, before, flags, None), (band, before_band, flags_band, (16, 32))):
        assert q_.sync() == 0
        assert np.array_equal(clean_flags(q_), fl_)
        TC.same(snap(q_), f_, rows)
    s.close(), band.close()


@pytest.mark.gpu
def test_composed_with_the_chain(small_synthetic):
    """Outline in place then antialias in place is aa_host(outline_host(...)); antialias then resolve(2) is the box filter
    of the host's frame; calling it twice filters twice."""
    import tiny_renderer_amd as T
    W, Hh = 256, 48
    s = scene(W, Hh, small_synthetic, "phong", instance_transforms=AC.table(W, Hh))
    drive(s)
    f = snap(s)
    ink = dict(radius=1, depth_step=OC.DEPTH_STEP, ink=OC.INK)
    inked = T.outline_host(f["z"], f["fb"], T.outline_params(**ink))
    once = host(f["fb"])
    twice = host(once)
    smooth_ink = host(inked)
    assert not np.array_equal(inked, f["fb"]) and not np.array_equal(smooth_ink, inked) and not np.array_equal(smooth_ink, once)
    assert not np.array_equal(once, f["fb"]) and not np.array_equal(twice, once)
    drive(s)
    s.outline(T.outline_params(**ink)), s.antialias(params())
    assert np.array_equal(s.get_frame_buffer(), smooth_ink), "the ink's edges are smoothed too"
    assert np.array_equal(bits(s.read_z_f32()), bits(f["z"]))
    drive(s)
    s.antialias(params())
    assert np.array_equal(s.resolve(2), box(once, 2))
    drive(s)
    s.antialias(params()), s.antialias(params())
    assert np.array_equal(s.get_frame_buffer(), twice), "filtering twice is the rule applied twice"
    s.close()


@pytest.mark.gpu
def test_cli_aa_runs_after_the_outline_and_writes_the_host_rule(african_head, tmp_path):
    import tiny_renderer_amd as T
    from tests import helpers as H
    from tiny_renderer_amd import cli
    common = ["-p", H.asset_dir("african_head"), "-s", "phong", "--width", "256", "--height", "128", "--camera-angle", "0.3",
              "--light-angle", "0.7", "--outline", "1", "--outline-depth", "3", "--outline-colour", "200,10,10"]
    inked, smooth, blend = (str(tmp_path / n) for n in ("inked.ppm", "smooth.ppm", "blend.ppm"))
    assert cli.main(common + ["--out", inked]) == 0
    assert cli.main(common + ["--aa", "--aa-contrast", "12,48", "--aa-search", "6", "--aa-subpixel", "128", "--out", smooth]) == 0
    assert cli.main(common + ["--aa", "--aa-show-blend", "--out", blend]) == 0
    hd = b"P6\n256 128\n255\n"
    a, b, c = (np.frombuffer(open(p, "rb").read()[len(hd):], np.uint8).reshape(128, 256, 3) for p in (inked, smooth, blend))
    want = T.aa_host(a, params(contrast_min=12, contrast_rel=48, search=6, subpixel=128))
    assert not np.array_equal(a, b) and np.array_equal(b, want), "the filter goes over the inked picture"
    assert np.array_equal(c, T.aa_host(a, params(show_blend=True)))
