"""Bilateral on the device: tr_scene_bilateral / tr_scene_get_bilateral (k_bilateral) equal tr_bilateral_host in every byte.

Every comparison is np.array_equal against bilateral_host of the frame and the depth the scene itself returns;
tests/test_bilateral_host.py pins bilateral_host against the rule in numpy.  Windows, tables, guides, edges and frame sizes
are tests/bilateral_cases.py's; the depth_scale of a rendered frame is bilateral_cases.scale_for of its own z."""
import ctypes as C

import numpy as np
import pytest

from tests import bilateral_cases as BC
from tests import dense_cases as DC
from tests import helpers as H
from tests import test_composite as TC
from tests import test_dense_frames as TD
from tests import test_outline as TO
from tests import test_resolve as TR

scene, snap, clean_flags = TC.scene, TC.snap, TC.clean_flags
device_buffer = TO.device_buffer
PIPELINES = TR.PIPELINES
GUARD = 64
ALL = BC.everything()
# both guides, the three store forms come with the frames; the mirror-sensitive window, the largest one, a centre that is no
# tap, one-row and one-column windows, every kind of table
SUBSET = ("3x3_step6_colour", "3x3_step6_depth", "15x15_random_colour", "15x15_all255_depth", "L_gaussian10_colour", "L_step6_depth",
          "5x3_random_random_depth", "5x3_random_zeros_colour", "centre_zero_step0_colour", "gaussian7_gaussian10_depth", "1x15_step6_colour", "15x1_step6_depth")


def drive(s, clear=True):
    TC.drive(s, BC.CAM, BC.LIGHT, clear)


def host(f, case, edge="clamp", border=(0, 0, 0), scale=None):
    """bilateral_host of the snapshot f = {"fb", "z"}."""
    import tiny_renderer_amd as T
    return T.bilateral_host(f["fb"], BC.params(case, edge, border, scale), f["z"])


def same(got, want, what):
    assert got.shape == want.shape and np.array_equal(got, want), "%s: %d bytes differ" % (what, int((got != want).sum()))


@pytest.mark.gpu
@pytest.mark.parametrize("W,Hh", BC.FRAMES, ids=["%dx%d" % s for s in BC.FRAMES])
def test_filtered_frame_equals_the_host_rule(small_synthetic, W, Hh):
    s = scene(W, Hh, small_synthetic, "phong")
    drive(s)
    f = snap(s)
    assert f["fb"].any()
    scale = BC.scale_for(f["z"])
    if (W, Hh) == (640, 480):
        flags = clean_flags(s)
        assert flags.any() and not flags.all(), "640 x 480 holds flagged and unflagged tiles"
        d = BC.depth_distance(f["z"][:, 1:], f["z"][:, :-1], scale)
        assert ((d > 0) & (d < 255)).any() and (d == 255).any() and (d == 0).any(), "the depth distances do not spread over the table"
    for name in SUBSET:
        for edge, border in BC.EDGES:
            same(s.get_bilateral(BC.params(ALL[name], edge, border, scale)), host(f, ALL[name], edge, border, scale), "%s %s %r" % (name, edge, border))
    same(s.get_bilateral(BC.params(ALL["1x1_step6_depth"], depth_scale=scale)), f["fb"], "one centre tap is a copy")
    same(s.get_frame_buffer(), f["fb"], "the getter leaves the frame")
    assert np.array_equal(TC.bits(s.read_z_f32()), TC.bits(f["z"])), "z changed"
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("W", [640, 636], ids=["wide", "narrow"])
def test_device_pinned_and_getter_targets_between_guards(small_synthetic, W):
    """A device pointer at offset 0 and 1, a tensor, a tr_host_alloc block and the getter, each pre-filled with 0xAA between
    guard bytes: every byte inside is written, none outside; a pointer off by one byte gives the same image."""
    import torch
    import tiny_renderer_amd as T
    Hh = 480
    s = scene(W, Hh, small_synthetic, "specular")
    drive(s)
    f = snap(s)
    scale = BC.scale_for(f["z"])
    L = T.load_library()
    for name in ("L_gaussian10_colour", "15x15_all255_depth"):
        p = BC.params(ALL[name], "border", BC.PAPER, scale)
        want = host(f, ALL[name], "border", BC.PAPER, scale)
        assert not (want == 0xAA).all()
        n = want.size
        dev = torch.full((n + 2 * GUARD,), 0xAA, dtype=torch.uint8, device="cuda")
        for off in (0, 1):
            dev[:] = 0xAA
            torch.cuda.synchronize()
            s.bilateral(p, dev.data_ptr() + GUARD + off)
            assert s.sync() == 0
            raw = dev.cpu().numpy()
            same(raw[GUARD + off:GUARD + off + n].reshape(want.shape), want, "%s device + %d" % (name, off))
            assert (raw[:GUARD + off] == 0xAA).all() and (raw[GUARD + off + n:] == 0xAA).all(), "a guard byte changed"
            dev[:] = 0xAA
            torch.cuda.synchronize()
            view = dev[GUARD + off:GUARD + off + n]
            assert s.bilateral(p, view) is view and s.sync() == 0
            raw = dev.cpu().numpy()
            same(raw[GUARD + off:GUARD + off + n].reshape(want.shape), want, "%s tensor + %d" % (name, off))
            assert (raw[:GUARD + off] == 0xAA).all() and (raw[GUARD + off + n:] == 0xAA).all(), "a guard byte changed"
        block = L.tr_host_alloc(n + 2 * GUARD)
        assert block
        pinned = np.ctypeslib.as_array((C.c_uint8 * (n + 2 * GUARD)).from_address(block))
        pinned[:] = 0xAA
        assert L.tr_scene_bilateral(s._h, C.addressof(p), block) == 0 and s.sync() == 0
        same(pinned[:n].reshape(want.shape), want, name + " tr_host_alloc block")
        assert (pinned[n:] == 0xAA).all(), "bytes behind the picture changed"
        assert L.tr_scene_bilateral(s._h, C.addressof(p), block + 1) != 0, "an address inside a tr_host_alloc block is no `out`"
        L.tr_host_free(block)
        mine = s.pinned_frame()
        mine[...] = 0xAA
        assert s.bilateral(p, mine) is mine and s.sync() == 0
        same(mine, want, name + " pinned_frame")
        guarded = np.full(n + 2 * GUARD, 0xAA, np.uint8)
        assert L.tr_scene_get_bilateral(s._h, C.addressof(p), guarded[GUARD:].ctypes.data) == 0
        same(guarded[GUARD:GUARD + n].reshape(want.shape), want, name + " getter")
        assert (guarded[:GUARD] == 0xAA).all() and (guarded[GUARD + n:] == 0xAA).all()
    same(s.get_frame_buffer(), f["fb"], "out of place leaves the frame")
    s.close()


DENSE = [(W, Hh, kind) for W, Hh in DC.SIZES_HALO for kind in DC.BACKDROPS]


@pytest.mark.gpu
@pytest.mark.parametrize("W,Hh,kind", DENSE, ids=["%dx%d-%s" % r for r in DENSE])
def test_dense_frames_in_a_callers_buffer(small_synthetic, W, Hh, kind):
    """Rendered frames are smooth and mostly black: noise, white and the planted picture in a caller's guarded buffer, drawn
    into without a clear.  On noise the plain mean differs from its input, and a step of 6 keeps few taps."""
    s, buf, f = TD.dense_scene(small_synthetic, W, Hh, kind)
    scale = BC.scale_for(f["z"])
    for name in SUBSET:
        for edge, border in BC.EDGES:
            want = host(f, ALL[name], edge, border, scale)
            if kind == "noise" and name in ("15x15_random_colour", "15x15_all255_depth", "L_gaussian10_colour"):
                assert not np.array_equal(want, f["fb"]), name + ": the filtered noise is the noise"
            same(s.get_bilateral(BC.params(ALL[name], edge, border, scale)), want, "%s %s %r" % (name, edge, border))
    TD.in_buffer(buf, f["fb"])
    s.close()


@pytest.mark.gpu
def test_stale_memory_behind_raised_flags_and_the_cleared_scene(small_synthetic):
    """A frame that covers the screen, then a clear and the small model: tiles lit in the first frame and flagged clean in the
    second hold the first frame's COLOUR in memory and must read as zeros.  (Reading z to build the expectation writes
    f32::MIN behind the depth flags, so stale DEPTH is the next test's, with a twin scene.)  Then the cleared scene's
    short-circuits on the k_bilateral launch count."""
    import tiny_renderer_amd as T
    mesh, texs = small_synthetic
    W, Hh = 640, 480
    s = T.Scene(W, Hh, mesh, texs, "phong")
    s.set_instances(np.array([[0.0, 0.0, 0.0, 3.0]], np.float32))
    TR.frame(s, 0.0, 0.0)
    one = s.get_frame_buffer()
    flags_one, t = TR.clean_flags(s)
    lit_one = TR.lit_tiles(one, t)
    assert lit_one.mean() > 0.9
    s.set_instances(None)
    TR.frame(s)
    f = {"fb": s.get_frame_buffer(), "z": s.read_z_f32()}
    flags_two, _ = TR.clean_flags(s)
    assert (lit_one & ~flags_one & flags_two).any(), "no tile lit in frame one is flagged clean in frame two"
    scale = BC.scale_for(f["z"])
    # an all-255 or random table lets an undrawn neighbour's colour in: stale colour would show
    for name in SUBSET:
        for edge, border in BC.EDGES:
            same(s.get_bilateral(BC.params(ALL[name], edge, border, scale)), host(f, ALL[name], edge, border, scale), "%s %s %r" % (name, edge, border))
    wide, small = ALL["15x15_all255_depth"], ALL["3x3_all255_colour"]   # (tables that let a border colour in)
    s.profile_enable(True)
    s.clear()
    dev = device_buffer(W * Hh * 3)
    s.bilateral(BC.params(wide, "clamp", BC.PAPER), dev.data_ptr())
    assert s.sync() == 0 and not dev.cpu().numpy().any(), "a cleared scene smooths to zeros"
    s.clear()
    assert not s.get_bilateral(BC.params(wide, "border")).any() and not s.get_bilateral(BC.params(small, "clamp")).any()
    assert s.bilateral(BC.params(small)) is None and s.sync() == 0
    assert "k_bilateral" not in s.profile_read(), "a cleared scene launches nothing where no border colour comes in"
    black = {"fb": np.zeros((Hh, W, 3), np.uint8), "z": np.full((Hh, W), BC.F32_MIN, np.float32)}
    for k, case in enumerate((small, wide)):
        s.clear()
        want = host(black, case, "border", BC.PAPER)
        assert want.any() and not want.all()
        same(s.get_bilateral(BC.params(case, "border", BC.PAPER)), want, "a cleared scene under another border")
        assert s.profile_read()["k_bilateral"]["launches"] == 2 * k + 1
        assert not s.get_frame_buffer().any()
        s.clear()
        s.bilateral(BC.params(case, "border", BC.PAPER))
        same(s.get_frame_buffer(), want, "a cleared scene in place under another border")
        flags = clean_flags(s)
        assert flags.any() and not (flags & TR.lit_tiles(want, s.band_tiles())).any(), "the frame of paper is flagged clean, or no inner tile is"
        assert s.profile_read()["k_bilateral"]["launches"] == 2 * k + 2
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("x,y", [(-0.5, 0.0), (0.5, 0.3), (0.0, -0.45)])
def test_stale_depth_behind_raised_depth_flags_reads_as_not_drawn(small_synthetic, x, y):
    """tests/test_ambient_occlusion.py's form.  512 x 64 is 4 x 4 tiles.  A large frame is rendered and its depth fetched into
    the slot's memory by one read of the LARGE frame; then a small model is rendered and smoothed under the DEPTH guide with
    NO z read in between: the tiles it leaves empty still hold the large frame's z behind raised depth flags when
    k_bilateral runs.  Reading z would write f32::MIN there, so the expectation comes from a twin scene.  A kernel that
    loaded that memory for its halo would give the host rule over the mixed field -- which must differ from the wanted
    picture: an undrawn centre in a drawn tile is 0 from an undrawn tap and 255 from a stale one, and the random table
    weighs the two differently."""
    import torch
    W, Hh = 512, 64
    big_at = np.array([[0.0, 0.0, 0.3, 1.0]], np.float32)
    twin = scene(W, Hh, small_synthetic, "phong", big_at)
    drive(twin)
    big = snap(twin)
    twin.set_instances(TC._small(x, y))
    drive(twin)
    small = snap(twin)
    twin.close()
    drawn = BC.bits(small["z"]) != BC.F32_MIN_BITS
    flagged = np.repeat(np.repeat(~TC.tiles_any(drawn), 16, 0), 128, 1)
    assert drawn.any() and flagged.any()
    stale = {"fb": small["fb"], "z": np.where(flagged, big["z"], small["z"])}
    assert (BC.bits(stale["z"]) != BC.bits(small["z"])).any()
    scale = BC.scale_for(small["z"])
    case = ALL["15x15_random_depth"]
    want = {e: host(small, case, e[0], e[1], scale) for e in BC.EDGES}
    for e in BC.EDGES:
        assert not np.array_equal(host(stale, case, e[0], e[1], scale), want[e]), "stale z would not show"
    s = scene(W, Hh, small_synthetic, "phong", big_at)
    drive(s)
    assert np.array_equal(BC.bits(s.read_z_f32()), BC.bits(big["z"]))   # the LARGE frame's depth, fetched into the slot's memory
    assert s.sync() == 0
    s.set_instances(TC._small(x, y))
    drive(s)
    # (nothing reads the small frame's z from here on: its empty tiles are stale behind their flags)
    for e in BC.EDGES:
        same(s.get_bilateral(BC.params(case, e[0], e[1], scale)), want[e], "the getter %s %r" % e)
    dev = torch.full((W * Hh * 3,), 0xAA, dtype=torch.uint8, device="cuda")
    s.bilateral(BC.params(case, "border", BC.PAPER, scale), dev)
    assert s.sync() == 0
    same(dev.cpu().numpy().reshape(Hh, W, 3), want[("border", BC.PAPER)], "out of place")
    s.bilateral(BC.params(case, "clamp", depth_scale=scale))
    same(s.get_frame_buffer(), want[("clamp", (0, 0, 0))], "in place")
    assert np.array_equal(BC.bits(s.read_z_f32()), BC.bits(small["z"]))
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("W,Hh", [(640, 480), (134, 21)], ids=["whole_tile_rows", "partial_tile_row"])
def test_in_place_the_frame_and_its_flags_follow(small_synthetic, W, Hh):
    """The frame afterwards is the out-of-place result; resize, resolve and the sparse read-back see it; z stays; a second
    call filters the filtered frame; a later clear and render is the caller's."""
    import tiny_renderer_amd as T
    s = scene(W, Hh, small_synthetic, "phong")
    drive(s)
    before = snap(s)
    scale = BC.scale_for(before["z"])
    for name, edge, border in (("15x15_random_colour", "border", (0, 0, 0)), ("L_step6_depth", "border", BC.PAPER), ("gaussian7_gaussian10_depth", "clamp", (0, 0, 0)),
                               ("3x3_step6_colour", "clamp", (0, 0, 0))):
        case = ALL[name]
        want = host(before, case, edge, border, scale)
        assert not np.array_equal(want, before["fb"])
        drive(s)
        assert s.bilateral(BC.params(case, edge, border, scale)) is None
        flags = clean_flags(s)
        lit = TR.lit_tiles(want, s.band_tiles())
        assert not (flags & lit).any(), "a tile that holds colour is flagged clean"
        if (W, Hh) == (640, 480) and border == (0, 0, 0):
            assert flags.any(), "no tile is flagged clean"
        same(s.get_frame_buffer(), want, name + ": the frame afterwards")
        pinned = s.pinned_frame()
        pinned[...] = 0xAA
        s.get_frame_buffer_async(pinned)
        assert s.sync() == 0
        same(pinned, want, name + ": the sparse read-back")
        same(s.resize(W // 2 + 1, Hh // 2 + 1), T.resize_host(want, W // 2 + 1, Hh // 2 + 1), name + ": resize afterwards")
        if W % 2 == 0 and Hh % 2 == 0:
            same(s.resolve(2), TR.box(want, 2), name + ": resolve afterwards")
        assert np.array_equal(TC.bits(s.read_z_f32()), TC.bits(before["z"])), "z changed"
        s.bilateral(BC.params(case, edge, border, scale))
        same(s.get_frame_buffer(), host({"fb": want, "z": before["z"]}, case, edge, border, scale), name + ": twice")
    drive(s)
    TC.same(snap(s), before)
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("guide", ["colour", "depth"])
def test_a_call_between_two_renders_is_ordered_on_the_stream(small_synthetic, guide):
    import torch
    W, Hh = 300, 200
    s = scene(W, Hh, small_synthetic, "phong", frames_per_launch=4)
    drive(s)
    f = snap(s)
    scale = BC.scale_for(f["z"])
    case = ALL["15x15_random_colour" if guide == "colour" else "L_step6_depth"]
    a = torch.full((W * Hh * 3,), 0xAA, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    TR.frame(s, BC.CAM, BC.LIGHT)
    s.bilateral(BC.params(case, "clamp", depth_scale=scale), a)
    TR.frame(s, 1.1, 0.2)
    assert s.sync() == 0
    two = s.get_frame_buffer()
    assert not np.array_equal(two, f["fb"])
    same(a.cpu().numpy().reshape(Hh, W, 3), host(f, case, "clamp", scale=scale), "the first frame, filtered before the second was rendered")
    s.close()


@pytest.mark.gpu
def test_only_the_depth_guide_provokes_a_depth_pass_and_the_profile_counts_the_launches(small_synthetic):
    """The colour half is tests/test_rank.py's test_no_depth_pass_is_provoked_and_the_profile_counts_the_launches, the same
    scene, size and order of calls (a getter, an out-of-place call, an in-place call): the k_tile / k_tile_depth launch
    counts afterwards equal those before, as there.  The depth half is tests/test_layer.py's WHERE-flag form: one pass
    more, once."""
    W, Hh = 256, 48
    s = scene(W, Hh, small_synthetic, "phong")
    s.profile_enable(True)
    drive(s)
    assert s.sync() == 0
    tiles = dict(s.profile_read())
    passes = lambda prof: {k: prof.get(k, {}).get("launches", 0) for k in ("k_tile", "k_tile_depth")}
    p = BC.params(ALL["L_gaussian10_colour"])
    s.get_bilateral(p)
    s.bilateral(BC.params(ALL["3x3_step6_colour"], "border", BC.PAPER), device_buffer(W * Hh * 3).data_ptr())
    s.bilateral(p)
    assert s.sync() == 0
    prof = s.profile_read()
    assert prof.get("k_bilateral", {}).get("launches") == 3 and prof["k_bilateral"]["total_ms"] > 0.0, prof
    assert passes(prof) == passes(tiles), "the colour guide provoked a pass"
    assert prof["k_tile"]["launches"] >= 1
    # the depth guide makes the depth real, once
    d = BC.params(ALL["L_step6_depth"], depth_scale=3.0)
    s.get_bilateral(d)
    once = passes(s.profile_read())
    assert sum(once.values()) == sum(passes(tiles).values()) + 1, (tiles, once)
    s.bilateral(d, device_buffer(W * Hh * 3).data_ptr())
    s.bilateral(d)
    assert s.sync() == 0
    prof = s.profile_read()
    assert passes(prof) == once and prof["k_bilateral"]["launches"] == 6, prof
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("pipe", PIPELINES)
def test_every_pipeline(small_synthetic, pipe):
    W, Hh = 640, 480
    s = scene(W, Hh, small_synthetic, pipe)
    drive(s)
    f = snap(s)
    scale = BC.scale_for(f["z"])
    drive(s)
    for name in ("L_step6_depth", "gaussian7_gaussian10_depth", "5x3_random_random_depth", "L_gaussian10_colour"):
        same(s.get_bilateral(BC.params(ALL[name], "border", BC.PAPER, scale)), host(f, ALL[name], "border", BC.PAPER, scale), pipe + " " + name)
    s.close()


@pytest.mark.gpu
def test_refusals_leave_the_scene_alone(small_synthetic):
    import tiny_renderer_amd as T
    from tiny_renderer_amd import _lib
    L = T.load_library()
    W, Hh = 256, 48
    s = scene(W, Hh, small_synthetic, "phong", tap=True)
    band = scene(W, Hh, small_synthetic, "phong", band_rows=(16, 32))
    drive(s), drive(band)
    before, flags = snap(s), clean_flags(s)
    before_band, flags_band = snap(band), clean_flags(band)
    s.profile_enable(True), band.profile_enable(True)
    p = BC.params(ALL["3x3_step6_depth"])
    q = C.addressof(p)
    host_out = np.full((Hh, W, 3), 0xAA, np.uint8)
    dev = device_buffer(W * Hh * 3)
    text = lambda: L.tr_last_error().decode()
    calls = (("tr_scene_bilateral", lambda sc, pp: L.tr_scene_bilateral(sc._h, pp, dev.data_ptr())),
             ("tr_scene_get_bilateral", lambda sc, pp: L.tr_scene_get_bilateral(sc._h, pp, host_out.ctypes.data)))

    def wrong(**kw):
        w = BC.params(ALL["3x3_step6_depth"])
        for k, v in kw.items():
            if k.startswith("spatial"):
                w.spatial[int(k[7:])] = v
            elif k.startswith("pad2_"):
                w.pad2[int(k[5:])] = v
            else:
                setattr(w, k, v)
        return w

    for who, call in calls:
        assert call(s, None) == _lib.TR_E_INVALID and text() == who + ": null argument"
        for kw, why in ((dict(struct_size=508), ": struct_size is not sizeof(tr_bilateral_params)"), (dict(kw=2), ": kw and kh must be odd and 1..15"),
                        (dict(kh=17), ": kw and kh must be odd and 1..15"), (dict(spatial9=1), ": spatial weights outside the kw x kh window"),
                        (dict(spatial224=1), ": spatial weights outside the kw x kh window"), ({"spatial%d" % k: 0 for k in range(9)}, ": the window is all zeros"),
                        (dict(guide=2), ": guide must be TR_BILATERAL_GUIDE_COLOUR or TR_BILATERAL_GUIDE_DEPTH"),
                        (dict(edge=2), ": edge must be TR_BILATERAL_BORDER or TR_BILATERAL_CLAMP"), (dict(depth_scale=-1.0), ": depth_scale must be finite and >= 0"),
                        (dict(depth_scale=float("inf")), ": depth_scale must be finite and >= 0"), (dict(depth_scale=float("nan"), guide=0), ": depth_scale must be finite and >= 0"),
                        (dict(pad=1), ": pad and pad2 must be 0"), (dict(pad2_2=1), ": pad and pad2 must be 0")):
            assert call(s, C.addressof(wrong(**kw))) == _lib.TR_E_INVALID and text() == who + why
        # which refusal wins: the parameters before the band, the band before the target
        assert call(band, C.addressof(wrong(edge=2))) == _lib.TR_E_INVALID and text() == who + ": edge must be TR_BILATERAL_BORDER or TR_BILATERAL_CLAMP"
        assert call(band, q) == _lib.TR_E_INVALID
        assert text() == who + ": a band scene (tr_options.band_row0/1) cannot be smoothed: its border taps lie in another rank's rows"
    assert L.tr_scene_bilateral(None, q, dev.data_ptr()) == _lib.TR_E_INVALID and text() == "tr_scene_bilateral: null scene"
    assert L.tr_scene_get_bilateral(None, q, host_out.ctypes.data) == _lib.TR_E_INVALID and text() == "tr_scene_get_bilateral: null scene"
    assert L.tr_scene_get_bilateral(s._h, q, None) == _lib.TR_E_INVALID and text() == "tr_scene_get_bilateral: null argument"
    assert L.tr_scene_bilateral(band._h, q, host_out.ctypes.data) == _lib.TR_E_INVALID and text().startswith("tr_scene_bilateral: a band scene")
    with pytest.raises(T.TinyRendererError):
        band.get_bilateral(p)
    assert L.tr_scene_bilateral(s._h, q, host_out.ctypes.data) == _lib.TR_E_INVALID
    assert text() == "tr_scene_bilateral: `out` is neither device memory nor from tr_host_alloc (tr_scene_get_bilateral takes any host memory)"
    small = L.tr_host_alloc(W * Hh * 3 - 1)
    assert small
    assert L.tr_scene_bilateral(s._h, q, small) == _lib.TR_E_INVALID and text() == "tr_scene_bilateral: the host buffer is smaller than the frame"
    L.tr_host_free(small)
    t = s.band_tiles()
    assert L.tr_scene_bilateral(s._h, q, int(t.frame_buffer_device) + 3) == _lib.TR_E_INVALID
    assert text() == "tr_scene_bilateral: `out` overlaps a frame buffer of the scene (out == NULL smooths in place)"
    assert (host_out == 0xAA).all() and (dev.cpu().numpy() == 0x5A).all(), "a refused call wrote `out`"
    for q_, f_, fl_, rows in ((s, before, flags, None), (band, before_band, flags_band, (16, 32))):
        assert q_.sync() == 0
        assert "k_bilateral" not in q_.profile_read(), "a refused call queued a kernel"
        assert np.array_equal(clean_flags(q_), fl_)
        TC.same(snap(q_), f_, rows)
    s.close(), band.close()


@pytest.mark.gpu
def test_cli_options_write_the_filtered_picture(african_head, tmp_path):
    import tiny_renderer_amd as T
    from tiny_renderer_amd import cli
    W, Hh = 256, 128
    common = ["-p", H.asset_dir("african_head"), "-s", "phong", "--width", str(W), "--height", str(Hh), "--camera-angle", "0.3", "--light-angle", "0.7"]
    names = ("full", "smooth", "ranged", "deep", "chain", "ao", "aosmooth")
    full, smooth, ranged, deep, chain, ao, aosmooth = (str(tmp_path / (n + ".ppm")) for n in names)
    assert cli.main(common + ["--out", full]) == 0
    assert cli.main(common + ["--smooth", "2", "--out", smooth]) == 0
    assert cli.main(common + ["--smooth", "7", "--smooth-range", "40", "--out", ranged]) == 0
    assert cli.main(common + ["--smooth", "3", "--smooth-guide", "depth", "--smooth-depth-scale", "20", "--smooth-range", "5", "--out", deep]) == 0
    assert cli.main(common + ["--median", "1", "--smooth", "1", "--out", chain]) == 0
    assert cli.main(common + ["--ao", "8", "--out", ao]) == 0
    assert cli.main(common + ["--ao", "8", "--ao-smooth", "2", "--smooth-depth-scale", "4", "--out", aosmooth]) == 0
    hd = ("P6\n%d %d\n255\n" % (W, Hh)).encode()
    a, b, c, d, e, g, h = (np.frombuffer(open(p, "rb").read()[len(hd):], np.uint8).reshape(Hh, W, 3) for p in (full, smooth, ranged, deep, chain, ao, aosmooth))
    mesh, texs = african_head
    s = scene(W, Hh, (mesh, texs), "phong")
    TC.drive(s)
    f = snap(s)
    s.close()
    assert a.any() and np.array_equal(f["fb"], a)
    box = lambda r: T.spatial_box(2 * r + 1, 2 * r + 1)
    same(b, T.bilateral_host(a, T.bilateral_params(box(2), T.range_step(16))), "--smooth")
    same(c, T.bilateral_host(a, T.bilateral_params(box(7), T.range_step(40))), "--smooth-range")
    same(d, T.bilateral_host(a, T.bilateral_params(box(3), T.range_step(5), guide="depth", depth_scale=20.0), f["z"]), "--smooth-guide depth")
    median = T.rank_host(a, T.rank_params(T.footprint_rect(3, 3), "median", edge="clamp"))
    same(e, T.bilateral_host(median, T.bilateral_params(box(1), T.range_step(16))), "--median before --smooth")
    same(g, T.ambient_occlusion_host(f["z"], a, radius=8), "--ao")
    same(h, T.bilateral_host(g, T.bilateral_params(box(2), T.range_step(16), guide="depth", depth_scale=4.0), f["z"]), "--ao-smooth directly behind --ao")
    assert not np.array_equal(b, a) and not np.array_equal(d, a) and not np.array_equal(h, g)
    for bad in (["--smooth", "2", "--view", "z"], ["--smooth", "0"], ["--smooth", "8"], ["--smooth", "x"], ["--smooth", "1", "--smooth", "2"],
                ["--smooth-range", "3"], ["--smooth-guide", "depth"], ["--smooth", "2", "--smooth-range", "256"], ["--smooth", "2", "--seconds", "1"],
                ["--ao-smooth", "2"], ["--ao", "8", "--ao-smooth", "9"], ["--ao", "8", "--ao-smooth", "2", "--smooth-guide", "colour"],
                ["--smooth", "2", "--smooth-depth-scale", "-1"], ["--smooth", "2", "--smooth-guide", "normal"]):
        with pytest.raises(SystemExit):
            cli.main(common + bad)
