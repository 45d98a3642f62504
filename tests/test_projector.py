"""The projector on the device: tr_scene_projector / tr_scene_get_projector (k_projector) equal tr_projector_host in
every byte.

Every comparison is np.array_equal against projector_host of what the scenes themselves return (get_frame_buffer,
read_z_f32 of the frame and of the occluder); tests/test_projector_host.py pins projector_host against the layer rule,
hand-computed values and the rule in numpy."""
import ctypes as C

import numpy as np
import pytest

from tests import projector_cases as PC
from tests import test_composite as TC
from tests import test_outline as TO

scene, snap, clean_flags, tiles_any = TC.scene, TC.snap, TC.clean_flags, TC.tiles_any
device_buffer, state, same_state, box = TO.device_buffer, TO.state, TO.same_state, TO.box
IDS = ["%dx%d" % s for s in PC.GPU_SIZES]
SIDE = 0.9


def drive(s, cam=PC.CAM, light=PC.LIGHT, clear=True):
    TC.drive(s, cam, light, clear)


def same(got, want, what):
    assert got.shape == want.shape and np.array_equal(got, want), "%s: %d bytes differ" % (what, int((got != want).sum()))


def table(W, Hh):
    return TC.DST_AT if W < 128 else PC.table(W, Hh)


def on_device(img, off=0, pad=0):
    """The image as a torch tensor on the device: packed, or `off` bytes into an allocation with rows `pad` bytes apart
    beyond their own (a strided view)."""
    import torch
    ph, pw, ch = img.shape
    if off == 0 and pad == 0:
        return torch.from_numpy(np.ascontiguousarray(img)).cuda()
    stride = pw * ch + pad
    raw = torch.full((off + stride * ph,), 0xEE, dtype=torch.uint8, device="cuda")
    view = raw[off:].as_strided((ph, pw, ch), (stride, ch, 1))
    view.copy_(torch.from_numpy(np.ascontiguousarray(img)).cuda())
    torch.cuda.synchronize()
    assert off == 0 or view.data_ptr() % 2 == 1
    return view


def params(m, img, mode="add", opacity=256, occlude=False, soft=False, depth_bias=0.0):
    import tiny_renderer_amd as T
    return T.projector_params(m, img.shape[1], img.shape[0], img.shape[2], mode, opacity, occlude, soft, depth_bias)


def host(f, p, img, occluder_z=None):
    import tiny_renderer_amd as T
    return T.projector_host(f["fb"], f["z"], p, img, occluder_z)


def launches(prof, name):
    return prof.get(name, {}).get("launches", 0)


def two_cameras(W, Hh, img, behind=False):
    import tiny_renderer_amd as T
    view, proj = PC.cameras(W, Hh, img.shape[1], img.shape[0], side=SIDE, behind=behind)
    return T.projector_matrix(view, proj)


def all_four_forms(s, f, p, img, dev_img, what, occluder=None, occluder_z=None):
    """The getter, device memory, a tr_host_alloc block and in place against the host rule; the frame is rendered again
    afterwards.  Returns the expected frame."""
    W, Hh = s.width, s.height
    want = host(f, p, img, occluder_z)
    flags = clean_flags(s)
    same(s.get_projector(p, dev_img, occluder), want, what + ": getter")
    dev, pinned = device_buffer(W * Hh * 3, 0xAB), s.pinned_frame()
    pinned[...] = 0xAB
    s.projector(p, dev_img, occluder, out=dev.data_ptr())
    s.projector(p, dev_img, occluder, out=pinned)
    assert s.sync() == 0
    same(dev.cpu().numpy().reshape(Hh, W, 3), want, what + ": device memory")
    same(pinned, want, what + ": tr_host_alloc")
    assert np.array_equal(clean_flags(s), flags), "an out-of-place call changed the frame's flags"
    same(s.get_frame_buffer(), f["fb"], what + ": out of place leaves the scene's frame")
    s.projector(p, dev_img, occluder)
    same(s.get_frame_buffer(), want, what + ": in place")
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("W,Hh", PC.GPU_SIZES, ids=IDS)
def test_frame_sizes_matrices_and_all_four_forms(small_synthetic, W, Hh):
    """Every frame size (phong and shadow in turn) under the identity with an image of the frame's size, a whole-pixel
    translation, a projector to the side and one behind the model, through all four entry-point forms."""
    pipe = ("phong", "shadow")[PC.GPU_SIZES.index((W, Hh)) % 2]
    s = scene(W, Hh, small_synthetic, pipe, table(W, Hh), tap=True)
    drive(s)
    f, before = snap(s), state(s)
    drawn = PC.bits(f["z"]) != PC.F32_MIN_BITS
    assert drawn.any(), "nothing is drawn"
    rng = np.random.default_rng(W * Hh)
    full3, full4, small = PC.random_image(rng, W, Hh, 3), PC.random_image(rng, W, Hh, 4), PC.random_image(rng, 64, 64, 4)
    yy, xx = np.mgrid[0:Hh, 0:W]
    m_behind = two_cameras(W, Hh, small, behind=True)
    mb = m_behind.astype(np.float64)
    w = mb[3] * xx + mb[7] * yy + mb[11] * f["z"].astype(np.float64) + mb[15]
    if W >= 128:
        assert (drawn & (w <= 0)).any() and (drawn & (w > 0)).any(), "the projector behind the model: w of both signs on drawn pixels"
    cases = (("identity", PC.identity(), full3, "add", 256), ("translation", PC.translation(3, -2), full4, "normal", 200),
             ("two cameras", two_cameras(W, Hh, small), small, "screen", 256), ("behind", m_behind, small, "normal", 256))
    changed = 0
    for name, m, img, mode, op in cases:
        p = params(m, img, mode, op)
        want = all_four_forms(s, f, p, img, on_device(img), name)
        changed += int(not np.array_equal(want, f["fb"]))
        same_state(state(s), before)
        drive(s)
    assert changed >= (3 if W >= 128 else 1), "the cases changed nothing"      # (below one tile the translated image and the projectors may miss the few drawn pixels)
    if W >= 128:
        import tiny_renderer_amd as T
        same(host(f, params(PC.identity(), full3, "add", 256), full3), T.layer_host(f["fb"], full3, 0, 0, "add", 256, "drawn", z=f["z"]), "the layer identity")
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("W,Hh", [(256, 48), (257, 33)], ids=["words", "bytes"])
def test_image_sizes_channels_odd_addresses_and_padded_strides(small_synthetic, W, Hh):
    s = scene(W, Hh, small_synthetic, "phong", table(W, Hh))
    drive(s)
    f = snap(s)
    rng = np.random.default_rng(W)
    changed = 0
    for k, (pw, ph) in enumerate(PC.IMAGES):
        for ch in (3, 4):
            img = PC.random_image(rng, pw, ph, ch)
            p = params(two_cameras(W, Hh, img), img, PC.MODES[(2 * k + ch) % 7], (256, 231)[ch - 3])
            want = host(f, p, img)
            changed += int(not np.array_equal(want, f["fb"]))
            same(s.get_projector(p, on_device(img)), want, "%d x %d x %d packed" % (pw, ph, ch))
            for off, pad in ((1, 0), (3, 5), (0, 7)):
                same(s.get_projector(p, on_device(img, off, pad)), want, "%d x %d x %d at +%d, rows +%d" % (pw, ph, ch, off, pad))
    assert changed >= 6
    # a page-locked image, in place
    img = PC.random_image(rng, 7, 5, 4)
    pin = s.pinned_layer(7, 5, 4)
    pin[...] = img
    p = params(two_cameras(W, Hh, img), img, "normal", 256)
    s.projector(p, pin)
    same(s.get_frame_buffer(), host(f, p, img), "a tr_host_alloc image, in place")
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("store_depth", [False, True], ids=["transient", "stored"])
def test_a_second_scene_as_occluder_and_which_depths_are_made_real(small_synthetic, store_depth):
    """OCCLUDE and OCCLUDE | SOFT with the projector's own scene as the shadow map.  k_projector has no entry in the profile
    (its table of names is full): its launches are counted by tr_scene_debug_projector_launches.  k_tile's count shows that the
    occluder's depth is made real by the call when it was left on the chip (one depth-only repeat), never when it was
    stored, and the frame's only where it was not real yet."""
    W, Hh, pw, ph = 256, 48, 64, 64
    s = scene(W, Hh, small_synthetic, "phong", table(W, Hh), store_depth=store_depth, auto_group=False)
    occ = scene(pw, ph, small_synthetic, "phong", table(W, Hh), store_depth=store_depth, auto_group=False)
    img = PC.random_image(np.random.default_rng(1), pw, ph, 4)
    dev_img = on_device(img)
    m = two_cameras(W, Hh, img)
    drive(s), drive(occ, PC.CAM + SIDE)
    f, fo = snap(s), snap(occ)
    assert (PC.bits(fo["z"]) != PC.F32_MIN_BITS).any() and (PC.bits(fo["z"]) == PC.F32_MIN_BITS).any()
    plain = host(f, params(m, img, "normal"), img)
    seen = []
    for soft, bias in ((False, 0.0), (False, 3.0), (True, 3.0), (True, -1.0)):
        p = params(m, img, "normal", 256, True, soft, bias)
        want = host(f, p, img, fo["z"])
        seen.append(want)
        drive(s), drive(occ, PC.CAM + SIDE)      # both depths are left on the chip again (unless stored)
        s.profile_enable(True), occ.profile_enable(True)
        n0 = s.debug_projector_launches()
        s.projector(p, dev_img, occ)
        assert s.sync() == 0 and occ.sync() == 0
        ps, po = s.profile_read(), occ.profile_read()
        assert s.debug_projector_launches() == n0 + 1 and occ.debug_projector_launches() == 0
        repeat = 0 if store_depth else 1
        assert launches(ps, "k_tile") == repeat and launches(po, "k_tile") == repeat, (ps, po)      # (the frames themselves ran before the profile)
        same(s.get_frame_buffer(), want, "occluder, soft=%r bias=%r, in place" % (soft, bias))
        # both depths are real now: a second call repeats no pass
        same(s.get_projector(p, dev_img, occ), host(dict(f, fb=want), p, img, fo["z"]), "twice")
        ps, po = s.profile_read(), occ.profile_read()
        assert launches(ps, "k_tile") == repeat and launches(po, "k_tile") == repeat and s.debug_projector_launches() == n0 + 2, (ps, po)
        s.profile_enable(False), occ.profile_enable(False)
        # the occluder can be rendered again right after the call: the call read the frame it was issued under
        drive(s)
        s.projector(p, dev_img, occ)
        drive(occ, PC.CAM + 2.0)
        same(s.get_frame_buffer(), want, "the occluder rendered again behind the call")
        drive(occ, PC.CAM + SIDE)
    assert any(not np.array_equal(w, plain) for w in seen) and any(not np.array_equal(w, f["fb"]) for w in seen), "no shadow, or nothing but shadow"
    assert not np.array_equal(seen[1], seen[2]), "SOFT changes nothing"
    same(snap(occ)["z"], fo["z"], "the occluder's depth")
    s.close(), occ.close()


@pytest.mark.gpu
def test_the_scene_itself_as_occluder_and_a_cleared_occluder(small_synthetic):
    W, Hh = 257, 33
    s = scene(W, Hh, small_synthetic, "phong", table(W, Hh), tap=True)
    drive(s)
    f, before = snap(s), state(s)
    rng = np.random.default_rng(2)
    img = PC.random_image(rng, W, Hh, 3)
    dev_img = on_device(img)
    for m, soft, bias in ((PC.identity(), False, 0.0), (PC.identity(), True, -1.0), (PC.translation(1.5, -0.25), False, -0.5), (PC.translation(1.5, -0.25), True, 0.25)):
        p = params(m, img, "add", 256, True, soft, bias)
        want = all_four_forms(s, f, p, img, dev_img, "self", s, f["z"])
        same_state(state(s), before)
        drive(s)
    same(host(f, params(PC.identity(), img, "add", 256, True, False, 0.0), img, f["z"]), host(f, params(PC.identity(), img), img), "self, bias 0: lit")
    same(host(f, params(PC.identity(), img, "add", 256, True, True, -1.0), img, f["z"]), f["fb"], "self, bias -1: shadowed")
    # a logically cleared occluder shadows nothing and nothing of it is read
    occ = scene(W, Hh, small_synthetic, "phong", table(W, Hh))
    occ.clear()
    p = params(PC.translation(1.5, -0.25), img, "add", 256, True, True, 0.0)
    same(s.get_projector(p, dev_img, occ), host(f, params(PC.translation(1.5, -0.25), img), img), "a cleared occluder")
    s.close(), occ.close()


@pytest.mark.gpu
def test_an_occluder_with_raised_depth_flags_over_stale_memory(small_synthetic):
    """The occluder is rendered twice with the model in different places and its depth stored: the tiles the second frame
    leaves empty have their z flags up over the FIRST frame's depths.  Those count as f32::MIN."""
    W, Hh = 256, 48
    s = scene(W, Hh, small_synthetic, "phong", table(W, Hh))
    occ = scene(W, Hh, small_synthetic, "phong", TC._small(0.5, 0.0, 0.0, 0.5), store_depth=True)
    drive(s)
    f = snap(s)
    drive(occ, PC.CAM)
    first = snap(occ)
    occ.set_instances(TC._small(-0.6, 0.0, 0.0, 0.3))
    drive(occ, PC.CAM)
    img = PC.random_image(np.random.default_rng(3), W, Hh, 3)
    dev_img = on_device(img)
    outs = []
    for soft in (False, True):
        p = params(PC.translation(0.5, 0.5), img, "normal", 256, True, soft, 0.0)
        dev = device_buffer(W * Hh * 3)
        s.projector(p, dev_img, occ, out=dev.data_ptr())
        assert s.sync() == 0
        outs.append((p, dev.cpu().numpy().reshape(Hh, W, 3)))
    second = snap(occ)               # (reading the depth back makes it real)
    d1, d2 = PC.bits(first["z"]) != PC.F32_MIN_BITS, PC.bits(second["z"]) != PC.F32_MIN_BITS
    gone = tiles_any(d1) & ~tiles_any(d2)
    assert gone.any(), "no tile of the occluder was drawn in the first frame and empty in the second"
    for p, got in outs:
        want = host(f, p, img, second["z"])
        stale = host(f, p, img, np.where(d2, second["z"], first["z"]))
        assert not np.array_equal(want, stale), "the stale depths would decide no pixel"
        same(got, want, "raised flags over stale depths")
    s.close(), occ.close()


@pytest.mark.gpu
@pytest.mark.parametrize("pipe", ["phong", "shadow"])
def test_flags_state_and_consumers_after_in_place_calls(small_synthetic, pipe):
    import tiny_renderer_amd as T
    W, Hh = 384, 48
    s = scene(W, Hh, small_synthetic, pipe, PC.table(256, 48), tap=True)
    drive(s)
    f, before, flags = snap(s), state(s), clean_flags(s)
    empty = ~tiles_any(PC.bits(f["z"]) != PC.F32_MIN_BITS)
    assert empty.any() and (flags & empty).any() and not (flags & ~empty).any(), "flagged tiles are tiles with nothing drawn"
    drive(s)
    img = PC.random_image(np.random.default_rng(4), W, Hh, 4)
    dev_img = on_device(img)
    # MULTIPLY and DARKEN, and every other mode: tiles that nothing reached are still flagged
    for mode in ("multiply", "darken", "normal", "add"):
        p = params(PC.identity(), img, mode, 256)
        s.projector(p, dev_img)
        assert np.array_equal(clean_flags(s), flags), mode
        want = host(f, p, img)
        assert not np.array_equal(want, f["fb"])
        same(s.get_frame_buffer(), want, mode)
        same_state(state(s), before)
        drive(s)
    # twice in place is the host rule twice; the consumers that look at the flags see the result
    p = params(PC.translation(0.5, 0.0), img, "screen", 200)
    once = host(f, p, img)
    twice = host(dict(f, fb=once), p, img)
    assert not np.array_equal(once, twice)
    s.projector(p, dev_img), s.projector(p, dev_img)
    same(s.get_frame_buffer(), twice, "twice in place")
    out = s.pinned_frame()
    out[...] = 0x5A
    s.get_frame_buffer_async(out)
    assert s.sync() == 0
    same(out, twice, "the sparse read-back")
    same(s.resolve(2), box(twice, 2), "resolve")
    for got, ref in zip(s.to_yuv("i420"), T.yuv_host(twice, "i420")):
        assert np.array_equal(got, ref), "to_yuv"
    assert np.array_equal(clean_flags(s), flags)
    same_state(state(s), before)
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("W,Hh", [(256, 48), (131, 19)], ids=["words", "bytes"])
def test_dense_planted_backdrop_frames(small_synthetic, W, Hh):
    from tests import dense_cases as DC
    from tests import test_dense_frames as TD
    rng = np.random.default_rng(W + 1)
    img = PC.random_image(rng, 64, 64, 4)
    dev_img = on_device(img)
    for k, mode in enumerate(("normal", "difference")):
        s, buf, f = TD.dense_scene(small_synthetic, W, Hh, "planted")
        p = params(two_cameras(W, Hh, img), img, mode, (256, 180)[k])
        want = host(f, p, img)
        assert not np.array_equal(want, f["fb"])
        same(s.get_projector(p, dev_img), want, "dense, getter " + mode)
        s.projector(p, dev_img)
        assert s.sync() == 0
        TD.in_buffer(buf, want)
        undrawn = (PC.bits(f["z"]) == PC.F32_MIN_BITS)[::-1]
        assert np.array_equal(want[undrawn], f["fb"][undrawn]), "the backdrop stays"
        s.close()


@pytest.mark.gpu
def test_shortcuts_launch_nothing(small_synthetic):
    W, Hh = 200, 40
    s = scene(W, Hh, small_synthetic, "phong", table(W, Hh))
    img = PC.random_image(np.random.default_rng(5), W, Hh, 3)
    dev_img = on_device(img)
    s.profile_enable(True)
    p = params(PC.identity(), img, "normal", 256)
    s.clear()
    assert not s.get_projector(p, dev_img).any()
    s.clear()
    out = device_buffer(W * Hh * 3)
    s.projector(p, dev_img, out=out.data_ptr())
    assert s.sync() == 0 and not out.cpu().numpy().any(), "zeros out of place"
    s.clear()
    s.projector(p, dev_img)
    assert not s.get_frame_buffer().any()
    drive(s)
    f = snap(s)
    s.projector(params(PC.identity(), img, "normal", 0), dev_img)
    same(s.get_frame_buffer(), f["fb"], "opacity 0 in place")
    assert s.debug_projector_launches() == 0, "a shortcut launched the kernel"
    # opacity 0 out of place copies the frame
    same(s.get_projector(params(PC.identity(), img, "normal", 0), dev_img), f["fb"], "opacity 0, getter")
    assert s.debug_projector_launches() == 1 and "k_projector" not in s.profile_read()
    s.close()


@pytest.mark.gpu
def test_refusals_queue_nothing(small_synthetic):
    import tiny_renderer_amd as T
    from tiny_renderer_amd import _lib
    L = T.load_library()
    W, Hh = 256, 48
    s = scene(W, Hh, small_synthetic, "phong", table(W, Hh), tap=True)
    band = scene(W, Hh, small_synthetic, "phong", table(W, Hh), band_rows=(16, 32))
    other = scene(64, 64, small_synthetic, "phong", table(W, Hh))
    drive(s), drive(band), drive(other)
    f, before, flags = snap(s), state(s), clean_flags(s)
    img = PC.random_image(np.random.default_rng(6), W, Hh, 3)
    dev_img = on_device(img)
    ptr, stride = dev_img.data_ptr(), W * 3
    host_out = np.full((Hh, W, 3), 0xAA, np.uint8)
    dev = device_buffer(W * Hh * 3)
    for sc in (s, band, other):
        sc.profile_enable(True)      # (from here on: whatever a call queues shows in the profile or in the launch count)

    def text():
        return L.tr_last_error().decode()

    def make(**kw):
        p = params(PC.identity(), img)
        for k, v in kw.items():
            if k == "m5":
                p.m[5] = v
            elif k == "r0":
                p.reserved[0] = v
            else:
                setattr(p, k, v)
        return p

    bad = ((dict(pw=0), ": pw and ph must be 1..8192"), (dict(ph=8193), ": pw and ph must be 1..8192"), (dict(channels=5), ": channels must be 3 or 4"),
           (dict(mode=7), ": mode must be TR_LAYER_NORMAL .. TR_LAYER_DIFFERENCE"), (dict(flags=8), ": unknown flags"),
           (dict(flags=2), ": TR_PROJECTOR_SOFT needs TR_PROJECTOR_OCCLUDE"), (dict(opacity=257), ": opacity must be 0..256"),
           (dict(depth_bias=float("nan")), ": depth_bias must be finite"), (dict(m5=float("inf")), ": every entry of m must be finite"),
           (dict(r0=1), ": reserved must be 0"), (dict(flags=1), ": TR_PROJECTOR_OCCLUDE needs an occluder"))
    good = make()
    q = C.addressof(good)
    occl = make(flags=1)
    for who, call in (("tr_scene_projector", lambda sc, pp, im=ptr, st=stride, oc=None: L.tr_scene_projector(sc, pp, im, st, oc, None)),
                      ("tr_scene_get_projector", lambda sc, pp, im=ptr, st=stride, oc=None: L.tr_scene_get_projector(sc, pp, im, st, oc, host_out.ctypes.data))):
        for kw, why in bad:
            p = make(**kw)
            assert call(s._h, C.addressof(p)) == _lib.TR_E_INVALID and text() == who + why, kw
        assert call(None, q) == _lib.TR_E_INVALID and text() == who + ": null scene"
        assert call(s._h, None) == _lib.TR_E_INVALID and text() == who + ": null argument"
        assert call(s._h, q, im=None) == _lib.TR_E_INVALID and text() == who + ": null argument"
        assert call(s._h, q, st=stride - 1) == _lib.TR_E_INVALID and text() == who + ": image_stride must be at least the bytes of a row"
        assert call(s._h, q, oc=s._h) == _lib.TR_E_INVALID and text() == who + ": an occluder needs TR_PROJECTOR_OCCLUDE"
        assert call(s._h, C.addressof(occl), oc=other._h) == _lib.TR_E_INVALID and text() == who + ": the occluder scene's frame is not pw x ph"
        assert call(band._h, q) == _lib.TR_E_INVALID and text() == who + ": a band scene (tr_options.band_row0/1) cannot be projected on"
        assert call(s._h, C.addressof(occl), oc=band._h) == _lib.TR_E_INVALID
        assert text() == who + ": the occluder is a band scene (tr_options.band_row0/1): it holds only its rows of the depth"
        assert call(s._h, q, im=img.ctypes.data) == _lib.TR_E_INVALID
        assert text() == who + ": `image` is neither device memory nor from tr_host_alloc (tr_projector_host takes any host memory)"
        small = s.pinned_layer(4, 4)
        assert call(s._h, q, im=small.ctypes.data) == _lib.TR_E_INVALID and text() == who + ": the host buffer `image` is smaller than the image"
        assert call(s._h, q, im=int(s.band_tiles().frame_buffer_device)) == _lib.TR_E_INVALID and text() == who + ": `image` overlaps a frame buffer of the scene"
    assert L.tr_scene_get_projector(s._h, q, ptr, stride, None, None) == _lib.TR_E_INVALID and text() == "tr_scene_get_projector: null argument"
    assert L.tr_scene_projector(s._h, q, ptr, stride, None, host_out.ctypes.data) == _lib.TR_E_INVALID
    assert text() == "tr_scene_projector: `out` is neither device memory nor from tr_host_alloc (tr_scene_get_projector takes any host memory)"
    assert L.tr_scene_projector(s._h, q, ptr, stride, None, int(s.band_tiles().frame_buffer_device) + 3) == _lib.TR_E_INVALID
    assert text() == "tr_scene_projector: `out` overlaps a frame buffer of the scene (out == NULL projects in place)"
    assert L.tr_scene_projector(s._h, q, ptr, stride, None, s.pinned_layer(4, 4).ctypes.data) == _lib.TR_E_INVALID
    assert text() == "tr_scene_projector: the host buffer is smaller than the frame"
    assert L.tr_scene_projector(s._h, q, ptr, stride, None, ptr + 5) == _lib.TR_E_INVALID and text() == "tr_scene_projector: `image` overlaps `out`"
    assert (host_out == 0xAA).all() and (dev.cpu().numpy() == 0x5A).all(), "a refused call wrote `out`"
    assert s.sync() == 0
    for sc in (s, band, other):
        assert sc.debug_projector_launches() == 0 and not sc.profile_read(), "a refused call queued a kernel"
    assert np.array_equal(clean_flags(s), flags)
    same(s.get_frame_buffer(), f["fb"], "a refused call changed the frame")
    same_state(state(s), before)
    with pytest.raises(ValueError):
        s.projector(PC.identity(), dev_img, occluder=7)
    with pytest.raises(ValueError):
        s.projector(good, on_device(img[:, :-1]))
    with pytest.raises(ValueError):
        s.projector(PC.identity(), dev_img, soft=True)
    s.close(), band.close(), other.close()


@pytest.mark.gpu
def test_the_cli_casts_an_image_with_shadows_in_a_child_process(built, tmp_path):
    """--projector FILE.tga --projector-shadows --projector-soft writes what projector_host gives on the plain render with
    the depth of a second scene rendered from the projector; --fog lies over the projected light.  Fresh processes."""
    import os
    import subprocess
    import sys
    import tiny_renderer_amd as T
    REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    W, Hh, pw, ph = 200, 120, 48, 40
    img = PC.random_image(np.random.default_rng(9), pw, ph, 3)
    tga = str(tmp_path / "slide.tga")
    T.save_tga(tga, img)
    mesh, texs = T.synthetic_scene()
    s = T.Scene(W, Hh, mesh, texs, "phong")
    drive(s, 0.3, 0.7)
    f = snap(s)
    stand, at = [1.2, 0.5, 1.0], [0.0, 0.0, 0.0]
    occ = T.Scene(pw, ph, mesh, texs, "default", store_depth=True)
    occ.clear(), occ.set_light_direction(list(s._light)), occ.set_camera(stand, at, list(s._camera[2])), occ.render()
    fo = snap(occ)
    st, view = T.prepare_uniforms(2, W, Hh, s._light, *s._camera)
    st2, proj = T.prepare_uniforms(0, pw, ph, s._light, stand, at, list(s._camera[2]))
    assert st == 0 and st2 == 0
    m = T.projector_matrix(view, proj)
    s.close(), occ.close()
    common = [sys.executable, "-m", "tiny_renderer_amd.cli", "--synthetic", "-s", "phong", "--width", str(W), "--height", str(Hh), "--camera-angle", "0.3",
              "--light-angle", "0.7"]
    place = ["--projector", tga, "--projector-from", "1.2,0.5,1.0", "--projector-at", "0,0,0"]
    runs = {"plain": [], "cast": place + ["--projector-mode", "screen", "--projector-opacity", "200"],
            "shadowed": place + ["--projector-shadows", "--projector-soft", "--projector-bias", "1.5", "--fog", "200,210,230", "--fog-span", "80,30"]}
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    hd = b"P6\n%d %d\n255\n" % (W, Hh)
    got = {}
    for name, extra in runs.items():
        path = str(tmp_path / (name + ".ppm"))
        done = subprocess.run(common + extra + ["--out", path], capture_output=True, text=True, cwd=REPO, env=env, timeout=120)
        assert done.returncode == 0, done.stdout + done.stderr
        got[name] = np.frombuffer(open(path, "rb").read()[len(hd):], np.uint8).reshape(Hh, W, 3)
    same(got["plain"], f["fb"], "the child's plain render")
    cast = host(f, params(m, img, "screen", 200), img)
    assert not np.array_equal(cast, f["fb"])
    same(got["cast"], cast, "--projector")
    shadowed = host(f, params(m, img, "add", 256, True, True, 1.5), img, fo["z"])
    assert not np.array_equal(shadowed, host(f, params(m, img, "add", 256), img)), "the model shadows nothing"
    fogged = T.ramp_host(shadowed, f["z"], T.ramp_fog((200, 210, 230)), T.ramp_params(*T.ramp_span(80.0, 30.0, 256)))
    same(got["shadowed"], fogged, "--projector-shadows --projector-soft under --fog")
    bad = subprocess.run(common + ["--projector-soft"], capture_output=True, text=True, cwd=REPO, env=env, timeout=120)
    assert bad.returncode != 0 and "--projector" in bad.stderr
