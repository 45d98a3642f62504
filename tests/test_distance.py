"""The distance field on the device: tr_scene_distance / tr_scene_get_distance (k_dist_mask, k_dist_row, k_dist) equal
tr_distance_host in every u16, and tr_scene_distance_ramp / tr_scene_get_distance_ramped (k_dist_apply behind them)
equal tr_distance_ramp_host in every byte.

Every comparison is np.array_equal against the host rule of what the scene itself returns (get_frame_buffer,
read_z_f32); tests/test_distance_host.py pins the host rule against the all-pairs minimum in numpy and asserts, on the
oracle's frames of these very cases, that every size has seeds, near pixels, FAR pixels and a tile that is all FAR."""
import ctypes as C

import numpy as np
import pytest

from tests import dense_cases as DN
from tests import distance_cases as DC
from tests import ramp_cases as RC
from tests import test_composite as TC
from tests import test_outline as TO

scene, snap, clean_flags, tiles_any = TC.scene, TC.snap, TC.clean_flags, TC.tiles_any
other_synthetic = TC.other_synthetic
device_buffer, state, same_state, box = TO.device_buffer, TO.state, TO.same_state, TO.box
GUARD = 64
FAR = DC.FAR
ALL_SIZES = tuple(DC.SIZES) + DC.EXTRA
IDS = ["%dx%d" % s for s in ALL_SIZES]
# (seed, threshold, invert): DRAWN, and KEY at threshold 0, 1, 128, 255, with and without INVERT
SEEDS = (("drawn", 0, False), ("drawn", 0, True), ("key", 0, False), ("key", 1, False), ("key", 128, True), ("key", 255, False), ("key", 1, True),
         ("key", 128, False), ("key", 255, True), ("key", 0, True))


def drive(s, cam=DC.CAM, light=DC.LIGHT, clear=True):
    TC.drive(s, cam, light, clear)


def same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype and np.array_equal(got, want), "%s: %d values differ" % (what, int((got != want).sum()))


def host_field(f, radius, seed="drawn", threshold=0, invert=False):
    import tiny_renderer_amd as T
    return T.distance_host(f["fb"], f["z"], T.distance_params(radius, seed, threshold, invert))


def ramp_kw(radius, step=256, mode="normal", opacity=256, repeat=False, alpha=0, keep=False, seed="drawn", threshold=0, invert=False):
    return dict(radius=radius, step=step, seed=seed, threshold=threshold, invert=invert, mode=mode, opacity=opacity, far=DC.far_of(alpha), repeat=repeat,
                keep_seeds=keep)


def host_ramp(f, tab, kw):
    import tiny_renderer_amd as T
    return T.distance_ramp_host(f["fb"], f["z"], tab, T.distance_ramp_params(**kw))


def guarded_u16(n, off):
    """A device block of n u16 at an odd multiple of 2 bytes between two guards of 0xAA: (tensor, byte offset)."""
    import torch
    out = torch.full((2 * n + 2 * GUARD + off,), 0xAA, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert out.data_ptr() % 4 == 0 and (GUARD + off) % 4 == 2
    return out, GUARD + off


@pytest.mark.gpu
@pytest.mark.parametrize("W,Hh", ALL_SIZES, ids=IDS)
def test_field_equals_the_host_rule_in_all_three_forms(small_synthetic, W, Hh):
    """Every radius and every seed form through the getter; into device memory at an odd multiple of 2 bytes between
    guards and into a tr_host_alloc block for one radius a seed form, the radius in turn."""
    s = scene(W, Hh, small_synthetic, "phong", DC.table(W, Hh), tap=True)
    drive(s)
    f, before, flags = snap(s), state(s), clean_flags(s)
    pinned = s.pinned_field()
    assert pinned.shape == (Hh, W) and pinned.dtype == np.uint16
    n = W * Hh
    seen = set()
    for i, (seed, thr, inv) in enumerate(SEEDS):
        for R in DC.GPU_RADII:
            want = host_field(f, R, seed, thr, inv)
            seen.update(np.unique(want).tolist())
            same(s.get_distance(R, seed, thr, inv), want, "getter R %d %s %d %s" % (R, seed, thr, inv))
        R = DC.GPU_RADII[i % 4]
        want = host_field(f, R, seed, thr, inv)
        dev, off = guarded_u16(n, 2)
        pinned[...] = 0xABAB
        s.distance(dev.data_ptr() + off, R, seed, thr, inv)
        s.distance(pinned, R, seed, thr, inv)
        assert s.sync() == 0
        raw = dev.cpu().numpy()
        same(raw[off:off + 2 * n].view(np.uint16).reshape(Hh, W), want, "device memory R %d %s %d %s" % (R, seed, thr, inv))
        assert (raw[:off] == 0xAA).all() and (raw[off + 2 * n:] == 0xAA).all(), "a guard byte changed"
        same(pinned, want, "tr_host_alloc R %d %s %d %s" % (R, seed, thr, inv))
    assert 0 in seen and FAR in seen and len(seen) > 10, "the cases hold seeds, FAR pixels and distances between"
    assert np.array_equal(clean_flags(s), flags), "a field call changed the frame's flags"
    same(s.get_frame_buffer(), f["fb"], "a field call leaves the scene's frame")
    same_state(state(s), before)
    s.close()


@pytest.mark.gpu
def test_a_tensor_as_out_and_the_profile(small_synthetic):
    import torch
    W, Hh = 384, 48
    s = scene(W, Hh, small_synthetic, "phong", DC.table(W, Hh))
    s.profile_enable(True)
    drive(s)
    f = snap(s)
    out = torch.full((Hh, W), 0x5A5A, dtype=torch.int16, device="cuda")
    s.distance(out, 16)
    assert s.sync() == 0
    same(out.cpu().numpy().view(np.uint16), host_field(f, 16), "a tensor")
    prof = s.profile_read()
    # the three field kernels share one name in the profile
    assert prof.get("k_dist", {}).get("launches") == 3 and prof["k_dist"]["total_ms"] > 0.0, prof.get("k_dist")
    assert "k_dist_apply" not in prof
    s.set_ramp(RC.random_table(np.random.default_rng(1), 16))
    s.distance_ramp(16)
    assert s.sync() == 0
    prof = s.profile_read()
    assert prof["k_dist"]["launches"] == 6 and prof["k_dist_apply"]["launches"] == 1, prof
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("store_depth", [False, True], ids=["transient", "stored"])
def test_frames_behind_flags(small_synthetic, other_synthetic, store_depth):
    """A logically cleared scene; whole tiles nothing drew into (their z and colour flags are up: constant mask words); a
    depth left on the chip made real under DRAWN; a composited frame; a frame graded in place to one flat colour."""
    import tiny_renderer_amd as T
    W, Hh = 384, 48
    s = scene(W, Hh, small_synthetic, "phong", DC.table(W, Hh), store_depth=store_depth, auto_group=False)
    s.clear()
    assert (s.get_distance(16) == FAR).all(), "cleared, DRAWN"
    s.clear()
    assert (s.get_distance(16, invert=True) == 0).all(), "cleared, DRAWN inverted"
    s.clear()
    assert (s.get_distance(16, "key", 0) == 0).all(), "cleared, KEY at threshold 0"
    s.clear()
    assert (s.get_distance(255, "key", 1) == FAR).all(), "cleared, KEY at threshold 1"
    s.clear()
    out = device_buffer(W * Hh * 2, 0xAB)
    s.distance(out.data_ptr(), 4, "key", 0, True)
    assert s.sync() == 0
    assert (out.cpu().numpy().view(np.uint16) == FAR).all(), "cleared, KEY at threshold 0 inverted, device memory"
    assert not s.get_frame_buffer().any(), "the cleared scene stays cleared"
    # a rendered frame: the field call is the first consumer of its depth
    drive(s)
    got = {R: s.get_distance(R) for R in (4, 255)}
    key = s.get_distance(16, "key", 1)
    flags = clean_flags(s)
    f = snap(s)
    assert flags.any() and not flags.all(), "tiles behind a raised colour flag and tiles without"
    for R in got:
        same(got[R], host_field(f, R), "the call made the depth real itself, R %d" % R)
    same(key, host_field(f, 16, "key", 1), "KEY behind raised colour flags")
    # a composited frame with merged depth
    src = scene(W, Hh, other_synthetic, "phong", store_depth=store_depth)
    drive(src, cam=1.1)
    s.composite(src)
    got = s.get_distance(16), s.get_distance(16, "key", 128, True)
    m = snap(s)
    assert not np.array_equal(RC.bits(m["z"]), RC.bits(f["z"])), "the merge changed no depth"
    same(got[0], host_field(m, 16), "after a composite, DRAWN")
    same(got[1], host_field(m, 16, "key", 128, True), "after a composite, KEY inverted")
    src.close()
    # graded in place to one flat colour: every tile is real, every pixel is (or is not) a seed under KEY
    drive(s)
    lut = np.empty((2, 2, 2, 3), np.uint8)
    lut[...] = (40, 130, 7)
    s.set_lut(lut)
    s.grade()
    assert not clean_flags(s).any() and (s.get_frame_buffer() == (40, 130, 7)).all()
    assert (s.get_distance(9, "key", 130) == 0).all() and (s.get_distance(9, "key", 131) == FAR).all()
    assert (s.get_distance(9, "key", 130, True) == FAR).all()
    same(s.get_distance(9), host_field(f, 9), "DRAWN after the grade: the depth is the frame's")
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", DN.BACKDROPS)
def test_dense_backdrops_under_key(small_synthetic, kind):
    """dense_cases' backdrops layered behind the model: no tile is flagged, and the key finds seeds all over the frame."""
    import torch
    W, Hh = DN.MIDDLE
    s = scene(W, Hh, small_synthetic, DN.PIPE, DN.table(W, Hh))
    drive(s)
    s.layer(torch.from_numpy(DN.backdrop(kind, W, Hh)).cuda(), where="undrawn")
    f = snap(s)
    for thr, inv, R in ((128, False, 4), (250, False, 255), (200, True, 16), (255, False, 16)):
        same(s.get_distance(R, "key", thr, inv), host_field(f, R, "key", thr, inv), "%s, threshold %d" % (kind, thr))
    same(s.get_distance(16), host_field(f, 16), kind + ", DRAWN")
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("W,Hh", ALL_SIZES, ids=IDS)
def test_ramped_frame_equals_the_host_rule_in_all_four_forms(small_synthetic, W, Hh):
    """distance_cases.SHORT's modes (ramp_cases.SHORT's, with KEEP_SEEDS in turn), the seed kind and the radius in turn:
    through the getter, into device memory, into a tr_host_alloc block and in place."""
    s = scene(W, Hh, small_synthetic, "phong", DC.table(W, Hh), tap=True)
    tab = RC.random_table(np.random.default_rng(W * Hh), 64)
    s.set_ramp(tab)
    drive(s)
    f, before, flags = snap(s), state(s), clean_flags(s)
    pinned = s.pinned_frame()
    for i, (mode, opacity, repeat, alpha, keep) in enumerate(DC.SHORT):
        seed, thr, inv = (("drawn", 0, False), ("key", 128, False), ("drawn", 0, True))[i % 3]
        kw = ramp_kw((4, 16, 255)[i % 3], (256, 700, 90)[i % 3], mode, opacity, repeat, alpha, keep, seed, thr, inv)
        want = host_ramp(f, tab, kw)
        assert not np.array_equal(want, f["fb"])
        same(s.get_distance_ramped(**kw), want, "getter %r" % (kw,))
        dev = device_buffer(W * Hh * 3 + 1, 0xAB)
        pinned[...] = 0xAB
        s.distance_ramp(out=dev.data_ptr() + 1, **kw)
        s.distance_ramp(out=pinned, **kw)
        assert s.sync() == 0
        same(dev.cpu().numpy()[1:].reshape(Hh, W, 3), want, "device memory at an odd address %r" % (kw,))
        same(pinned, want, "tr_host_alloc %r" % (kw,))
        assert np.array_equal(clean_flags(s), flags), "an out-of-place call changed the frame's flags"
        same(s.get_frame_buffer(), f["fb"], "out of place leaves the scene's frame")
        s.distance_ramp(**kw)
        same(s.get_frame_buffer(), want, "in place %r" % (kw,))
        same_state(state(s), before)
        drive(s)
    s.close()


@pytest.mark.gpu
def test_the_builders_keep_seeds_and_in_place_twice(small_synthetic):
    import tiny_renderer_amd as T
    W, Hh = 256, 48
    s = scene(W, Hh, small_synthetic, "phong", DC.table(W, Hh), tap=True)
    drive(s)
    f, before = snap(s), state(s)
    seeds = DC.seeds_np(f["fb"], f["z"])
    builders = ((T.ramp_glow(DC.GLOW, 12, "smooth"), dict(radius=12, mode="add", keep=True)), (T.ramp_stroke((10, 20, 30), 3), dict(radius=5, keep=True)),
                (T.ramp_rings((0, 0, 0, 200), 6, 2), dict(radius=40, repeat=True)), (T.ramp_glow((255, 255, 255), 8), dict(radius=8, invert=True, keep=True)))
    for (tab, step), extra in builders:
        s.set_ramp(tab)
        kw = ramp_kw(step=step, **extra)
        want = host_ramp(f, tab, kw)
        assert not np.array_equal(want, f["fb"])
        if kw["keep_seeds"]:
            m = ~seeds if kw["invert"] else seeds
            assert np.array_equal(want[m], f["fb"][m]), "KEEP_SEEDS touched a seed"
        same(s.get_distance_ramped(**kw), want, "getter")
        s.distance_ramp(**kw)
        same(s.get_frame_buffer(), want, "in place")
        # twice: the second call's seeds and colours are the first call's frame (the depth has not changed)
        twice = host_ramp(dict(f, fb=want), tab, kw)
        s.distance_ramp(**kw)
        same(s.get_frame_buffer(), twice, "in place twice")
        same_state(state(s), before)
        drive(s)
    # under KEY the seeds are read before any colour changes: an opaque stroke that would make new seeds
    tab, step = T.ramp_stroke((255, 255, 255), 6)
    s.set_ramp(tab)
    kw = ramp_kw(8, step, seed="key", threshold=128)
    want = host_ramp(f, tab, kw)
    s.distance_ramp(**kw)
    same(s.get_frame_buffer(), want, "KEY in place")
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("pipe", ["phong", "shadow"])
def test_what_stays_and_which_flags_come_down(small_synthetic, other_synthetic, pipe):
    import tiny_renderer_amd as T
    W, Hh = 384, 48
    s = scene(W, Hh, small_synthetic, pipe, DC.table(W, Hh), tap=True)
    tab = RC.random_table(np.random.default_rng(3), 256)
    s.set_ramp(tab)
    drive(s)
    f, before, flags = snap(s), state(s), clean_flags(s)
    # far alpha 0: a tile whose pixels are all FAR is left behind its flag, whatever the mode; a flagged tile in reach is
    # stored whole and its flag comes down, but under MULTIPLY.  At R = 4 the flagged tiles are out of reach, at R = 40 in it
    seen = [False, False]
    for R in (4, 40):
        far_tiles = ~tiles_any((host_field(f, R) != FAR)[::-1])
        seen = [seen[0] or (flags & far_tiles).any(), seen[1] or (flags & ~far_tiles).any()]
        for mode in ("normal", "add", "multiply"):
            drive(s)
            kw = ramp_kw(R, 256, mode)
            s.distance_ramp(**kw)
            assert np.array_equal(clean_flags(s), flags & (far_tiles | (mode == "multiply"))), (R, mode)
            same(s.get_frame_buffer(), host_ramp(f, tab, kw), mode)
            same_state(state(s), before)
    assert all(seen), "flagged tiles that are all FAR, and flagged tiles in reach"
    drive(s)
    # MULTIPLY and DARKEN keep a flagged tile black behind its flag, with an opaque `far` too
    for mode in ("multiply", "darken"):
        kw = ramp_kw(4, 256, mode, alpha=255)
        s.distance_ramp(**kw)
        assert np.array_equal(clean_flags(s), flags), mode
        same(s.get_frame_buffer(), host_ramp(f, tab, kw), mode)
        drive(s)
    # far alpha 255 under NORMAL: every flagged tile is stored whole and its flag comes down; every consumer sees it
    kw = ramp_kw(4, 256, "normal", alpha=255)
    want = host_ramp(f, tab, kw)
    s.distance_ramp(**kw)
    assert not clean_flags(s).any(), "a tile that holds the far colour is still flagged clean"
    same(s.get_frame_buffer(), want, "get_frame_buffer")
    out = s.pinned_frame()
    out[...] = 0x5A
    s.get_frame_buffer_async(out)
    assert s.sync() == 0
    same(out, want, "the sparse read-back")
    same(s.resolve(2), box(want, 2), "resolve")
    assert np.array_equal(s.get_frame_stats().raw, T.frame_stats_host(want).raw), "frame_stats"
    same_state(state(s), before)
    s.close()


@pytest.mark.gpu
def test_refusals_queue_nothing(small_synthetic):
    import tiny_renderer_amd as T
    from tiny_renderer_amd import _lib
    L = T.load_library()
    W, Hh = 256, 48
    s = scene(W, Hh, small_synthetic, "phong", DC.table(W, Hh), tap=True)
    band = scene(W, Hh, small_synthetic, "phong", DC.table(W, Hh), band_rows=(16, 32))
    bare = scene(W, Hh, small_synthetic, "phong", DC.table(W, Hh))
    tab = RC.random_table(np.random.default_rng(4), 256)
    s.set_ramp(tab), band.set_ramp(tab)
    drive(s), drive(band), drive(bare)
    f, before, flags = snap(s), state(s), clean_flags(s)
    host16 = np.full((Hh, W), 0xAAAA, np.uint16)
    host8 = np.full((Hh, W, 3), 0xAA, np.uint8)
    dev = device_buffer(W * Hh * 3)

    def text():
        return L.tr_last_error().decode()

    def fparams(seed=0, threshold=0, radius=4, flags=0, res=(0, 0, 0, 0)):
        return T.DistanceParams(seed, threshold, radius, flags, (C.c_uint32 * 4)(*res))

    def rparams(field=None, step=256, mode=0, opacity=256, far=0xFF102030, flags=0, res=(0, 0, 0)):
        return T.DistanceRampParams(field or fparams(), step, mode, opacity, far, flags, (C.c_uint32 * 3)(*res))

    for sc in (s, band, bare):
        sc.profile_enable(True)
    bad_field = ((dict(seed=2), ": seed must be TR_DIST_SEED_DRAWN or TR_DIST_SEED_KEY"), (dict(threshold=256), ": threshold must be 0..255"),
                 (dict(radius=0), ": radius must be 1..TR_DIST_MAX_RADIUS"), (dict(radius=256), ": radius must be 1..TR_DIST_MAX_RADIUS"),
                 (dict(flags=2), ": unknown flags"), (dict(res=(1, 0, 0, 0)), ": reserved must be 0"))
    bad_ramp = ((dict(step=0), ": step must be 1..65536"), (dict(step=65537), ": step must be 1..65536"),
                (dict(mode=7), ": mode must be TR_LAYER_NORMAL .. TR_LAYER_DIFFERENCE"), (dict(opacity=257), ": opacity must be 0..256"),
                (dict(flags=4), ": unknown flags"), (dict(res=(0, 0, 1)), ": reserved must be 0"))
    field_calls = (("tr_scene_distance", lambda sc, pp: L.tr_scene_distance(sc, pp, dev.data_ptr())),
                   ("tr_scene_get_distance", lambda sc, pp: L.tr_scene_get_distance(sc, pp, host16.ctypes.data)))
    ramp_calls = (("tr_scene_distance_ramp", lambda sc, pp: L.tr_scene_distance_ramp(sc, pp, None)),
                  ("tr_scene_get_distance_ramped", lambda sc, pp: L.tr_scene_get_distance_ramped(sc, pp, host8.ctypes.data)))
    for who, call in field_calls:
        for kw, why in bad_field:
            p = fparams(**kw)
            assert call(s._h, C.addressof(p)) == _lib.TR_E_INVALID and text() == who + why, kw
            assert call(band._h, C.addressof(p)) == _lib.TR_E_INVALID and text() == who + why, kw   # parameters first, then the scene
        good = fparams()
        assert call(s._h, None) == _lib.TR_E_INVALID and text() == who + ": null argument"
        assert call(None, C.addressof(good)) == _lib.TR_E_INVALID and text() == who + ": null scene"
        assert call(band._h, C.addressof(good)) == _lib.TR_E_INVALID and text() == who + ": a band scene (tr_options.band_row0/1) has no distance field"
    for who, call in ramp_calls:
        for kw, why in bad_field:
            p = rparams(fparams(**kw))
            assert call(s._h, C.addressof(p)) == _lib.TR_E_INVALID and text() == who + why, kw
        for kw, why in bad_ramp:
            p = rparams(**kw)
            assert call(s._h, C.addressof(p)) == _lib.TR_E_INVALID and text() == who + why, kw
            assert call(bare._h, C.addressof(p)) == _lib.TR_E_INVALID and text() == who + why, kw
        good = rparams()
        assert call(s._h, None) == _lib.TR_E_INVALID and text() == who + ": null argument"
        assert call(None, C.addressof(good)) == _lib.TR_E_INVALID and text() == who + ": null scene"
        assert call(bare._h, C.addressof(good)) == _lib.TR_E_INVALID and text() == who + ": the scene has no ramp table (tr_scene_set_ramp)"
        assert call(band._h, C.addressof(good)) == _lib.TR_E_INVALID and text() == who + ": a band scene (tr_options.band_row0/1) has no distance field"
    g, r = fparams(), rparams()
    q, qr = C.addressof(g), C.addressof(r)
    assert L.tr_scene_get_distance(s._h, q, None) == _lib.TR_E_INVALID and text() == "tr_scene_get_distance: null argument"
    assert L.tr_scene_get_distance_ramped(s._h, qr, None) == _lib.TR_E_INVALID and text() == "tr_scene_get_distance_ramped: null argument"
    assert L.tr_scene_distance(s._h, q, None) == _lib.TR_E_INVALID
    assert text() == "tr_scene_distance: out == NULL (the field is no frame of the scene: there is no in-place form)"
    assert L.tr_scene_distance(s._h, q, host16.ctypes.data) == _lib.TR_E_INVALID
    assert text() == "tr_scene_distance: `out` is neither device memory nor from tr_host_alloc (tr_scene_get_distance takes any host memory)"
    assert L.tr_scene_distance_ramp(s._h, qr, host8.ctypes.data) == _lib.TR_E_INVALID
    assert text() == "tr_scene_distance_ramp: `out` is neither device memory nor from tr_host_alloc (tr_scene_get_distance_ramped takes any host memory)"
    assert L.tr_scene_distance(s._h, q, dev.data_ptr() + 1) == _lib.TR_E_INVALID and text() == "tr_scene_distance: `out` must be 2-byte aligned"
    fb = int(s.band_tiles().frame_buffer_device)
    assert L.tr_scene_distance(s._h, q, fb + 2) == _lib.TR_E_INVALID
    assert text() == "tr_scene_distance: `out` overlaps a frame buffer of the scene (there is no in-place form)"
    assert L.tr_scene_distance_ramp(s._h, qr, fb + 3) == _lib.TR_E_INVALID
    assert text() == "tr_scene_distance_ramp: `out` overlaps a frame buffer of the scene (out == NULL ramps in place)"
    small = s.pinned_layer(4, 4)
    assert L.tr_scene_distance(s._h, q, small.ctypes.data) == _lib.TR_E_INVALID and text() == "tr_scene_distance: the host buffer is smaller than the field"
    assert L.tr_scene_distance_ramp(s._h, qr, small.ctypes.data) == _lib.TR_E_INVALID
    assert text() == "tr_scene_distance_ramp: the host buffer is smaller than the frame"
    assert (host16 == 0xAAAA).all() and (host8 == 0xAA).all() and (dev.cpu().numpy() == 0x5A).all(), "a refused call wrote `out`"
    assert s.sync() == 0
    for sc in (s, band, bare):
        assert not [k for k in sc.profile_read() if k.startswith("k_dist")], "a refused call queued a kernel"
    assert np.array_equal(clean_flags(s), flags)
    same(s.get_frame_buffer(), f["fb"], "a refused call changed the frame")
    same_state(state(s), before)
    # a dropped table is a refusal of the ramp calls alone
    s.set_ramp(None)
    assert L.tr_scene_distance_ramp(s._h, qr, None) == _lib.TR_E_INVALID and text() == "tr_scene_distance_ramp: the scene has no ramp table (tr_scene_set_ramp)"
    same(s.get_distance(4), host_field(f, 4), "the field needs no table")
    with pytest.raises(T.TinyRendererError):
        s.distance(np.zeros((Hh, W), np.uint16), 4)          # (ordinary host memory: the library's refusal)
    with pytest.raises(ValueError):
        s.distance(np.zeros((Hh, W), np.uint8), 4)
    with pytest.raises(ValueError):
        s.distance(None, 4)
    with pytest.raises(ValueError):
        s.distance_ramp(0)
    s.close(), band.close(), bare.close()


@pytest.mark.gpu
def test_the_cli_in_a_child_process(built, tmp_path):
    """--glow, --stroke and --inner-glow write what distance_ramp_host gives on the plain render; each run is a fresh
    process.  With --gpus 2 they are refused."""
    import os
    import subprocess
    import sys
    import tiny_renderer_amd as T
    REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    W, Hh = 200, 120
    common = [sys.executable, "-m", "tiny_renderer_amd.cli", "--synthetic", "-s", "phong", "--width", str(W), "--height", str(Hh), "--camera-angle", "0.3",
              "--light-angle", "0.7"]
    runs = {"plain": [], "glow": ["--glow", "255,200,40", "--glow-radius", "12"], "stroke": ["--stroke", "10,20,30,200", "--stroke-width", "3"],
            "inner": ["--inner-glow", "255,255,255"]}
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    hd = b"P6\n%d %d\n255\n" % (W, Hh)
    got = {}
    for name, extra in runs.items():
        path = str(tmp_path / (name + ".ppm"))
        done = subprocess.run(common + extra + ["--out", path], capture_output=True, text=True, cwd=REPO, env=env, timeout=120)
        assert done.returncode == 0, done.stdout + done.stderr
        got[name] = np.frombuffer(open(path, "rb").read()[len(hd):], np.uint8).reshape(Hh, W, 3)
    mesh, texs = T.synthetic_scene()
    s = T.Scene(W, Hh, mesh, texs, "phong")
    drive(s, 0.3, 0.7)
    f = snap(s)
    s.close()
    same(got["plain"], f["fb"], "the child's plain render")

    def want(table_step, radius, **kw):
        return T.distance_ramp_host(f["fb"], f["z"], table_step[0], T.distance_ramp_params(radius, table_step[1], keep_seeds=True, **kw))

    same(got["glow"], want(T.ramp_glow((255, 200, 40), 12), 12, mode="add"), "--glow")
    same(got["stroke"], want(T.ramp_stroke((10, 20, 30, 200), 3), 4), "--stroke")
    same(got["inner"], want(T.ramp_glow((255, 255, 255), 24), 24, mode="add", invert=True), "--inner-glow")
    assert not np.array_equal(got["glow"], got["plain"]) and not np.array_equal(got["inner"], got["plain"])
    bad = subprocess.run(common + ["--glow-radius", "9"], capture_output=True, text=True, cwd=REPO, env=env, timeout=120)
    assert bad.returncode != 0 and "--glow-radius" in bad.stderr
    bad = subprocess.run(common + ["--glow", "1,2,3", "--gpus", "2"], capture_output=True, text=True, cwd=REPO, env=env, timeout=120)
    assert bad.returncode != 0 and "--gpus 1" in bad.stderr
