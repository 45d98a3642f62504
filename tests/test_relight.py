"""Relighting on the device: tr_scene_relight / tr_scene_get_relit (k_relight) equal tr_relight_host in every byte.

Every comparison is np.array_equal against relight_host of what the scenes themselves return (get_frame_buffer,
read_z_f32); tests/test_relight_host.py pins relight_host against hand-computed values, the layer rule and the rule in
numpy."""
import ctypes as C

import numpy as np
import pytest

from tests import relight_cases as RC
from tests import test_composite as TC
from tests import test_outline as TO

scene, snap, clean_flags, tiles_any = TC.scene, TC.snap, TC.clean_flags, TC.tiles_any
device_buffer, state, same_state, box = TO.device_buffer, TO.state, TO.same_state, TO.box
IDS = ["%dx%d" % s for s in RC.GPU_SIZES]


def drive(s, cam=RC.CAM, light=RC.LIGHT, clear=True):
    TC.drive(s, cam, light, clear)


def same(got, want, what):
    assert got.shape == want.shape and np.array_equal(got, want), "%s: %d bytes differ" % (what, int((got != want).sum()))


def table(W, Hh):
    return TC.DST_AT if W < 128 else RC.table(W, Hh)


def host(f, p, lights=()):
    import tiny_renderer_amd as T
    return T.relight_host(f["fb"], f["z"], p, lights)


def all_four_forms(s, f, p, lights, what):
    """The getter, device memory at an odd byte address, a tr_host_alloc block and in place against the host rule, one
    k_relight each.  Returns the expected frame; the scene's frame is the lit one afterwards."""
    W, Hh = s.width, s.height
    want = host(f, p, lights)
    flags, n0 = clean_flags(s), s.debug_relight_launches()
    same(s.get_relit(p, lights), want, what + ": getter")
    dev, pinned = device_buffer(W * Hh * 3 + 1, 0xAB), s.pinned_frame()
    pinned[...] = 0xAB
    assert (dev.data_ptr() + 1) % 2 == 1
    s.relight(p, lights, out=dev.data_ptr() + 1)
    s.relight(p, lights, out=pinned)
    assert s.sync() == 0
    got = dev.cpu().numpy()
    assert got[0] == 0xAB, "the byte in front of `out`"
    same(got[1:].reshape(Hh, W, 3), want, what + ": device memory at an odd address")
    same(pinned, want, what + ": tr_host_alloc")
    assert np.array_equal(clean_flags(s), flags), "an out-of-place call changed the frame's flags"
    same(s.get_frame_buffer(), f["fb"], what + ": out of place leaves the scene's frame")
    s.relight(p, lights)
    same(s.get_frame_buffer(), want, what + ": in place")
    assert s.debug_relight_launches() == n0 + 4, "one launch per call"
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("W,Hh", RC.GPU_SIZES, ids=IDS)
def test_frame_sizes_light_sets_modes_and_all_four_forms(small_synthetic, W, Hh):
    """Every frame size (phong and shadow in turn): no light but the ambient term, one light of each kind, eight lights
    with and without highlights, every mode once, ALBEDO and SHOW_NORMALS, through all four entry-point forms."""
    import tiny_renderer_amd as T
    pipe = ("phong", "shadow")[RC.GPU_SIZES.index((W, Hh)) % 2]
    s = scene(W, Hh, small_synthetic, pipe, table(W, Hh), tap=True)
    drive(s)
    f, before = snap(s), state(s)
    drawn = RC.bits(f["z"]) != RC.F32_MIN_BITS
    assert drawn.any(), "nothing is drawn"
    valid = T.relight_normals_host(f["z"], RC.view_params(W, Hh))[1]
    assert valid.any() and not (valid & ~drawn).any()
    eight, plain = RC.scene_lights(8), RC.scene_lights(8, specular=False)
    cases = (("ambient alone", (), dict(ambient=(40, 90, 160), mode="normal", opacity=200)),
             ("a point light", eight[0:1], dict(mode="add")),
             ("a spot light", eight[1:2], dict(mode="screen", ambient=(10, 10, 10))),
             ("a directional light", eight[2:3], dict(mode="multiply", albedo=False, ambient=(30, 30, 30))),
             ("eight lights", eight, dict(mode="add", ambient=(5, 5, 5))),
             ("eight without a highlight", plain, dict(mode="lighten", opacity=255)),
             ("darken", eight[0:3], dict(mode="darken", ambient=(20, 20, 20))),
             ("difference, albedo", eight[3:6], dict(mode="difference", albedo=True, opacity=128)),
             ("normals", eight[0:2], dict(mode="normal", show_normals=True)))
    changed = 0
    for name, lights, kw in cases:
        p = RC.view_params(W, Hh, **kw)
        want = all_four_forms(s, f, p, list(lights), name)
        changed += int(not np.array_equal(want, f["fb"]))
        same_state(state(s), before)
        drive(s)
    assert changed >= 7, "the cases changed nothing"
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("store_depth", [False, True], ids=["transient", "stored"])
def test_a_depth_left_on_the_chip_is_made_real(small_synthetic, store_depth):
    """Without STORE_DEPTH the frame's depth stays on the chip: the call repeats the depth pass once (k_tile's count) and
    gives the same bytes as with a stored depth; a second call repeats nothing."""
    W, Hh = 257, 33
    s = scene(W, Hh, small_synthetic, "phong", table(W, Hh), store_depth=store_depth, auto_group=False)
    drive(s)
    f = snap(s)
    p, lights = RC.view_params(W, Hh, mode="add"), RC.scene_lights(4)
    want = host(f, p, lights)
    assert not np.array_equal(want, f["fb"])
    drive(s)
    s.profile_enable(True)
    s.relight(p, lights)
    assert s.sync() == 0
    prof = s.profile_read()
    assert prof.get("k_tile", {}).get("launches", 0) == (0 if store_depth else 1), prof
    assert "k_relight" not in prof and s.debug_relight_launches() == 1
    same(s.get_frame_buffer(), want, "in place")
    same(s.get_relit(p, lights), host(dict(f, fb=want), p, lights), "twice")
    assert s.profile_read().get("k_tile", {}).get("launches", 0) == (0 if store_depth else 1)
    s.close()


@pytest.mark.gpu
def test_shortcuts_and_the_launch_counter(small_synthetic):
    W, Hh = 200, 40
    s = scene(W, Hh, small_synthetic, "phong", table(W, Hh))
    p, lights = RC.view_params(W, Hh, mode="normal", ambient=(9, 9, 9)), RC.scene_lights(2)
    s.clear()
    assert not s.get_relit(p, lights).any()
    s.clear()
    out = device_buffer(W * Hh * 3)
    s.relight(p, lights, out=out.data_ptr())
    assert s.sync() == 0 and not out.cpu().numpy().any(), "zeros out of place"
    s.clear()
    s.relight(p, lights)
    assert not s.get_frame_buffer().any()
    drive(s)
    f = snap(s)
    p0 = RC.view_params(W, Hh, mode="normal", opacity=0)
    s.relight(p0, lights)
    same(s.get_frame_buffer(), f["fb"], "opacity 0 in place")
    out = device_buffer(W * Hh * 3)
    s.relight(p0, lights, out=out.data_ptr())
    assert s.sync() == 0
    same(out.cpu().numpy().reshape(Hh, W, 3), f["fb"], "opacity 0 out of place: a copy")
    same(s.get_relit(p0, lights), f["fb"], "opacity 0, getter")
    assert s.debug_relight_launches() == 0, "a shortcut launched the kernel"
    # no lights is no shortcut: the ambient term is blended
    same(s.get_relit(p, ()), host(f, p), "no lights")
    assert s.debug_relight_launches() == 1 and not np.array_equal(host(f, p), f["fb"])
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("pipe", ["phong", "shadow"])
def test_flags_state_and_consumers_after_in_place_calls(small_synthetic, pipe):
    import tiny_renderer_amd as T
    W, Hh = 384, 48
    s = scene(W, Hh, small_synthetic, pipe, RC.table(256, 48), tap=True)
    other = scene(W, Hh, small_synthetic, "phong", TC.SRC_AT)
    drive(s), drive(other, 0.5)
    f, before, flags = snap(s), state(s), clean_flags(s)
    empty = ~tiles_any(RC.bits(f["z"]) != RC.F32_MIN_BITS)
    assert empty.any() and (flags & empty).any() and not (flags & ~empty).any(), "flagged tiles are tiles with nothing drawn"
    lights = RC.scene_lights(3)
    # every mode: tiles with nothing drawn are still flagged, and black behind their flags
    for mode in RC.MODES:
        p = RC.view_params(W, Hh, mode=mode, ambient=(60, 60, 60), albedo=False)
        s.relight(p, lights)
        assert np.array_equal(clean_flags(s), flags), mode
        want = host(f, p, lights)
        assert not np.array_equal(want, f["fb"])
        same(s.get_frame_buffer(), want, mode)
        same_state(state(s), before)
        drive(s)
    # twice in place is the host rule twice; the consumers see the result
    p = RC.view_params(W, Hh, mode="add", ambient=(10, 0, 0))
    once = host(f, p, lights)
    twice = host(dict(f, fb=once), p, lights)
    assert not np.array_equal(once, twice)
    s.relight(p, lights), s.relight(p, lights)
    same(s.get_frame_buffer(), twice, "twice in place")
    same(s.resolve(2), box(twice, 2), "resolve")
    fo = snap(other)
    other.layer_from(s, 0, 0, "screen")
    same(other.get_frame_buffer(), T.layer_host(fo["fb"], twice, 0, 0, "screen"), "layer_from the relit scene")
    assert np.array_equal(clean_flags(s), flags)
    same_state(state(s), before)
    s.close(), other.close()


@pytest.mark.gpu
def test_after_a_backdrop_layer_and_after_grade_in_place(small_synthetic):
    """A WHERE_UNDRAWN backdrop lowers the colour flags of tiles whose z flags stay up; grade in place rewrites the
    colour.  The lights fall on what those calls left, and the backdrop stays where nothing is drawn."""
    import tiny_renderer_amd as T
    W, Hh = 384, 48
    s = scene(W, Hh, small_synthetic, "phong", RC.table(256, 48))
    drive(s)
    f = snap(s)
    undrawn = (RC.bits(f["z"]) == RC.F32_MIN_BITS)[::-1]
    back = T.layer_gradient(W, Hh, (20, 40, 200), (240, 230, 220))
    pin = s.pinned_layer(W, Hh)
    pin[...] = back
    s.layer(pin, where="undrawn")
    assert not clean_flags(s).any(), "the backdrop lowered every colour flag"
    layered = T.layer_host(f["fb"], back, 0, 0, "normal", 256, "undrawn", z=f["z"])
    same(s.get_frame_buffer(), layered, "the backdrop")
    p, lights = RC.view_params(W, Hh, mode="add", ambient=(12, 12, 12)), RC.scene_lights(5)
    want = host(dict(f, fb=layered), p, lights)
    same(s.get_relit(p, lights), want, "over a backdrop, getter")
    s.relight(p, lights)
    same(s.get_frame_buffer(), want, "over a backdrop, in place")
    assert np.array_equal(want[undrawn], layered[undrawn]) and not np.array_equal(want, layered), "the backdrop stays"
    s.set_lut(T.lut_from_function(17, lambda v: 1.0 - v))
    s.grade()
    graded = T.grade_host(want, T.lut_from_function(17, lambda v: 1.0 - v))
    same(s.get_frame_buffer(), graded, "grade in place")
    pm = RC.view_params(W, Hh, mode="multiply", albedo=False, ambient=(128, 128, 128))
    s.relight(pm, lights)
    same(s.get_frame_buffer(), host(dict(f, fb=graded), pm, lights), "after grade in place")
    same(snap(s)["z"], f["z"], "the depth")
    s.close()


@pytest.mark.gpu
def test_a_composited_frame_and_a_kept_frame(small_synthetic):
    import tiny_renderer_amd as T
    W, Hh = 256, 48
    other = T.synthetic_scene(n_lat=9, n_lon=17, tex_size=128, radius=0.75)
    a, b = scene(W, Hh, small_synthetic, "phong", TC.DST_AT), scene(W, Hh, other, "phong", TC.SRC_AT)
    drive(a), drive(b, light=0.2)
    a.composite(b)
    merged = snap(a)
    p, lights = RC.view_params(W, Hh, mode="add"), RC.scene_lights(3)
    want = host(merged, p, lights)
    assert not np.array_equal(want, merged["fb"])
    same(a.get_relit(p, lights), want, "a composited frame, getter")
    a.relight(p, lights)
    same(a.get_frame_buffer(), want, "a composited frame, in place")
    same(snap(a)["z"], merged["z"], "the merged depth")
    a.close(), b.close()
    # a kept frame: the call lights the selected one and leaves the others
    W, Hh, n = 200, 40, 5
    frames = TC._params(n)
    s = scene(W, Hh, small_synthetic, "phong", RC.table(W, Hh), frames_per_launch=4)
    s.render_frames(frames)
    assert s.frames_kept() >= 3
    kept = []
    for back in range(3):
        s.select_frame(back)
        kept.append(snap(s))
    s.select_frame(1)
    lf, la, up = frames[1, 3:6], frames[1, 6:9], frames[1, 9:12]
    st, view = T.prepare_uniforms(2, W, Hh, [float(v) for v in frames[1, 0:3]], [float(v) for v in lf], [float(v) for v in la], [float(v) for v in up])
    assert st == 0
    pk = T.relight_params(view, RC.eye_of(view, lf), mode="add")
    want = host(kept[1], pk, lights)
    assert not np.array_equal(want, kept[1]["fb"])
    same(s.get_relit(pk, lights), want, "a kept frame, getter")
    s.relight(pk, lights)
    same(s.get_frame_buffer(), want, "a kept frame, in place")
    for back in (0, 2):
        s.select_frame(back)
        TC.same(snap(s), kept[back])
    s.close()


@pytest.mark.gpu
def test_refusals_queue_nothing(small_synthetic):
    import tiny_renderer_amd as T
    from tiny_renderer_amd import _lib
    L = T.load_library()
    W, Hh = 256, 48
    s = scene(W, Hh, small_synthetic, "phong", table(W, Hh), tap=True)
    band = scene(W, Hh, small_synthetic, "phong", table(W, Hh), band_rows=(16, 32))
    drive(s), drive(band)
    f, before, flags = snap(s), state(s), clean_flags(s)
    host_out = np.full((Hh, W, 3), 0xAA, np.uint8)
    dev = device_buffer(W * Hh * 3)
    for sc in (s, band):
        sc.profile_enable(True)
    good = RC.view_params(W, Hh, mode="add")
    q = C.addressof(good)
    lights = RC.scene_lights(2)
    tab = (T.Light * 2)(*lights)

    def text():
        return L.tr_last_error().decode()

    def bad_params(**kw):
        p = RC.view_params(W, Hh, mode="add")
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    worse = (T.Light * 2)(*RC.scene_lights(2))
    worse[1].falloff = -1.0
    for who, call in (("tr_scene_relight", lambda sc, pp, t=tab, n=2: L.tr_scene_relight(sc, pp, t, n, None)),
                      ("tr_scene_get_relit", lambda sc, pp, t=tab, n=2: L.tr_scene_get_relit(sc, pp, t, n, host_out.ctypes.data))):
        for kw, why in ((dict(mode=7), ": mode must be TR_LAYER_NORMAL .. TR_LAYER_DIFFERENCE"), (dict(flags=4), ": unknown flags"), (dict(opacity=257), ": opacity must be 0..256")):
            assert call(s._h, C.addressof(bad_params(**kw))) == _lib.TR_E_INVALID and text() == who + why, kw
        assert call(None, q) == _lib.TR_E_INVALID and text() == who + ": null scene"
        assert call(s._h, None) == _lib.TR_E_INVALID and text() == who + ": null argument"
        assert call(s._h, q, t=None) == _lib.TR_E_INVALID and text() == who + ": null argument"
        assert call(s._h, q, n=9) == _lib.TR_E_INVALID and text() == who + ": n_lights must be 0..TR_RELIGHT_MAX_LIGHTS"
        assert call(s._h, q, t=worse) == _lib.TR_E_INVALID and text() == who + ": light 1: falloff must be >= 0"
        assert call(band._h, q) == _lib.TR_E_INVALID
        assert text() == who + ": a band scene (tr_options.band_row0/1) cannot be relit: its border neighbours lie in another rank's rows"
    assert L.tr_scene_get_relit(s._h, q, tab, 2, None) == _lib.TR_E_INVALID and text() == "tr_scene_get_relit: null argument"
    assert L.tr_scene_relight(s._h, q, tab, 2, host_out.ctypes.data) == _lib.TR_E_INVALID
    assert text() == "tr_scene_relight: `out` is neither device memory nor from tr_host_alloc (tr_scene_get_relit takes any host memory)"
    assert L.tr_scene_relight(s._h, q, tab, 2, int(s.band_tiles().frame_buffer_device) + 3) == _lib.TR_E_INVALID
    assert text() == "tr_scene_relight: `out` overlaps a frame buffer of the scene (out == NULL relights in place)"
    assert L.tr_scene_relight(s._h, q, tab, 2, s.pinned_layer(4, 4).ctypes.data) == _lib.TR_E_INVALID
    assert text() == "tr_scene_relight: the host buffer is smaller than the frame"
    # a refusal by the parameters, by the lights and by the scene with `out` in device memory: nothing of it is written
    assert L.tr_scene_relight(s._h, C.addressof(bad_params(opacity=257)), tab, 2, dev.data_ptr()) == _lib.TR_E_INVALID and text() == "tr_scene_relight: opacity must be 0..256"
    assert L.tr_scene_relight(s._h, q, worse, 2, dev.data_ptr()) == _lib.TR_E_INVALID and text() == "tr_scene_relight: light 1: falloff must be >= 0"
    assert L.tr_scene_relight(band._h, q, tab, 2, dev.data_ptr()) == _lib.TR_E_INVALID
    assert L.tr_scene_debug_relight_launches(None) == _lib.TR_E_INVALID and text() == "tr_scene_debug_relight_launches: null scene"
    assert (host_out == 0xAA).all() and (dev.cpu().numpy() == 0x5A).all(), "a refused call wrote `out`"
    assert s.sync() == 0
    for sc in (s, band):
        assert sc.debug_relight_launches() == 0 and not sc.profile_read(), "a refused call queued a kernel"
    assert np.array_equal(clean_flags(s), flags)
    same(s.get_frame_buffer(), f["fb"], "a refused call changed the frame")
    same_state(state(s), before)
    with pytest.raises(ValueError):
        s.relight(RC.IDENTITY, lights)
    with pytest.raises(ValueError):
        s.relight(good, [3])
    s.close(), band.close()


@pytest.mark.gpu
def test_the_cli_lays_lights_in_a_child_process(built, tmp_path):
    """--light-point, --light-spot, --light-dir with --light-ambient and --light-specular write what relight_host gives on
    the plain render; --fog lies over the lights; --show-normals writes the normal map.  Fresh processes."""
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
    st, view = T.prepare_uniforms(2, W, Hh, s._light, *s._camera)
    assert st == 0
    eye = RC.eye_of(view, s._camera[0])
    s.close()
    common = [sys.executable, "-m", "tiny_renderer_amd.cli", "--synthetic", "-s", "phong", "--width", str(W), "--height", str(Hh), "--camera-angle", "0.3",
              "--light-angle", "0.7"]
    lamps = ["--light-point", "1.5,1,2:255,120,40:1.5:0.3", "--light-spot=-1.5,1.5,2.5:0,0,0:60,140,255:8,25:2.5", "--light-dir", "0.3,1,0.4:200,255,200:0.5"]
    runs = {"plain": [], "lit": lamps + ["--light-ambient", "10,10,10", "--light-specular", "0.5,4"],
            "fogged": lamps + ["--light-mode", "screen", "--fog", "200,210,230", "--fog-span", "80,30"], "normals": ["--show-normals", "--light-mode", "normal"]}
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    hd = b"P6\n%d %d\n255\n" % (W, Hh)
    got = {}
    for name, extra in runs.items():
        path = str(tmp_path / (name + ".ppm"))
        done = subprocess.run(common + extra + ["--out", path], capture_output=True, text=True, cwd=REPO, env=env, timeout=120)
        assert done.returncode == 0, done.stdout + done.stderr
        got[name] = np.frombuffer(open(path, "rb").read()[len(hd):], np.uint8).reshape(Hh, W, 3)
    same(got["plain"], f["fb"], "the child's plain render")

    def lights(spec, shin):
        return [T.light_point((1.5, 1, 2), (255, 120, 40), 1.5, 0.3, spec, shin), T.light_spot((-1.5, 1.5, 2.5), (0, 0, 0), 8.0, 25.0, (60, 140, 255), 2.5, 0.0, spec, shin),
                T.light_directional((0.3, 1, 0.4), (200, 255, 200), 0.5, spec, shin)]
    lit = T.relight_host(f["fb"], f["z"], T.relight_params(view, eye, (10, 10, 10), "add"), lights(0.5, 4))
    assert not np.array_equal(lit, f["fb"])
    same(got["lit"], lit, "--light-point --light-spot --light-dir")
    screened = T.relight_host(f["fb"], f["z"], T.relight_params(view, eye, (0, 0, 0), "screen"), lights(0.0, 0))
    fogged = T.ramp_host(screened, f["z"], T.ramp_fog((200, 210, 230)), T.ramp_params(*T.ramp_span(80.0, 30.0, 256)))
    same(got["fogged"], fogged, "--light-mode screen under --fog")
    same(got["normals"], T.relight_host(f["fb"], f["z"], T.relight_params(view, eye, mode="normal", show_normals=True)), "--show-normals")
    bad = subprocess.run(common + ["--light-specular", "0.5,4"], capture_output=True, text=True, cwd=REPO, env=env, timeout=120)
    assert bad.returncode != 0 and "--light" in bad.stderr


@pytest.mark.gpu
def test_light_falls_into_drawn_tiles_behind_raised_colour_flags(small_synthetic):
    """A warp in place whose grid shows nothing but the border (black) stores every tile as zeros without a load and
    raises its colour flag; z is not touched, so flags are up over DRAWN tiles.  In place, a flagged tile into which light
    falls is stored whole (tr_relight_host over zeros) and its flag lowered, a flagged tile none of whose pixels changes
    keeps its flag, and under MULTIPLY and DARKEN every tile stays flagged and black; out of place the flagged tiles
    count as zeros and no flag moves."""
    import tiny_renderer_amd as T
    W, Hh = 384, 48
    s = scene(W, Hh, small_synthetic, "phong", RC.table(256, 48))
    s.set_warp(T.warp_grid_from_function(lambda X, Y: (X + 4.0 * W, Y), W, Hh), W, Hh)
    wp = T.warp_params("border", (0, 0, 0))
    lights = RC.scene_lights(3)

    def black():
        drive(s)
        s.warp(wp)
        assert not s.get_frame_buffer().any()
        return clean_flags(s)

    flags = black()
    f = snap(s)
    drawn_tiles = tiles_any(RC.bits(f["z"]) != RC.F32_MIN_BITS)
    assert flags.all() and drawn_tiles.any() and not drawn_tiles.all(), "the guard: flagged tiles with drawn depth, and empty ones beside them"
    p = RC.view_params(W, Hh, mode="add", albedo=False, ambient=(30, 20, 10))
    want = host(f, p, lights)
    changed = tiles_any((want != 0).any(2)[::-1])
    assert changed.any() and not (changed & ~drawn_tiles).any()
    # out of place: zeros behind the flags, the lights over them; the frame and its flags stay
    same(s.get_relit(p, lights), want, "getter over flagged tiles")
    dev = device_buffer(W * Hh * 3, 0xAB)
    s.relight(p, lights, out=dev.data_ptr())
    assert s.sync() == 0
    same(dev.cpu().numpy().reshape(Hh, W, 3), want, "device memory over flagged tiles")
    assert np.array_equal(clean_flags(s), flags) and not s.get_frame_buffer().any()
    # in place: stored whole where a pixel changes, and only there the flag comes down
    n0 = s.debug_relight_launches()
    s.relight(p, lights)
    same(s.get_frame_buffer(), want, "in place over flagged tiles")
    assert np.array_equal(clean_flags(s), flags & ~changed), "the flags are down exactly where a pixel changed"
    assert s.debug_relight_launches() == n0 + 1
    # ADD with ALBEDO over zeros changes nothing: the vote says no, every flag stays up
    flags = black()
    s.relight(RC.view_params(W, Hh, mode="add", albedo=True, ambient=(30, 20, 10)), lights)
    assert np.array_equal(clean_flags(s), flags) and not s.get_frame_buffer().any(), "albedo over black"
    for mode in ("multiply", "darken"):
        flags = black()
        pm = RC.view_params(W, Hh, mode=mode, albedo=False, ambient=(30, 20, 10))
        same(host(f, pm, lights), f["fb"], mode + " of black is black")
        s.relight(pm, lights)
        assert np.array_equal(clean_flags(s), flags) and not s.get_frame_buffer().any(), mode
        same(s.get_relit(pm, lights), f["fb"], mode + ", getter")
    same(snap(s)["z"], f["z"], "the depth")
    s.close()
