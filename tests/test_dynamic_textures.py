"""Dynamic textures (tr_scene_set_texture / _device / _from_frame): a scene whose image `which` was replaced renders, bit
for bit, what a scene created with that image renders -- colour, z, shadow buffer, winner words, status -- in every
pipeline, with and without a texel set, on the lit path, from host memory, from device memory and from another scene's (or
its own) frame; frames issued before the call keep the old texture without any sync in between."""
import ctypes as C

import numpy as np
import pytest

from tests import helpers as H

pytestmark = pytest.mark.gpu

ALL = ["default", "phong", "normal_map", "specular", "darboux", "shadow", "occlusion"]
TWO_PASS = ("shadow", "occlusion")
SIZES = [(8, 4), (7, 5), (64, 64), (130, 17)]   # (w, h): whole blocks, ragged in both block shapes, whole, ragged + two tiles
W, Hh = 96, 64
CAMS = (0.4, 2.1)


@pytest.fixture(scope="module")
def mesh(built):
    import tiny_renderer_amd as T
    return T.synthetic_scene(n_lat=6, n_lon=12, tex_size=8)[0]


def images(w, h, seed, n=4):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(n)]


def scene(mesh, texs, pipe, w=W, h=Hh, **kw):
    import tiny_renderer_amd as T
    return T.Scene(w, h, mesh, texs, pipe, **kw)


def draw(s, cam, clear=True):
    if clear:
        s.clear()
    s.set_light_direction(H.light(cam - 0.3))
    s.set_camera(*H.camera(cam))
    s.render()


def state(s, pipe, tap=True):
    """Everything a frame is: colour, status, z bits, shadow bits, winner words."""
    fb = s.get_frame_buffer(strict=False)
    out = [fb, np.int64(s.last_status), s.read_z_f32().view(np.uint32)]
    if pipe in TWO_PASS:
        out.append(s.read_shadow_f32().view(np.uint32))
    if tap:
        out.append(s.read_winner_u32())
    return out


def same(a, b):
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x, y), "part %d differs at %d places" % (k, int((np.asarray(x) != np.asarray(y)).sum()))


def frames_of(s, pipe, tap=True):
    out = []
    for cam in CAMS:
        draw(s, cam)
        out += state(s, pipe, tap)
    return out


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("pipe", ALL)
def test_set_texture_equals_a_scene_created_with_the_image(mesh, pipe, size):
    import tiny_renderer_amd as T
    w, h = size
    texs = images(w, h, 100 + w)
    for which in range(4):
        img = images(w, h, 200 + which, 1)[0]
        b = scene(mesh, texs, pipe, winner_tap=True)
        draw(b, 1.0)                      # (a frame with the old texture first: the arrays have been read)
        b.set_texture(which, img)
        new = list(texs)
        new[which] = img
        b2 = scene(mesh, new, pipe, winner_tap=True)
        same(frames_of(b, pipe), frames_of(b2, pipe))
        want, _ = T.texel_set_host(pipe, new)
        assert want.size and np.array_equal(b.debug_texel_set(), want) and np.array_equal(b2.debug_texel_set(), want)
        assert np.array_equal(b.read_texture(which), img)
        for k in range(4):
            assert np.array_equal(b.read_texture(k), new[k])
        b.close()
        b2.close()


@pytest.mark.parametrize("pipe", ["phong", "specular", "darboux", "occlusion"])
def test_images_of_different_sizes_take_the_plain_arrays(mesh, pipe):
    texs = [images(9, 7, 1, 1)[0], images(8, 4, 2, 1)[0], images(8, 4, 3, 1)[0], images(5, 6, 4, 1)[0]]
    for which in range(4):
        hh, ww = texs[which].shape[:2]
        img = images(ww, hh, 300 + which, 1)[0]
        b = scene(mesh, texs, pipe, winner_tap=True)
        draw(b, 1.0)
        b.set_texture(which, img)
        new = list(texs)
        new[which] = img
        b2 = scene(mesh, new, pipe, winner_tap=True)
        same(frames_of(b, pipe), frames_of(b2, pipe))
        assert b.debug_texel_set().size == 0 and b2.debug_texel_set().size == 0
        assert np.array_equal(b.read_texture(which), img)
        b.close()
        b2.close()


@pytest.mark.parametrize("pipe", ["normal_map", "specular"])
def test_lit_path_sees_the_new_images(mesh, pipe, monkeypatch):
    """k_lit shades the texel set once per texel and frame: the set it reads must be the new one from the next frame on."""
    monkeypatch.setenv("TR_LIT", "1")
    texs = images(64, 64, 11)
    for tap in (True, False):
        b = scene(mesh, texs, pipe, winner_tap=tap)
        b.profile_enable(True)
        draw(b, CAMS[0])
        first = state(b, pipe, tap)
        new = list(texs)
        for which in (0, 1, 3):
            new[which] = images(64, 64, 400 + which, 1)[0]
            b.set_texture(which, new[which])
        draw(b, CAMS[1])
        second = state(b, pipe, tap)
        assert b.profile_read()["k_lit"]["launches"] >= 2
        assert b.profile_read()["k_pack_texels"]["launches"] == 3
        old = scene(mesh, texs, pipe, winner_tap=tap)
        draw(old, CAMS[0])
        same(first, state(old, pipe, tap))
        b2 = scene(mesh, new, pipe, winner_tap=tap)
        draw(b2, CAMS[1])
        same(second, state(b2, pipe, tap))
        for s in (b, old, b2):
            s.close()


# --- from a frame -------------------------------------------------------------------------------

def _src_plain(mesh):
    s = scene(mesh, images(16, 16, 21), "phong", 64, 64)
    draw(s, 0.7)
    return s, []


def _src_flagged_over_drawn(mesh):
    """camera 1 fills the frame's tiles; after a clear, camera 2 looks past the model: empty tiles over drawn memory"""
    s = scene(mesh, images(16, 16, 22), "phong", 64, 64)
    draw(s, 0.7)
    s.sync()
    s.clear()
    s.set_light_direction(H.light(0.2))
    s.set_camera([0.0, 0.0, 1.0], [0.0, 1.1, 0.0], [0.0, 1.0, 0.0])
    s.render()
    return s, []


def _src_cleared(mesh):
    s = scene(mesh, images(16, 16, 23), "phong", 64, 64)
    draw(s, 0.7)
    s.clear()
    return s, []


def _src_kept_frame(mesh):
    s = scene(mesh, images(16, 16, 24), "phong", 64, 64, frames_per_launch=4)
    p = np.zeros((6, 12), np.float32)
    for i in range(6):
        p[i, 0:3] = H.light(0.3 * i)
        p[i, 3:6], p[i, 6:9], p[i, 9:12] = H.camera(0.5 * i)
    s.render_frames(p)
    s.select_frame(2)
    return s, []


def _src_callers_buffer(mesh):
    import torch
    buf = torch.zeros(64 * 64 * 3, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    s = scene(mesh, images(16, 16, 25), "phong", 64, 64)
    s.set_frame_buffer_device(buf.data_ptr())
    draw(s, 0.9)
    return s, [buf]


def _src_composited(mesh):
    s = scene(mesh, images(16, 16, 26), "phong", 64, 64, store_depth=True)
    o = scene(mesh, images(16, 16, 27), "default", 64, 64, store_depth=True, instances=np.array([[0.3, 0.1, 0.2, 0.6]], np.float32))
    draw(s, 0.7)
    draw(o, 0.7)
    s.composite(o)
    return s, [o]


def _src_blurred(mesh):
    import tiny_renderer_amd as T
    s = scene(mesh, images(16, 16, 28), "phong", 64, 64)
    draw(s, 0.7)
    s.depth_of_field(T.dof_params(focus=0.0, scale=0.05, max_radius=3, background_radius=1))
    return s, []


SOURCES = {"plain": _src_plain, "flagged_over_drawn": _src_flagged_over_drawn, "cleared": _src_cleared, "kept_frame": _src_kept_frame,
           "callers_buffer": _src_callers_buffer, "composited": _src_composited, "blurred": _src_blurred}


@pytest.mark.parametrize("source", sorted(SOURCES))
@pytest.mark.parametrize("pipe,which", [("phong", 0), ("normal_map", 1)])
def test_texture_from_a_frame(mesh, pipe, which, source):
    src, keep = SOURCES[source](mesh)
    texs = images(64, 64, 31)
    dst = scene(mesh, texs, pipe, winner_tap=True)
    draw(dst, 1.0)
    dst.set_texture_from(src, which)          # (no sync: ordered behind src's frame on the device)
    got = frames_of(dst, pipe)
    img = src.get_frame_buffer()
    if source == "cleared":
        assert not img.any()
    else:
        assert img.any()
    if source == "flagged_over_drawn":
        assert any(not img[16 * k:16 * k + 16].any() for k in range(4))   # (an empty tile row, which camera 1 had drawn into)
    assert np.array_equal(dst.read_texture(which), img)
    new = list(texs)
    new[which] = img
    ref = scene(mesh, new, pipe, winner_tap=True)
    same(got, frames_of(ref, pipe))
    for s in [dst, ref, src] + [k for k in keep if hasattr(k, "close")]:
        s.close()


def test_texture_from_a_narrow_frame_with_partial_tiles(mesh):
    src = scene(mesh, images(16, 16, 41), "phong", 130, 17)
    draw(src, 0.5)
    for pipe, which in (("default", 0), ("darboux", 2), ("specular", 3)):
        texs = images(130, 17, 42)
        dst = scene(mesh, texs, pipe, winner_tap=True)
        dst.set_texture_from(src, which)
        got = frames_of(dst, pipe)
        img = src.get_frame_buffer()
        assert img.any()
        new = list(texs)
        new[which] = img
        ref = scene(mesh, new, pipe, winner_tap=True)
        same(got, frames_of(ref, pipe))
        dst.close()
        ref.close()
    src.close()


def test_feedback_of_a_scenes_own_frame(mesh):
    """src == dst: the last frame becomes the texture of the next, three rounds, against the host loop that reads the
    frame back and builds a new scene each round."""
    texs = images(64, 64, 51)
    s = scene(mesh, texs, "phong", 64, 64)
    cur = list(texs)
    for cam in (3.1, 3.3, 3.0):   # (the side of the model whose uv meet the middle of the image: the picture stays alive)
        draw(s, cam)
        s.set_texture_from(s, 0)
        ref = scene(mesh, cur, "phong", 64, 64)
        draw(ref, cam)
        img = ref.get_frame_buffer()
        assert img.any()
        assert np.array_equal(s.get_frame_buffer(), img)
        assert np.array_equal(s.read_texture(0), img)
        cur[0] = img
        ref.close()
    s.close()


def test_texture_from_device_memory_behind_its_producer(mesh):
    import torch
    src = scene(mesh, images(16, 16, 61), "phong", 128, 128)
    draw(src, 0.8)
    buf = torch.zeros(64 * 64 * 3, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    src.resolve_into(2, buf.data_ptr())
    texs = images(64, 64, 62)
    dst = scene(mesh, texs, "specular", winner_tap=True)
    draw(dst, 1.0)
    dst.set_texture_device(0, buf.data_ptr(), 64, 64, producer=src)
    got = frames_of(dst, "specular")
    img = src.resolve(2)
    assert img.any() and np.array_equal(dst.read_texture(0), img)
    new = [img] + texs[1:]
    ref = scene(mesh, new, "specular", winner_tap=True)
    same(got, frames_of(ref, "specular"))
    for s in (dst, ref, src):
        s.close()


# --- ordering without a sync in between ---------------------------------------------------------

def _old_new(mesh, pipe, texs, img, cams, **kw):
    """The frames at `cams` of a scene with the old images and of one with image 0 replaced."""
    out = []
    for t in (texs, [img] + texs[1:]):
        s = scene(mesh, t, pipe, **kw)
        fr = []
        for cam in cams:
            draw(s, cam)
            fr.append(s.get_frame_buffer())
        s.close()
        out.append(fr)
    return out


def test_queued_read_back_keeps_the_old_texture(mesh):
    texs, img = images(64, 64, 71), images(64, 64, 72, 1)[0]
    old, new = _old_new(mesh, "phong", texs, img, CAMS)
    s = scene(mesh, texs, "phong")
    p1, p2 = s.pinned_frame(), s.pinned_frame()
    draw(s, CAMS[0])
    s.get_frame_buffer_async(p1)
    s.set_texture(0, img)
    draw(s, CAMS[1])
    s.get_frame_buffer_async(p2)
    s.sync()
    assert np.array_equal(p1, old[0]) and np.array_equal(p2, new[1])
    assert not np.array_equal(old[1], new[1])
    s.close()


def test_a_frame_held_back_keeps_the_old_texture(mesh):
    texs, img = images(64, 64, 73), images(64, 64, 74, 1)[0]
    old, new = _old_new(mesh, "phong", texs, img, CAMS)
    s = scene(mesh, texs, "phong")
    assert s.frames_per_launch > 1           # (auto-grouping holds cleared frames back on the library's stream)
    draw(s, CAMS[0])                          # held back on the host
    s.set_texture(0, img)                     # submits it first
    assert np.array_equal(s.get_frame_buffer(), old[0])
    draw(s, CAMS[1])
    assert np.array_equal(s.get_frame_buffer(), new[1])
    s.close()


def test_kept_frames_stay_and_the_next_call_draws_the_new_texture(mesh):
    texs, img = images(64, 64, 75), images(64, 64, 76, 1)[0]
    cams = [0.4 * i for i in range(6)]
    p = np.zeros((6, 12), np.float32)
    for i, cam in enumerate(cams):
        p[i, 0:3] = H.light(cam - 0.3)
        p[i, 3:6], p[i, 6:9], p[i, 9:12] = H.camera(cam)
    old, new = _old_new(mesh, "normal_map", texs, img, cams, auto_group=False)
    s = scene(mesh, texs, "normal_map", frames_per_launch=4)
    s.render_frames(p)
    s.set_texture(0, img)
    s.select_frame(2)
    assert np.array_equal(s.get_frame_buffer(), old[5 - 2])
    s.render_frames(p)
    for back in range(s.frames_kept()):
        s.select_frame(back)
        assert np.array_equal(s.get_frame_buffer(), new[5 - back])
    assert not np.array_equal(old[5], new[5])
    s.close()


def test_split_passes_draw_the_new_texture(mesh):
    texs, img = images(64, 64, 77), images(64, 64, 78, 1)[0]
    _, new = _old_new(mesh, "shadow", texs, img, CAMS[:1])
    s = scene(mesh, texs, "shadow")
    draw(s, 1.3)
    s.set_texture(0, img)
    s.clear()
    s.set_light_direction(H.light(CAMS[0] - 0.3))
    s.set_camera(*H.camera(CAMS[0]))
    s.render_shadow_pass()
    s.render_colour_pass()
    assert np.array_equal(s.get_frame_buffer(), new[0])
    s.close()


# --- errors ------------------------------------------------------------------------------------

def test_invalid_calls_change_nothing(mesh):
    import torch
    import tiny_renderer_amd as T
    from tiny_renderer_amd import _lib
    L = T.load_library()
    texs = images(64, 64, 81)
    s = scene(mesh, texs, "specular", winner_tap=True)
    ref = scene(mesh, texs, "specular", winner_tap=True)
    want = frames_of(ref, "specular")
    good = np.ascontiguousarray(images(64, 64, 82, 1)[0])
    small = np.ascontiguousarray(images(32, 64, 83, 1)[0])
    dev = torch.zeros(64 * 64 * 3, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    band = scene(mesh, images(16, 16, 84), "phong", 64, 64, band_rows=(0, 32))
    other = scene(mesh, images(16, 16, 85), "phong", 32, 64)
    draw(band, 0.3)
    draw(other, 0.3)

    def img(a):
        return _lib.ImageRgb8(a.ctypes.data_as(C.POINTER(C.c_uint8)), a.shape[1], a.shape[0])

    calls = [
        lambda: L.tr_scene_set_texture(None, 0, C.byref(img(good))),
        lambda: L.tr_scene_set_texture(s._h, 0, None),
        lambda: L.tr_scene_set_texture(s._h, 0, C.byref(_lib.ImageRgb8(None, 64, 64))),
        lambda: L.tr_scene_set_texture(s._h, 4, C.byref(img(good))),
        lambda: L.tr_scene_set_texture(s._h, 0, C.byref(img(small))),
        lambda: L.tr_scene_set_texture_device(None, 0, dev.data_ptr(), 64, 64, None),
        lambda: L.tr_scene_set_texture_device(s._h, 0, None, 64, 64, None),
        lambda: L.tr_scene_set_texture_device(s._h, 4, dev.data_ptr(), 64, 64, None),
        lambda: L.tr_scene_set_texture_device(s._h, 0, dev.data_ptr(), 32, 64, None),
        lambda: L.tr_scene_set_texture_device(s._h, 0, good.ctypes.data, 64, 64, None),    # ordinary host memory
        lambda: L.tr_scene_set_texture_from_frame(None, 0, ref._h),
        lambda: L.tr_scene_set_texture_from_frame(s._h, 0, None),
        lambda: L.tr_scene_set_texture_from_frame(s._h, 4, ref._h),
        lambda: L.tr_scene_set_texture_from_frame(s._h, 0, ref._h),     # a 96 x 64 frame for a 64 x 64 texture
        lambda: L.tr_scene_set_texture_from_frame(s._h, 0, other._h),   # 32 x 64
        lambda: L.tr_scene_set_texture_from_frame(s._h, 0, band._h),    # a band scene
    ]
    if torch.cuda.device_count() > 1:
        far = scene(mesh, images(16, 16, 86), "phong", 64, 64, device=1)
        calls.append(lambda: L.tr_scene_set_texture_from_frame(s._h, 0, far._h))
        calls.append(lambda: L.tr_scene_set_texture_device(s._h, 0, dev.data_ptr(), 64, 64, far._h))
    for k, call in enumerate(calls):
        assert call() == _lib.TR_E_INVALID, "call %d" % k
        assert L.tr_last_error(), "call %d left no text" % k
        same(frames_of(s, "specular"), want)
    with pytest.raises(ValueError):
        s.set_texture(7, good)
    with pytest.raises(ValueError):
        s.set_texture(0, small)
    assert L.tr_scene_read_texture(s._h, 4, good.ctypes.data) == _lib.TR_E_INVALID
    assert L.tr_scene_debug_texel_set(s._h, good.ctypes.data, 3) == _lib.TR_E_INVALID
    for k in range(4):
        assert np.array_equal(s.read_texture(k), texs[k])
    for x in (s, ref, band, other) + ((far,) if torch.cuda.device_count() > 1 else ()):
        x.close()
