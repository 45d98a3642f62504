"""The protocol the draw entry points share behind the C ABI -- tr_scene_render_frames and its instanced, transformed,
morphed and skinned forms, and the setters of tables, targets, weights, skin, palette and lookup table: which refusal is
reported and in which words, that a refusal leaves the scene as it was, and that every place where the library renders a
frame again on its own (a depth-only repeat, a frame held back, a group, a replay after a bin overflow) draws that frame
under the state it was issued in and leaves the state the caller has set since alone.

Every expected text below is the library's own, character for character; the features' own test files match them by a
word only.  What a table, a pose or a palette draws is the business of those files: here the expectation is always a
second scene that was only ever given the state in question, compared with np.array_equal.
Frames are 256 x 48 (2 x 3 whole tiles) and 200 x 40 (partial tiles).

A state is a view (light and camera), a transform table of two entries and, where the case says so, a morph pose of two
targets or a palette of two bones; A is the state a frame is issued in, B the one the caller sets afterwards.

One case reads differently from its first description: a clear() followed by get_frame_buffer() returns the cleared
frame (the reference's semantics: the getter makes the clear real), so the frame that was held back is read from the
frame buffer's device memory after a sync(), which renders it and leaves the clear pending."""
import ctypes as C

import numpy as np
import pytest

from tests import helpers as H

PIPE = "phong"
SIZES = [(256, 48), (200, 40)]
KINDS = ("table", "pose", "palette")     # what a state holds beside its view and table

NULL_ARG = b"null argument"
NULL_SCENE = b"null scene"
NULL_FB = b"null frame buffer in the list"
NULL_TABLE = b"null instance table"
TOO_MANY = b"too many polygons (mesh polygons x instances)"
TABLES_TOO_LARGE = b"instance tables too large"
N_WEIGHTS = b"n_weights must be 0 or the scene's number of morph targets"
NULL_WEIGHTS = b"null weights"
N_BONES = b"n_bones must be 0 or the bone count of the scene's skin"
NULL_PALETTE = b"null palette"
NULL_PALETTES = b"null palettes"
MANY_TARGETS = b"more than TR_MORPH_MAX_TARGETS morph targets"
NULL_DELTA = b"null delta array"
MANY_BONES = b"more than TR_SKIN_MAX_BONES bones"
NULL_INFLUENCE = b"null influence array"
BONE_BEYOND = b"bone index beyond n_bones"
LUT_NULL_SCENE = b"tr_scene_set_lut: null scene"
LUT_EDGE = b"tr_scene_set_lut: the table's edge n must be 2..TR_GRADE_MAX_N"
LUT_NULL_TABLE = b"tr_scene_set_lut: null table"


def lib():
    import tiny_renderer_amd as T
    return T.load_library()


def view(cam, light):
    return np.concatenate([np.asarray(H.light(light), np.float32)] + [np.asarray(v, np.float32) for v in H.camera(cam)])


def table(yaw, dx):
    import tiny_renderer_amd as T
    return T.rotation_instances([yaw, -2.0 * yaw], [0.2, -0.3], [0.0, 0.5], [[-0.35 + dx, 0.05, 0.0], [0.3 + dx, -0.1, 0.1]], [0.6, 0.45])


def palette(turn):
    import tiny_renderer_amd as T
    return T.rotation_instances([turn, -turn], [0.1, 0.3 * turn], [0.0, 0.2], [[0.0, 0.0, 0.0], [0.05, 0.1 * turn, 0.0]], [1.0, 0.8])


VIEWS = {"A": view(0.3, 0.7), "B": view(1.4, -0.5), "C0": view(-0.6, 0.2), "C1": view(0.1, 1.1), "C2": view(0.9, 0.4)}
TABLES = {"A": lambda: table(0.4, 0.0), "B": lambda: table(-0.9, 0.1), "C0": lambda: table(0.2, -0.1), "C1": lambda: table(1.3, 0.05),
          "C2": lambda: table(-0.4, 0.0)}
POSES = {"A": np.array([0.9, 0.3], np.float32), "B": np.array([-0.25, 1.0], np.float32), "C0": np.array([0.5, 0.5], np.float32),
         "C1": np.array([0.0, 1.2], np.float32), "C2": np.array([1.1, -0.4], np.float32)}
PALETTES = {"A": lambda: palette(0.5), "B": lambda: palette(-0.8)}
CALL = ("C0", "C1", "C2")                # the three frames of a render_frames call


def targets(mesh):
    """Two morph targets: an inflation and a squash in y with normals of its own."""
    pos = np.asarray(mesh["pos"], np.float32).reshape(-1, 3)
    nrm = np.asarray(mesh["nrm"], np.float32).reshape(-1, 3)
    dp, dn = np.zeros((2,) + pos.shape, np.float32), np.zeros((2,) + nrm.shape, np.float32)
    dp[0] = pos * np.float32(0.2)
    dp[1, :, 1] = np.float32(-0.35) * pos[:, 1]
    dn[1, :, 1] = np.float32(0.3) * nrm[:, 1]
    return dp, dn


def rig(mesh):
    """Two bones: the upper half follows bone 1, the lower half bone 0, a belt both."""
    y = np.asarray(mesh["pos"], np.float32).reshape(-1, 3)[:, 1]
    bones = np.zeros((y.shape[0], 4), np.uint32)
    weights = np.zeros((y.shape[0], 4), np.float32)
    bones[:, 1] = 1
    weights[:, 0] = np.clip(0.5 - 2.0 * y, 0.0, 1.0)
    weights[:, 1] = np.float32(1.0) - weights[:, 0]
    return bones, weights


def make(ms, W, Hh, kind, **kw):
    """A scene that can be given the states of `kind`."""
    import tiny_renderer_amd as T
    s = T.Scene(W, Hh, ms[0], ms[1], PIPE, **kw)
    if kind == "pose":
        s.set_morph_targets(*targets(ms[0]))
    if kind == "palette":
        s.set_skin(*rig(ms[0]), n_bones=2)
    return s


def give(s, kind, v, t=None, p=None):
    """Sets view v, table t and pose / palette p (names; p defaults to t, t to v) without rendering."""
    t = v if t is None else t
    p = t if p is None else p
    q = VIEWS[v]
    s.set_light_direction(q[0:3])
    s.set_camera(q[3:6], q[6:9], q[9:12])
    s.set_instance_transforms(TABLES[t]())
    if kind == "pose":
        s.set_morph_weights(POSES[p])
    if kind == "palette":
        s.set_bone_palette(PALETTES[p]())


def frame(s):
    s.clear()
    s.render()
    return s.get_frame_buffer()


def bits(z):
    return np.ascontiguousarray(z, np.float32).view(np.uint32)


_only = {}


def only(ms, W, Hh, kind, v, t=None, p=None, twice=False):
    """(frame, z bits) of a scene that stores its depth and was only ever given this state; twice: rendered a second
    time without a clear.  Computed once per state and shared."""
    key = (W, Hh, kind, v, t, p, twice)
    if key not in _only:
        s = make(ms, W, Hh, kind, store_depth=True, auto_group=False)
        give(s, kind, v, t, p)
        s.clear()
        s.render()
        if twice:
            s.render()
        fb, z = s.get_frame_buffer(), bits(s.read_z_f32())
        s.close()
        assert fb.any()
        fb.setflags(write=False), z.setflags(write=False)
        _only[key] = (fb, z)
    return _only[key]


def device_frame(s):
    """The current frame buffer's device memory as it is now: no getter, so a pending clear stays pending."""
    import torch
    assert s.sync() == 0
    n = s.width * s.height * 3

    class Bytes:
        __cuda_array_interface__ = {"shape": (n,), "typestr": "|u1", "data": (int(s.frame_buffer_device()), False), "version": 2}

    return torch.as_tensor(Bytes(), device="cuda").cpu().numpy().reshape(s.height, s.width, 3)


def test_states_differ():
    """(no GPU) the names stand for different values, or the state tests below would compare a thing with itself"""
    for d in (VIEWS, {k: f() for k, f in TABLES.items()}, POSES, {k: f() for k, f in PALETTES.items()}):
        keys = sorted(d)
        for i, a in enumerate(keys):
            for b in keys[i + 1:]:
                assert not np.array_equal(d[a], d[b]), (a, b)


# ------------------------------------------------------------------------------------------------------------------
# Refusals
# ------------------------------------------------------------------------------------------------------------------

def frames_arg(n=2):
    return np.ascontiguousarray(np.stack([VIEWS[k] for k in ("C0", "C1", "C2")[:n]]), np.float32)


def expect(code, text):
    from tiny_renderer_amd import _lib
    got = lib().tr_last_error()
    assert code == _lib.TR_E_INVALID and got == text, (code, got, text)


def test_null_scene_texts(built):
    L = lib()
    f = frames_arg()
    x = np.zeros(64, np.float32)
    fp, xp = f.ctypes.data, x.ctypes.data
    expect(L.tr_scene_render_frames(None, 2, fp, None), NULL_ARG)
    expect(L.tr_scene_render_frames(None, 0, None, None), NULL_ARG)           # ... before the n_frames == 0 shortcut
    for fn in (L.tr_scene_render_frames_instanced, L.tr_scene_render_frames_transformed, L.tr_scene_render_frames_morphed,
               L.tr_scene_render_frames_skinned):
        expect(fn(None, 2, fp, 1, xp, None), NULL_ARG)
        expect(fn(None, 0, None, 1, None, None), NULL_ARG)                    # ... before the call's own checks
    for fn in (L.tr_scene_set_instances, L.tr_scene_set_instance_transforms, L.tr_scene_set_morph_weights, L.tr_scene_set_bone_palette):
        expect(fn(None, 1, xp), NULL_SCENE)
        expect(fn(None, 1, None), NULL_SCENE)
    expect(L.tr_scene_set_morph_targets(None, 1, xp, xp), NULL_SCENE)
    expect(L.tr_scene_set_morph_targets(None, 65, None, None), NULL_SCENE)
    expect(L.tr_scene_set_skin(None, 1, xp, xp), NULL_SCENE)
    expect(L.tr_scene_set_skin(None, 129, None, None), NULL_SCENE)
    expect(L.tr_scene_set_lut(None, 2, xp), LUT_NULL_SCENE)
    expect(L.tr_scene_set_lut(None, 1, None), LUT_NULL_SCENE)


class Refusals:
    """A scene under state A with targets, a skin and a lookup table; every refusal is followed by a look at the scene."""

    def __init__(self, ms, W, Hh):
        from tests.test_stage_entry_points import random_lut
        self.s = s = make(ms, W, Hh, "pose")
        s.set_skin(*rig(ms[0]), n_bones=2)
        s.set_lut(random_lut(5, W))
        give(s, "pose", "A")
        s.set_bone_palette(PALETTES["A"]())
        self.fb = frame(s)
        self.graded = s.get_graded()
        self.rows = s.debug_morph_rows()
        assert self.fb.any() and self.rows >= 1 and not np.array_equal(self.graded, self.fb)

    def unchanged(self):
        s = self.s
        assert np.array_equal(frame(s), self.fb), "the scene draws another frame after the call"
        assert s.debug_morph_rows() == self.rows
        assert (s.n_morph_targets, s.n_bones) == (2, 2)

    def refused(self, code, text):
        expect(code, text)
        self.unchanged()

    def accepted(self, code):
        assert code == 0, (code, lib().tr_last_error())
        self.unchanged()


@pytest.mark.gpu
@pytest.mark.parametrize("W,Hh", SIZES)
def test_render_frames_refusals(small_synthetic, W, Hh):
    L = lib()
    r = Refusals(small_synthetic, W, Hh)
    h = r.s._h
    f = frames_arg()
    fp = f.ctypes.data
    bad_list = (C.c_void_p * 2)(int(r.s.frame_buffer_device()), None)
    x = np.zeros(2 * 2 * 24, np.float32)           # two frames' worth of anything
    xp = x.ctypes.data
    # tables that pass the polygon limit one by one and exceed 2^32 entries together
    n_tri = np.asarray(small_synthetic[0]["idx"]).reshape(-1, 9).shape[0]
    big_n = 0xFFFFFFEF // n_tri
    many = 0xFFFFFFFF // big_n + 1
    assert n_tri * big_n < 0xFFFFFFF0 and many * big_n > 0xFFFFFFFF and many < 4096
    many_f = np.ascontiguousarray(np.tile(VIEWS["C0"], (many, 1)), np.float32)
    many_list = (C.c_void_p * many)(*([int(r.s.frame_buffer_device()), None] * many)[:many])

    # --- tr_scene_render_frames
    r.refused(L.tr_scene_render_frames(h, 2, None, None), NULL_ARG)
    r.refused(L.tr_scene_render_frames(h, 2, None, bad_list), NULL_ARG)          # null frames and a null entry: the frames
    r.refused(L.tr_scene_render_frames(h, 2, fp, bad_list), NULL_FB)
    r.accepted(L.tr_scene_render_frames(h, 0, fp, bad_list))                     # the shortcut comes before the scan
    r.accepted(L.tr_scene_render_frames(h, 0, None, bad_list))

    # --- the table calls
    for fn in (L.tr_scene_render_frames_instanced, L.tr_scene_render_frames_transformed):
        r.refused(fn(h, 2, None, 2, xp, None), NULL_ARG)
        r.refused(fn(h, 2, None, 2, None, bad_list), NULL_ARG)                   # null frames first
        r.refused(fn(h, 2, fp, 2, None, None), NULL_TABLE)
        r.refused(fn(h, 2, fp, 2, None, bad_list), NULL_TABLE)                   # the table before the list
        r.refused(fn(h, 0, fp, 2, None, None), NULL_TABLE)                       # ... and before the shortcut
        r.refused(fn(h, 0, None, 2, None, bad_list), NULL_TABLE)
        r.refused(fn(h, 2, fp, 0xFFFFFFFF, xp, None), TOO_MANY)                  # (refused before the table is read)
        r.refused(fn(h, 0, fp, 0xFFFFFFFF, xp, bad_list), TOO_MANY)
        r.refused(fn(h, 2, fp, 0xFFFFFFFF, None, None), NULL_TABLE)              # null table and too many: the table
        r.refused(fn(h, many, many_f.ctypes.data, big_n, xp, many_list), TABLES_TOO_LARGE)   # (before the table is read, and) before the list
        r.accepted(fn(h, 0, many_f.ctypes.data, big_n, xp, many_list))           # ... and after the shortcut
        r.refused(fn(h, 2, fp, 2, xp, bad_list), NULL_FB)
        r.accepted(fn(h, 0, fp, 2, xp, bad_list))
        r.accepted(fn(h, 0, None, 0, None, bad_list))

    # --- the posed calls
    for fn, count, null_v in ((L.tr_scene_render_frames_morphed, N_WEIGHTS, NULL_WEIGHTS),
                              (L.tr_scene_render_frames_skinned, N_BONES, NULL_PALETTES)):
        r.refused(fn(h, 2, None, 2, xp, None), NULL_ARG)
        r.refused(fn(h, 2, None, 3, None, bad_list), NULL_ARG)                   # null frames first
        r.refused(fn(h, 2, fp, 3, xp, None), count)
        r.refused(fn(h, 2, fp, 1, xp, None), count)
        r.refused(fn(h, 2, fp, 3, None, bad_list), count)                        # the count before the vectors and the list
        r.refused(fn(h, 0, fp, 3, xp, None), count)                              # ... and before the shortcut
        r.refused(fn(h, 0, None, 3, None, bad_list), count)
        r.refused(fn(h, 2, fp, 2, None, None), null_v)
        r.refused(fn(h, 2, fp, 2, None, bad_list), null_v)                       # the vectors before the list
        r.accepted(fn(h, 0, fp, 2, None, bad_list))                              # no frames: no vectors needed
        r.refused(fn(h, 2, fp, 2, xp, bad_list), NULL_FB)
        r.refused(fn(h, 2, fp, 0, None, bad_list), NULL_FB)
        r.accepted(fn(h, 0, fp, 2, xp, bad_list))
        r.accepted(fn(h, 0, None, 0, None, bad_list))
    r.s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("W,Hh", SIZES)
def test_setter_refusals(small_synthetic, W, Hh):
    from tiny_renderer_amd import _lib
    L = lib()
    r = Refusals(small_synthetic, W, Hh)
    h = r.s._h
    mesh = small_synthetic[0]
    x = np.zeros(2 * 24, np.float32)
    xp = x.ctypes.data

    for fn in (L.tr_scene_set_instances, L.tr_scene_set_instance_transforms):
        r.refused(fn(h, 2, None), NULL_TABLE)
        r.refused(fn(h, 0xFFFFFFFF, None), NULL_TABLE)                           # null table and too many: the table
        r.refused(fn(h, 0xFFFFFFFF, xp), TOO_MANY)                               # (refused before the table is read)

    r.refused(L.tr_scene_set_morph_weights(h, 3, xp), N_WEIGHTS)
    r.refused(L.tr_scene_set_morph_weights(h, 1, None), N_WEIGHTS)               # the count before the pointer
    r.refused(L.tr_scene_set_morph_weights(h, 2, None), NULL_WEIGHTS)
    r.refused(L.tr_scene_set_bone_palette(h, 3, xp), N_BONES)
    r.refused(L.tr_scene_set_bone_palette(h, 1, None), N_BONES)
    r.refused(L.tr_scene_set_bone_palette(h, 2, None), NULL_PALETTE)

    dp, dn = targets(mesh)
    many = _lib.TR_MORPH_MAX_TARGETS + 1
    r.refused(L.tr_scene_set_morph_targets(h, many, dp.ctypes.data, dn.ctypes.data), MANY_TARGETS)   # (refused before they are read)
    r.refused(L.tr_scene_set_morph_targets(h, many, None, None), MANY_TARGETS)   # too many and null: the number
    r.refused(L.tr_scene_set_morph_targets(h, 2, None, dn.ctypes.data), NULL_DELTA)
    r.refused(L.tr_scene_set_morph_targets(h, 2, dp.ctypes.data, None), NULL_DELTA)

    bones, weights = rig(mesh)
    beyond = bones.copy()
    beyond[-1, 3] = 2
    many = _lib.TR_SKIN_MAX_BONES + 1
    r.refused(L.tr_scene_set_skin(h, many, bones.ctypes.data, weights.ctypes.data), MANY_BONES)
    r.refused(L.tr_scene_set_skin(h, many, None, None), MANY_BONES)              # too many and null: the number
    r.refused(L.tr_scene_set_skin(h, 2, None, weights.ctypes.data), NULL_INFLUENCE)
    r.refused(L.tr_scene_set_skin(h, 2, bones.ctypes.data, None), NULL_INFLUENCE)
    r.refused(L.tr_scene_set_skin(h, 2, beyond.ctypes.data, None), NULL_INFLUENCE)   # null before the indices are read
    r.refused(L.tr_scene_set_skin(h, 2, beyond.ctypes.data, weights.ctypes.data), BONE_BEYOND)
    r.refused(L.tr_scene_set_skin(h, 1, bones.ctypes.data, weights.ctypes.data), BONE_BEYOND)

    r.refused(L.tr_scene_set_lut(h, 1, xp), LUT_EDGE)
    r.refused(L.tr_scene_set_lut(h, 34, xp), LUT_EDGE)
    r.refused(L.tr_scene_set_lut(h, 1, None), LUT_EDGE)                          # the edge before the pointer
    r.refused(L.tr_scene_set_lut(h, 5, None), LUT_NULL_TABLE)
    assert np.array_equal(r.s.get_graded(), r.graded), "a refused tr_scene_set_lut changed the table"
    r.s.close()


@pytest.mark.gpu
def test_python_render_frames_refusals(small_synthetic):
    s = make(small_synthetic, 256, 48, "pose")
    s.set_skin(*rig(small_synthetic[0]), n_bones=2)
    f = frames_arg(2)
    one, three = frames_arg(1), frames_arg(3)
    inst = np.zeros((2, 2, 4), np.float32)
    xf = np.stack([TABLES["A"](), TABLES["B"]()])
    w = np.stack([POSES["A"], POSES["B"]])
    pal = np.stack([PALETTES["A"](), PALETTES["B"]()])
    beside_palettes = "bone_palettes= draws the scene's current pose and table: nothing else per frame beside it"
    cases = [
        (dict(bone_palettes=pal, morph_weights=w), beside_palettes),
        (dict(bone_palettes=pal, instances=inst), beside_palettes),
        (dict(bone_palettes=pal, instance_transforms=xf), beside_palettes),
        (dict(bone_palettes=pal, instances=inst, instance_transforms=xf), beside_palettes),     # the palettes' text comes first
        (dict(instances=inst, instance_transforms=xf), "one table per frame: instances= or instance_transforms=, not both"),
        (dict(instances=inst, instance_transforms=xf, morph_weights=w), "one table per frame: instances= or instance_transforms=, not both"),
        (dict(morph_weights=w, instances=inst), "morph_weights= draws the scene's current table: no table per frame beside it"),
        (dict(morph_weights=w, instance_transforms=xf), "morph_weights= draws the scene's current table: no table per frame beside it"),
    ]
    for kw, text in cases:
        with pytest.raises(ValueError) as e:
            s.render_frames(f, **kw)
        assert str(e.value) == text, kw.keys()
    fb = int(s.frame_buffer_device())
    per_frame = [(dict(frame_buffers_device=[fb, fb]), "one frame buffer per frame"), (dict(bone_palettes=pal), "one palette per frame"),
                 (dict(morph_weights=w), "one pose per frame"), (dict(instance_transforms=xf), "one instance transform table per frame"),
                 (dict(instances=inst), "one instance table per frame")]
    for kw, text in per_frame:
        for frames in (one, three):
            with pytest.raises(ValueError) as e:
                s.render_frames(frames, **kw)
            assert str(e.value) == text, kw.keys()
    assert s.frames_kept() == 0, "a refused call rendered"
    s.close()


# ------------------------------------------------------------------------------------------------------------------
# State across the places that render a frame again
# ------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("W,Hh", SIZES)
@pytest.mark.parametrize("kind", KINDS)
def test_ensure_depth_draws_the_frames_state_and_leaves_the_callers(small_synthetic, kind, W, Hh):
    a, b = only(small_synthetic, W, Hh, kind, "A"), only(small_synthetic, W, Hh, kind, "B")
    assert not np.array_equal(a[0], b[0]) and not np.array_equal(a[1], b[1])
    s = make(small_synthetic, W, Hh, kind, auto_group=False)      # no stored depth: the frame's z stays on the chip
    give(s, kind, "A")
    s.clear()
    s.render()
    give(s, kind, "B")
    assert np.array_equal(bits(s.read_z_f32()), a[1]), "the depth-only repeat did not draw the frame's own state"
    assert np.array_equal(s.get_frame_buffer(), a[0])
    assert np.array_equal(frame(s), b[0]), "the repeat did not put the caller's state back"
    assert np.array_equal(bits(s.read_z_f32()), b[1])
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("W,Hh", SIZES)
@pytest.mark.parametrize("kind", KINDS)
def test_a_frame_held_back_alone_keeps_its_state_and_a_later_clear(small_synthetic, kind, W, Hh):
    a, b = only(small_synthetic, W, Hh, kind, "A"), only(small_synthetic, W, Hh, kind, "B")
    s = make(small_synthetic, W, Hh, kind, frames_per_launch=2)   # (auto-group is on: a cleared frame is held back)
    give(s, kind, "A")
    s.clear()
    s.render()
    give(s, kind, "B")
    s.clear()
    assert np.array_equal(device_frame(s), a[0]), "the frame held back was not drawn under the state it was issued in"
    s.render()
    assert np.array_equal(s.get_frame_buffer(), b[0]), "the clear issued after the frame did not stay pending, or B was lost"
    assert np.array_equal(bits(s.read_z_f32()), b[1])
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("W,Hh", SIZES)
@pytest.mark.parametrize("kind", KINDS)
def test_a_group_without_tables_draws_the_current_one_and_leaves_the_last_view(small_synthetic, kind, W, Hh):
    s = make(small_synthetic, W, Hh, kind, frames_per_launch=2)
    give(s, kind, "A")
    s.clear()
    s.render()
    give(s, kind, "B")
    s.render_frames(np.stack([VIEWS[k] for k in CALL]))
    assert s.frames_kept() == 2
    last = only(small_synthetic, W, Hh, kind, "C2", "B")
    assert np.array_equal(s.get_frame_buffer(), last[0])
    assert np.array_equal(bits(s.read_z_f32()), last[1])
    assert np.array_equal(frame(s), last[0]), "render() after the call: the call's last view under B's table"
    s.render_frames(np.stack([VIEWS[k] for k in CALL]))
    s.select_frame(1)
    assert np.array_equal(s.get_frame_buffer(), only(small_synthetic, W, Hh, kind, "C1", "B")[0])
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("W,Hh", SIZES)
def test_a_replayed_call_draws_its_tables_and_leaves_the_callers_state(small_synthetic, W, Hh):
    kind = "table"
    s = make(small_synthetic, W, Hh, kind, bin_capacity=64, frames_per_launch=2)   # 1 152 polygons: far more than 64 pairs
    give(s, kind, "A")
    s.render_frames(np.stack([VIEWS[k] for k in CALL]), instance_transforms=np.stack([TABLES[k]() for k in CALL]))
    give(s, kind, "B")
    assert np.array_equal(s.get_frame_buffer(), only(small_synthetic, W, Hh, kind, "C2")[0]), "the last frame, complete"
    assert s.frames_kept() == 2
    b = only(small_synthetic, W, Hh, kind, "B")
    assert np.array_equal(frame(s), b[0]), "the replay did not put the caller's state back"
    assert np.array_equal(bits(s.read_z_f32()), b[1])
    s.close()
    # the older kept frame was rendered again too
    s = make(small_synthetic, W, Hh, kind, bin_capacity=64, frames_per_launch=2)
    s.render_frames(np.stack([VIEWS[k] for k in CALL]), instance_transforms=np.stack([TABLES[k]() for k in CALL]))
    give(s, kind, "B")
    assert s.sync() == 0
    s.select_frame(1)
    assert np.array_equal(s.get_frame_buffer(), only(small_synthetic, W, Hh, kind, "C1")[0])
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("W,Hh", SIZES)
@pytest.mark.parametrize("auto_group", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_a_replayed_render_draws_its_state_and_leaves_the_callers(small_synthetic, kind, auto_group, W, Hh):
    a, b = only(small_synthetic, W, Hh, kind, "A"), only(small_synthetic, W, Hh, kind, "B")
    s = make(small_synthetic, W, Hh, kind, bin_capacity=64, auto_group=auto_group)
    give(s, kind, "A")
    s.clear()
    s.render()
    give(s, kind, "B")
    assert np.array_equal(s.get_frame_buffer(), a[0]), "the frame rendered again after the overflow, complete"
    assert np.array_equal(bits(s.read_z_f32()), a[1])
    assert np.array_equal(frame(s), b[0]), "the replay did not put the caller's state back"
    assert np.array_equal(bits(s.read_z_f32()), b[1])
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("W,Hh", SIZES)
@pytest.mark.parametrize("kind", ["pose", "palette"])
def test_select_frame_installs_the_frames_view_and_pose(small_synthetic, kind, W, Hh):
    s = make(small_synthetic, W, Hh, kind, frames_per_launch=4)
    give(s, kind, "A")
    per_frame = dict(morph_weights=np.stack([POSES[k] for k in CALL])) if kind == "pose" else \
        dict(bone_palettes=np.stack([PALETTES[k]() for k in ("A", "B", "A")]))
    names = CALL if kind == "pose" else ("A", "B", "A")
    s.render_frames(np.stack([VIEWS[k] for k in CALL]), **per_frame)
    assert s.frames_kept() == 3
    give(s, kind, "B")
    s.select_frame(1)
    s.render()                                       # no clear: onto the selected frame, under its view, table (A) and pose
    want = only(small_synthetic, W, Hh, kind, "C1", "A", names[1], twice=True)
    assert np.array_equal(s.get_frame_buffer(), want[0])
    assert np.array_equal(bits(s.read_z_f32()), want[1])
    once = only(small_synthetic, W, Hh, kind, "C1", "A", names[1])
    assert np.array_equal(frame(s), once[0]), "the selection stays: a cleared render draws the selected frame again"
    s.close()
