"""Morph targets (tr_scene_set_morph_targets, tr_scene_set_morph_weights, tr_scene_render_frames_morphed,
tr_morph_mesh): a scene under a pose must render bit for bit what a scene created from the host-morphed mesh renders
-- rgb, z bits, shadow bits, winner index -- and what the oracle draws of that mesh.  Everything here is exact equality
of bytes or bits; no tolerance appears anywhere."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import helpers as H

ALL = ("default", "phong", "normal_map", "specular", "darboux", "shadow", "occlusion")
W, HH = 640, 480


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _targets(mesh):
    """Four targets of the GPU tests: 0 a scaled copy (inflate), 1 a sine displacement along x by height, 2 a squash in y,
    3 a shear turning x into z.  Normals get deltas of their own (they are not renormalised)."""
    pos = np.asarray(mesh["pos"], np.float32).reshape(-1, 3)
    nrm = np.asarray(mesh["nrm"], np.float32).reshape(-1, 3)
    dp = np.zeros((4,) + pos.shape, np.float32)
    dn = np.zeros((4,) + nrm.shape, np.float32)
    dp[0] = pos * np.float32(0.2)
    dp[1, :, 0] = np.float32(0.12) * np.sin(np.float32(7.0) * pos[:, 1])
    dn[1, :, 1] = np.float32(-0.4) * np.cos(np.float32(7.0) * nrm[:, 1]) * nrm[:, 0]
    dp[2, :, 1] = np.float32(-0.35) * pos[:, 1]
    dn[2, :, 1] = np.float32(0.3) * nrm[:, 1]
    dp[3, :, 2] = np.float32(0.25) * pos[:, 0]
    dn[3, :, 0] = np.float32(-0.25) * nrm[:, 2]
    return dp, dn


POSE = np.array([1.25, 0.0, -0.6, 0.5], np.float32)      # above 1, a zero, a negative
POSE_B = np.array([0.0, 1.0, 0.0, 0.0], np.float32)      # one target only
POSE_BIG = np.array([6.0, 0.0, 0.0, 0.0], np.float32)    # the mesh 2.2 times as large: many more (polygon, tile) pairs


def _poses(n):
    """A pose per frame: a triangle wave on target 1, a ramp on 0, target 2 on every third frame, 3 never."""
    w = np.zeros((n, 4), np.float32)
    for i in range(n):
        w[i, 0] = 0.1 * i
        w[i, 1] = 1.0 - abs((i % 4) / 2.0 - 1.0)
        w[i, 2] = -0.5 if i % 3 == 0 else 0.0
    return w


LONG_CALL = 400   # frames of the pool test's call: a hundred groups of four


def _long_call(n):
    """Views and poses of a long call: the camera turns, the pose moves on every frame."""
    p = np.zeros((n, 12), np.float32)
    w = np.zeros((n, 4), np.float32)
    for i in range(n):
        p[i, 0:3] = H.light(0.7)
        p[i, 3:6], p[i, 6:9], p[i, 9:12] = H.camera(0.3 + 0.01 * i)
        w[i, 0] = 0.2 + 0.002 * i
        w[i, 1] = 1.0 - abs((i % 16) / 8.0 - 1.0)
    return p, w


def _posed(mesh, w, targets=None):
    import tiny_renderer_amd as T
    dp, dn = targets if targets is not None else _targets(mesh)
    pos, nrm = T.morph_mesh(mesh, dp, dn, w)
    return dict(mesh, pos=pos, nrm=nrm)


def _frame(s, cam=0.3, light=0.7):
    s.clear()
    s.set_light_direction(H.light(light))
    s.set_camera(*H.camera(cam))
    s.render()


def _params(n, cam=0.3, light=0.7):
    p = np.zeros((n, 12), np.float32)
    for i in range(n):
        p[i, 0:3] = H.light(light + 0.05 * i)
        p[i, 3:6], p[i, 6:9], p[i, 9:12] = H.camera(cam + 0.1 * i)
    return p


def _frame_p(s, q):
    s.clear()
    s.set_light_direction(q[0:3])
    s.set_camera(q[3:6], q[6:9], q[9:12])
    s.render()


def _default_q(cam=0.3, light=0.7):
    return np.concatenate([np.asarray(H.light(light), np.float32)] + [np.asarray(v, np.float32) for v in H.camera(cam)])


def _oracle_frame(mesh, texs, pipe, q, w=W, h=HH):
    from oracle import oracle as O
    cpu = O.Scene(w, h, mesh, texs, pipe)
    cpu.clear()
    cpu.set_light_direction(q[0:3])
    cpu.set_camera(q[3:6], q[6:9], q[9:12])
    status = cpu.render()
    return cpu, status


def _assert_same(a, b, pipe, winner=False):
    za, zb = a.read_z_f32().view(np.uint32), b.read_z_f32().view(np.uint32)
    assert np.array_equal(za, zb), "z bits differ at %d pixels" % int((za != zb).sum())
    if pipe in ("shadow", "occlusion"):
        sa, sb = a.read_shadow_f32().view(np.uint32), b.read_shadow_f32().view(np.uint32)
        assert np.array_equal(sa, sb), "shadow bits differ at %d pixels" % int((sa != sb).sum())
    if winner:
        wa, wb = a.read_winner_u32(), b.read_winner_u32()
        assert np.array_equal(wa, wb), "winner differs at %d pixels" % int((wa != wb).sum())
        assert len(np.unique(wa[wa != 0xFFFFFFFF])) > 1
    fa, fb = a.get_frame_buffer(), b.get_frame_buffer()
    assert np.array_equal(fa, fb), "rgb differs at %d pixels" % int((fa != fb).any(-1).sum())
    assert fa.any(), "empty frame"


def _assert_oracle(gpu, cpu, pipe):
    """z bits, shadow bits and rgb against the oracle (no winner tap needed)."""
    zo, zg = cpu.z_f32().view(np.uint32), gpu.read_z_f32().view(np.uint32)
    assert np.array_equal(zg, zo), "z bits differ from the oracle's at %d pixels" % int((zg != zo).sum())
    if pipe in ("shadow", "occlusion"):
        so, sg = cpu.shadow_f32().view(np.uint32), gpu.read_shadow_f32().view(np.uint32)
        assert np.array_equal(sg, so), "shadow bits differ from the oracle's at %d pixels" % int((sg != so).sum())
    fo, fg = cpu.get_frame_buffer(), gpu.get_frame_buffer()
    assert np.array_equal(fg, fo), "rgb differs from the oracle's at %d pixels" % int((fg != fo).any(-1).sum())


def _morphing(T, w, h, mesh, texs, pipe, **kw):
    s = T.Scene(w, h, mesh, texs, pipe, **kw)
    s.set_morph_targets(*_targets(mesh))
    return s


# --- CPU ----------------------------------------------------------------------------------------

def test_morph_symbols_declared_exported_typed(built):
    import tiny_renderer_amd as T
    from tiny_renderer_amd import _lib
    hdr = open(os.path.join(H.REPO, "include", "tiny_renderer.h")).read()
    lib = C.CDLL(T.library_path())
    want = {
        "tr_scene_set_morph_targets": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]),
        "tr_scene_set_morph_weights": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p]),
        "tr_scene_render_frames_morphed": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]),
        "tr_morph_mesh": (C.c_int, [C.POINTER(_lib.Mesh), C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
        "tr_scene_debug_morph_rows": (C.c_int, [C.c_void_p]),
    }
    for name, sig in want.items():
        assert name + "(" in hdr.replace(" (", "(")
        assert hasattr(lib, name)
        assert _lib.SYMBOLS[name] == sig
    assert "#define TR_MORPH_MAX_TARGETS 64" in hdr and _lib.TR_MORPH_MAX_TARGETS == 64
    assert T.load_library().tr_abi_version() == 3
    assert "#define TR_ABI_VERSION 3 " in hdr


def _rule(p, w, d):
    """The rule restated in numpy float32: every product and every sum is one float32 operation."""
    v = np.array(p, np.float32, copy=True)
    with np.errstate(all="ignore"):
        for k in range(len(w)):
            if w[k] != 0.0:
                v = (v + (np.float32(w[k]) * d[k]).astype(np.float32)).astype(np.float32)
    return v


def _rule_contracted(p, w, d):
    """As a fusing implementation would: the product enters the sum unrounded (exact in float64), one rounding per step."""
    v = np.array(p, np.float32, copy=True)
    with np.errstate(all="ignore"):
        for k in range(len(w)):
            if w[k] != 0.0:
                v = (v.astype(np.float64) + np.float64(w[k]) * d[k].astype(np.float64)).astype(np.float32)
    return v


def _rule_reversed(p, w, d):
    v = np.array(p, np.float32, copy=True)
    with np.errstate(all="ignore"):
        for k in reversed(range(len(w))):
            if w[k] != 0.0:
                v = (v + (np.float32(w[k]) * d[k]).astype(np.float32)).astype(np.float32)
    return v


def _rule_cases(mesh):
    """(name, mesh, dpos, dnrm, w) of the host-rule test."""
    rs = np.random.RandomState(7)
    pos = np.asarray(mesh["pos"], np.float32)
    nrm = np.asarray(mesh["nrm"], np.float32)
    cases = []
    dp = (rs.standard_normal((5,) + pos.shape) * 0.3).astype(np.float32)
    dn = (rs.standard_normal((5,) + nrm.shape) * 0.3).astype(np.float32)
    cases.append(("several", mesh, dp, dn, np.array([0.3, 0.9, 0.1, 0.7, 0.45], np.float32)))
    cases.append(("sparse, negative", mesh, dp, dn, np.array([0.0, -0.8, 0.0, -0.0, -1.0 / 3.0], np.float32)))
    cases.append(("above one", mesh, dp, dn, np.array([1.7, 0.0, 3.1, 2.2, 0.0], np.float32)))
    cases.append(("the gpu tests'", mesh) + _targets(mesh) + (POSE,))
    # a -0.0 component under a pose of zeros (either sign) stays -0.0, whatever the targets hold
    mz = dict(mesh, pos=pos.copy(), nrm=nrm.copy())
    mz["pos"][::3, 0] = np.float32(-0.0)
    mz["nrm"][::5, 2] = np.float32(-0.0)
    cases.append(("zeros", mz, dp, dn, np.array([0.0, -0.0, 0.0, 0.0, -0.0], np.float32)))
    # a zero weight on a target holding inf and nan is skipped
    bad_p, bad_n = dp.copy(), dn.copy()
    bad_p[1, ::2] = np.float32(np.inf)
    bad_p[1, 1::2] = np.float32(np.nan)
    bad_n[1] = np.float32(-np.inf)
    bad_n[3, ::2] = np.float32(np.nan)
    cases.append(("non-finite at weight zero", mz, bad_p, bad_n, np.array([0.6, 0.0, -0.2, -0.0, 1.5], np.float32)))
    # an exact cancellation: d = -p at weight 1 gives +0.0, then a second target builds on it
    cp = np.stack([-pos, pos * np.float32(0.5)])
    cn = np.stack([-nrm, nrm * np.float32(0.25)])
    cases.append(("cancellation", mesh, cp, cn, np.array([1.0, 0.0], np.float32)))
    cases.append(("cancellation, then more", mesh, cp, cn, np.array([1.0, 2.0], np.float32)))
    return cases


def test_host_rule_equals_numpy_bit_for_bit(small_synthetic):
    import tiny_renderer_amd as T
    fused_differs = order_differs = 0
    for name, mesh, dp, dn, w in _rule_cases(small_synthetic[0]):
        pos, nrm = T.morph_mesh(mesh, dp, dn, w)
        for got, key, d in ((pos, "pos", dp), (nrm, "nrm", dn)):
            base = np.asarray(mesh[key], np.float32)
            want = _rule(base, w, d)
            assert np.array_equal(_bits(got), _bits(want)), "%s, %s: %d words differ" % (name, key, int((_bits(got) != _bits(want)).sum()))
            fused_differs += int((_bits(got) != _bits(_rule_contracted(base, w, d))).sum())
            order_differs += int((_bits(got) != _bits(_rule_reversed(base, w, d))).sum())
            if name == "zeros":
                assert np.array_equal(_bits(got), _bits(base)) and np.signbit(got[got == 0.0]).any()
            if name == "non-finite at weight zero":
                assert np.isfinite(got).all() and not np.isfinite(d).all()
            if name == "cancellation":
                assert not _bits(got).any()   # every component +0.0
    # a contracted evaluation, and one in the reverse target order, would be noticed on these inputs
    assert fused_differs > 0
    assert order_differs > 0


def test_morph_deltas_from_a_second_mesh(small_synthetic):
    import tiny_renderer_amd as T
    mesh = small_synthetic[0]
    other = _posed(mesh, POSE)
    dp, dn = T.morph_deltas(mesh, other)
    assert dp.shape == (1,) + np.asarray(mesh["pos"]).shape and dn.shape == (1,) + np.asarray(mesh["nrm"]).shape
    assert np.array_equal(_bits(dp[0]), _bits(other["pos"] - np.asarray(mesh["pos"], np.float32)))
    assert np.array_equal(_bits(dn[0]), _bits(other["nrm"] - np.asarray(mesh["nrm"], np.float32)))
    with pytest.raises(ValueError):
        T.morph_deltas(mesh, dict(other, idx=np.asarray(mesh["idx"])[::-1]))
    with pytest.raises(ValueError):
        T.morph_deltas(mesh, dict(other, pos=other["pos"][:-1]))


def _check_posed_frame(mesh, posed, texs, pipe, q, w=W, h=HH):
    """The three conditions on a posed mesh a GPU test draws: no device-error status, a frame that differs from the base
    mesh's, winners from more than one polygon."""
    cpu, status = _oracle_frame(posed, texs, pipe, q, w, h)
    base, status0 = _oracle_frame(mesh, texs, pipe, q, w, h)
    assert status == 0 and status0 == 0
    win = cpu.winner_u32()
    assert len(np.unique(win[win != 0xFFFFFFFF])) > 1
    assert not np.array_equal(cpu.get_frame_buffer(), base.get_frame_buffer())
    cpu.close()
    base.close()


def test_oracle_draws_every_posed_mesh_of_the_gpu_tests(small_synthetic, synthetic):
    import tiny_renderer_amd as T
    mesh, texs = small_synthetic
    for pipe in ALL:
        _check_posed_frame(mesh, _posed(mesh, POSE), texs, pipe, _default_q())
    for w in (POSE_B, POSE_BIG):
        _check_posed_frame(mesh, _posed(mesh, w), texs, "phong", _default_q(), 320, 256)
    n = 9
    p, poses = _params(n), _poses(n)
    for pipe in ("phong", "shadow"):
        for i in range(n - 4, n):
            _check_posed_frame(mesh, _posed(mesh, poses[i]), texs, pipe, p[i], 320, 256)
    _check_posed_frame(mesh, _posed(mesh, poses[n - 1]), texs, "phong", _default_q(1.1, 0.7 + 0.05 * (n - 1)), 320, 256)
    _check_posed_frame(mesh, _posed(mesh, poses[n - 3]), texs, "phong", _default_q(0.2, 0.1), 320, 256)
    from tests.test_instancing import TABLE
    from tests.test_instance_transforms import _table
    posed = _posed(mesh, POSE)
    _check_posed_frame(T.apply_instances(mesh, TABLE), T.apply_instances(posed, TABLE), texs, "phong", _default_q())
    _check_posed_frame(T.apply_instance_transforms(mesh, _table()), T.apply_instance_transforms(posed, _table()), texs, "phong",
                       _default_q())
    # the compose test's fused frames: poses 4 and 2 of five, and POSE_B, under each table at 320 x 256
    p5, poses5 = _params(5), _poses(5)
    for apply, table in ((T.apply_instances, TABLE), (T.apply_instance_transforms, _table())):
        for i in (4, 2):
            _check_posed_frame(apply(mesh, table), apply(_posed(mesh, poses5[i]), table), texs, "phong", p5[i], 320, 256)
        _check_posed_frame(apply(mesh, table), apply(_posed(mesh, POSE_B), table), texs, "phong", p5[4], 320, 256)
    # the held-back test's poses at 320 x 256, the errors test's frame at 256 x 256, the pool test's frames at 128 x 64
    for w in (POSE, POSE_BIG * np.float32(0.25)):
        _check_posed_frame(mesh, _posed(mesh, w), texs, "phong", _default_q(), 320, 256)
    _check_posed_frame(mesh, _posed(mesh, POSE), texs, "phong", _default_q(), 256, 256)
    pl, wl = _long_call(LONG_CALL)
    for i in (LONG_CALL - 1, LONG_CALL - 3):
        _check_posed_frame(mesh, _posed(mesh, wl[i]), texs, "phong", pl[i], 128, 64)
    # the enlarging test needs every frame of its group to want more than its 64 records: one per kept polygon at least
    for w in (POSE_B, POSE, POSE_BIG):
        cpu, status = _oracle_frame(_posed(mesh, w), texs, "phong", _default_q(), 320, 256)
        assert status == 0 and max(st["tri_kept"] for st in cpu.stats()) > 64, cpu.stats()
        cpu.close()
    big, big_texs = synthetic
    _check_posed_frame(big, _posed(big, POSE), big_texs, "phong", _default_q(0.0, 0.0), 1024, 512)


def test_python_layer_rejects_bad_shapes(small_synthetic):
    import tiny_renderer_amd as T
    mesh = small_synthetic[0]
    dp, dn = _targets(mesh)
    with pytest.raises(ValueError):
        T.morph_mesh(mesh, dp[:, :-1], dn, POSE)
    with pytest.raises(ValueError):
        T.morph_mesh(mesh, dp, dn[:2], POSE)
    with pytest.raises(ValueError):
        T.morph_mesh(mesh, dp, dn, POSE[:3])
    with pytest.raises(ValueError):
        T.morph_mesh(mesh, dp[0], dn[0], POSE[:1])
    with pytest.raises(ValueError):
        T.morph_mesh(mesh, np.zeros((65,) + dp.shape[1:], np.float32), np.zeros((65,) + dn.shape[1:], np.float32), np.zeros(65, np.float32))
    # the C entry point itself: more targets than the limit, NULL where data is required
    from tiny_renderer_amd import _lib
    from tiny_renderer_amd.scene import _mesh_struct
    L = _lib.load_library()
    keep = []
    m = _mesh_struct(mesh, keep)
    out_p, out_n = np.empty_like(dp[0]), np.empty_like(dn[0])
    w = np.zeros(65, np.float32)
    assert L.tr_morph_mesh(C.byref(m), 65, dp.ctypes.data, dn.ctypes.data, w.ctypes.data, out_p.ctypes.data, out_n.ctypes.data) == _lib.TR_E_INVALID
    assert L.tr_morph_mesh(C.byref(m), 4, None, dn.ctypes.data, w.ctypes.data, out_p.ctypes.data, out_n.ctypes.data) == _lib.TR_E_INVALID
    assert L.tr_morph_mesh(C.byref(m), 4, dp.ctypes.data, dn.ctypes.data, None, out_p.ctypes.data, out_n.ctypes.data) == _lib.TR_E_INVALID
    assert L.tr_morph_mesh(None, 4, dp.ctypes.data, dn.ctypes.data, w.ctypes.data, out_p.ctypes.data, out_n.ctypes.data) == _lib.TR_E_INVALID


# --- GPU ----------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("pipe", ALL)
def test_posed_scene_equals_morphed_mesh_and_oracle(small_synthetic, pipe):
    import tiny_renderer_amd as T
    from tests.test_gpu_parity import assert_parity
    mesh, texs = small_synthetic
    posed = _posed(mesh, POSE)
    s = _morphing(T, W, HH, mesh, texs, pipe, winner_tap=True)
    s.set_morph_weights(POSE)
    ref = T.Scene(W, HH, posed, texs, pipe, winner_tap=True)
    for q in (s, ref):
        _frame(q)
    _assert_same(s, ref, pipe, winner=True)
    cpu, status = _oracle_frame(posed, texs, pipe, _default_q())
    assert status == 0
    assert_parity(s, cpu, pipe)
    cpu.close()
    # a pose of zeros and no pose at all: the mesh itself
    base = T.Scene(W, HH, mesh, texs, pipe, winner_tap=True)
    _frame(base)
    for w in (np.zeros(4, np.float32), None):
        s.set_morph_weights(w)
        _frame(s)
        _assert_same(s, base, pipe, winner=True)
    for q in (s, ref, base):
        q.close()


@pytest.mark.gpu
@pytest.mark.parametrize("pipe", ["phong", "shadow"])
def test_render_frames_morphed_groups(small_synthetic, pipe):
    import tiny_renderer_amd as T
    mesh, texs = small_synthetic
    w, h, n = 320, 256, 9   # 2 x frames_per_launch + 1
    p, poses = _params(n), _poses(n)
    fused = _morphing(T, w, h, mesh, texs, pipe, frames_per_launch=4)
    fused.render_frames(p, morph_weights=poses)
    assert fused.frames_kept() == 4
    loop = _morphing(T, w, h, mesh, texs, pipe)
    for back in range(fused.frames_kept()):
        i = n - 1 - back
        posed = _posed(mesh, poses[i])
        fused.select_frame(back)
        loop.set_morph_weights(poses[i])
        _frame_p(loop, p[i])
        ref = T.Scene(w, h, posed, texs, pipe)
        _frame_p(ref, p[i])
        cpu, status = _oracle_frame(posed, texs, pipe, p[i], w, h)
        assert status == 0
        # (read_z_f32 of a fused frame goes through the transient-depth repeat, which must draw the frame's pose)
        _assert_oracle(fused, cpu, pipe)
        _assert_same(fused, ref, pipe)
        _assert_same(loop, ref, pipe)
        cpu.close()
        ref.close()
    # a group followed by a plain render() without clear: the last frame's pose is current, the frame accumulates
    fused.render_frames(p, morph_weights=poses)
    ref = T.Scene(w, h, _posed(mesh, poses[n - 1]), texs, pipe)
    _frame_p(ref, p[n - 1])
    for s in (fused, ref):
        s.set_camera(*H.camera(1.1))
        s.render()
    _assert_same(fused, ref, pipe)
    # a kept frame's pose comes back with it: a later render without a clear accumulates under it
    fused.render_frames(p, morph_weights=poses)
    fused.select_frame(2)
    ref2 = T.Scene(w, h, _posed(mesh, poses[n - 3]), texs, pipe)
    _frame_p(ref2, p[n - 3])
    for s in (fused, ref2):
        s.set_light_direction(H.light(0.1))
        s.set_camera(*H.camera(0.2))
        s.render()
    _assert_same(fused, ref2, pipe)
    # plain render_frames draws the current pose in every frame
    fused.set_morph_weights(POSE_B)
    fused.render_frames(p)
    ref3 = T.Scene(w, h, _posed(mesh, POSE_B), texs, pipe)
    for back in (0, 3):
        fused.select_frame(back)
        _frame_p(ref3, p[n - 1 - back])
        _assert_same(fused, ref3, pipe)
    for s in (fused, loop, ref, ref2, ref3):
        s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["offset_scale", "transform"])
def test_pose_composes_with_instance_tables(small_synthetic, kind):
    import tiny_renderer_amd as T
    from tests.test_instancing import TABLE
    from tests.test_instance_transforms import _table
    mesh, texs = small_synthetic
    pipe = "phong"
    posed = _posed(mesh, POSE)
    s = _morphing(T, W, HH, mesh, texs, pipe, winner_tap=True)
    if kind == "offset_scale":
        s.set_morph_weights(POSE)      # pose first, table second ...
        s.set_instances(TABLE)
        cat = T.apply_instances(posed, TABLE)
    else:
        s.set_instance_transforms(_table())   # ... and the other way round
        s.set_morph_weights(POSE)
        cat = T.apply_instance_transforms(posed, _table())
    ref = T.Scene(W, HH, cat, texs, pipe, winner_tap=True)
    for q in (s, ref):
        _frame(q)
    _assert_same(s, ref, pipe, winner=True)
    # through the fused path: a pose per frame under the current table, then a table per frame under the current pose
    g = _morphing(T, 320, 256, mesh, texs, pipe, frames_per_launch=4)
    p, poses = _params(5), _poses(5)
    tables = np.stack([TABLE] * 5) if kind == "offset_scale" else np.stack([_table()] * 5)
    apply = T.apply_instances if kind == "offset_scale" else T.apply_instance_transforms
    if kind == "offset_scale":
        g.set_instances(TABLE)
    else:
        g.set_instance_transforms(_table())
    g.render_frames(p, morph_weights=poses)
    for back in (0, 2):
        g.select_frame(back)
        r = T.Scene(320, 256, apply(_posed(mesh, poses[4 - back]), tables[0]), texs, pipe)
        _frame_p(r, p[4 - back])
        _assert_same(g, r, pipe)
        r.close()
    g.set_morph_weights(POSE_B)
    if kind == "offset_scale":
        g.render_frames(p, instances=tables)
    else:
        g.render_frames(p, instance_transforms=tables)
    r = T.Scene(320, 256, apply(_posed(mesh, POSE_B), tables[0]), texs, pipe)
    _frame_p(r, p[4])
    _assert_same(g, r, pipe)
    for q in (s, ref, g, r):
        q.close()


@pytest.mark.gpu
def test_held_back_frames_keep_their_pose(small_synthetic):
    """On a scene that holds cleared frames back to fuse them, every frame keeps the pose it was issued with; no pose and
    a pose alternate."""
    import torch
    import tiny_renderer_amd as T
    mesh, texs = small_synthetic
    w, h, pipe = 320, 256, "phong"
    steps = [POSE, None, POSE_B, None, POSE, np.zeros(4, np.float32), POSE_BIG * np.float32(0.25)]
    s = _morphing(T, w, h, mesh, texs, pipe)
    assert s.frames_per_launch > 1
    bufs = [torch.zeros(h * w * 3, dtype=torch.uint8, device="cuda") for _ in steps]
    for pose, buf in zip(steps, bufs):
        s.set_morph_weights(pose)
        s.set_frame_buffer_device(buf.data_ptr())
        _frame(s)
    s.set_morph_weights(POSE_B)   # (changes nothing of what was issued)
    s.sync()
    torch.cuda.synchronize()
    base = T.Scene(w, h, mesh, texs, pipe)
    _frame(base)
    for pose, buf in zip(steps, bufs):
        got = buf.cpu().numpy().reshape(h, w, 3)
        assert got.any()
        if pose is None or not pose.any():
            assert np.array_equal(got, base.get_frame_buffer())
            continue
        ref = T.Scene(w, h, _posed(mesh, pose), texs, pipe)
        _frame(ref)
        assert np.array_equal(got, ref.get_frame_buffer())
        assert not np.array_equal(got, base.get_frame_buffer())
        ref.close()
    s.close()
    base.close()


@pytest.mark.gpu
@pytest.mark.parametrize("fused", [False, True])
def test_enlarging_pose_under_a_small_bin_capacity(small_synthetic, fused):
    """Posed frames that want more records than the pools hold: the internal re-render draws the same pose again.  The
    pools start at 64 records and every posed frame here keeps more than 64 polygons (the CPU test asserts it from the
    oracle), so the first attempt of every frame overflows -- in the fused case all three are queued before anything
    grows -- and the profile must show that more tile-kernel frames ran than the call has."""
    import tiny_renderer_amd as T
    mesh, texs = small_synthetic
    w, h, pipe = 320, 256, "phong"
    order = [POSE_B, POSE, POSE_BIG] if fused else [POSE_BIG]
    s = _morphing(T, w, h, mesh, texs, pipe, bin_capacity=64, frames_per_launch=4 if fused else 0)
    s.profile_enable(True)
    if fused:
        s.render_frames(np.stack([_default_q()] * 3), morph_weights=np.stack(order))
    else:
        s.set_morph_weights(POSE_BIG)
        _frame(s)
    assert s.sync() == 0
    prof = s.profile_read()
    s.profile_enable(False)
    assert prof["k_tile"]["frames"] > len(order), prof["k_tile"]      # frames were rendered again ...
    assert prof["k_morph"]["frames"] == len(order), prof["k_morph"]   # ... from the rows blended once
    for back, pose in enumerate(reversed(order)):
        if fused:
            s.select_frame(back)
        cpu, status = _oracle_frame(_posed(mesh, pose), texs, pipe, _default_q(), w, h)
        assert status == 0
        _assert_oracle(s, cpu, pipe)
        cpu.close()
    s.close()


@pytest.mark.gpu
def test_a_long_morphed_call_does_not_grow_the_row_pool(small_synthetic):
    """A pose's rows are held by its frame's slot, the kept frames and work in flight -- not by the call: after 400 frames
    in groups of four the scene has at most one set per frame slot (<= 32), per frame of the groups in flight (4 sets of
    groups x 4) and for the current pose, and the free ones go back to the device with the targets."""
    import tiny_renderer_amd as T
    mesh, texs = small_synthetic
    w, h, pipe, n = 128, 64, "phong", LONG_CALL
    p, poses = _long_call(n)
    s = _morphing(T, w, h, mesh, texs, pipe, frames_per_launch=4)
    assert s.debug_morph_rows() == 0
    s.render_frames(p, morph_weights=poses)
    bound = 32 + 4 * 4 + 1
    during = s.debug_morph_rows()
    assert 0 < during <= bound, during
    s.sync()
    s.render_frames(p, morph_weights=poses)   # a second call takes its rows from the pool
    assert s.debug_morph_rows() <= bound
    for back in (0, 2):
        s.select_frame(back)
        i = n - 1 - back
        ref = T.Scene(w, h, _posed(mesh, poses[i]), texs, pipe)
        _frame_p(ref, p[i])
        _assert_same(s, ref, pipe)
        ref.close()
    held = s.debug_morph_rows()
    s.set_morph_targets(None)    # waits for the device: what nobody holds goes back
    assert s.debug_morph_rows() <= min(held, 32 + 1)
    s.close()


@pytest.mark.gpu
def test_morphed_band_scenes(synthetic):
    import tiny_renderer_amd as T
    mesh, texs = synthetic
    w, h = 1024, 512
    full = _morphing(T, w, h, mesh, texs, "phong")
    full.set_morph_weights(POSE)
    _frame(full, cam=0.0, light=0.0)
    want = full.get_frame_buffer()
    ref = T.Scene(w, h, _posed(mesh, POSE), texs, "phong")
    _frame(ref, cam=0.0, light=0.0)
    assert np.array_equal(want, ref.get_frame_buffer()) and want.any()
    full.close()
    ref.close()
    for band in ((0, 128), (256, 512)):
        b = _morphing(T, w, h, mesh, texs, "phong", band_rows=band)
        b.set_morph_weights(POSE)
        _frame(b, cam=0.0, light=0.0)
        got = b.get_frame_buffer()[band[0]:band[1]]
        assert np.array_equal(got, want[band[0]:band[1]]) and got.any()
        b.close()


@pytest.mark.gpu
def test_resolve_of_a_posed_frame(small_synthetic):
    import tiny_renderer_amd as T
    mesh, texs = small_synthetic
    s = _morphing(T, W, HH, mesh, texs, "phong")
    s.set_morph_weights(POSE)
    _frame(s)
    fb = s.get_frame_buffer()
    assert fb.any()
    want = ((fb.astype(np.uint32).reshape(HH // 2, 2, W // 2, 2, 3).sum(axis=(1, 3)) + 2) // 4).astype(np.uint8)
    assert np.array_equal(s.resolve(2), want)
    s.close()


@pytest.mark.gpu
def test_morph_errors_leave_targets_and_pose(small_synthetic):
    import tiny_renderer_amd as T
    from tiny_renderer_amd import _lib
    mesh, texs = small_synthetic
    w, h, pipe = 256, 256, "phong"
    L = _lib.load_library()
    dp, dn = _targets(mesh)
    s = _morphing(T, w, h, mesh, texs, pipe)
    s.set_morph_weights(POSE)
    _frame(s)
    before = (s.get_frame_buffer(), s.read_z_f32().view(np.uint32))
    assert before[0].any()
    p = _params(1)
    five = np.zeros(5, np.float32)
    assert L.tr_scene_set_morph_targets(s._h, 65, dp.ctypes.data, dn.ctypes.data) == _lib.TR_E_INVALID
    assert L.tr_scene_set_morph_targets(s._h, 4, None, dn.ctypes.data) == _lib.TR_E_INVALID
    assert L.tr_scene_set_morph_targets(s._h, 4, dp.ctypes.data, None) == _lib.TR_E_INVALID
    assert L.tr_scene_set_morph_targets(None, 4, dp.ctypes.data, dn.ctypes.data) == _lib.TR_E_INVALID
    assert L.tr_scene_set_morph_weights(s._h, 5, five.ctypes.data) == _lib.TR_E_INVALID
    assert L.tr_scene_set_morph_weights(s._h, 3, five.ctypes.data) == _lib.TR_E_INVALID
    assert L.tr_scene_set_morph_weights(s._h, 4, None) == _lib.TR_E_INVALID
    assert L.tr_scene_set_morph_weights(None, 4, five.ctypes.data) == _lib.TR_E_INVALID
    assert L.tr_scene_render_frames_morphed(s._h, 1, p.ctypes.data, 5, five.ctypes.data, None) == _lib.TR_E_INVALID
    assert L.tr_scene_render_frames_morphed(s._h, 1, p.ctypes.data, 4, None, None) == _lib.TR_E_INVALID
    assert L.tr_scene_render_frames_morphed(None, 1, p.ctypes.data, 4, five.ctypes.data, None) == _lib.TR_E_INVALID
    with pytest.raises(ValueError):
        s.set_morph_weights(five)
    with pytest.raises(ValueError):
        s.set_morph_targets(dp[:, :-1], dn)
    with pytest.raises(ValueError):
        s.render_frames(p, morph_weights=np.zeros((2, 4), np.float32))
    with pytest.raises(ValueError):
        s.render_frames(p, morph_weights=np.zeros((1, 4), np.float32), instances=np.zeros((1, 1, 4), np.float32))
    _frame(s)
    assert np.array_equal(s.get_frame_buffer(), before[0]) and np.array_equal(s.read_z_f32().view(np.uint32), before[1])
    ref = T.Scene(w, h, _posed(mesh, POSE), texs, pipe)
    _frame(ref)
    _assert_same(s, ref, pipe)
    # dropping the targets drops the pose: the mesh itself, and weights are then an error
    s.set_morph_targets(None)
    assert L.tr_scene_set_morph_weights(s._h, 4, POSE.ctypes.data) == _lib.TR_E_INVALID
    base = T.Scene(w, h, mesh, texs, pipe)
    for q in (s, base):
        _frame(q)
    _assert_same(s, base, pipe)
    for q in (s, ref, base):
        q.close()
