"""Skinning (tr_scene_set_skin, tr_scene_set_bone_palette, tr_scene_render_frames_skinned, tr_skin_mesh): a scene under a
bone palette must render bit for bit what a scene created from the host-skinned mesh renders -- rgb, z bits, shadow
bits, winner index -- and what the oracle draws of that mesh.  Everything here is exact equality of bytes or bits; no
tolerance appears anywhere."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import helpers as H
from tests.test_instance_transforms import _rot, _table
from tests.test_morph import (ALL, W, HH, POSE, _assert_oracle, _assert_same, _bits, _check_posed_frame, _default_q, _frame,
                              _frame_p, _oracle_frame, _params, _posed, _targets)

N_BONES = 5


def _rig(mesh):
    """The rig of the tests, per position index: a cap (y > 0.8) of all-zero weights, a base (y < -0.5) of one influence
    of weight 1.0f whose bone follows the longitude, and in between four non-zero influences -- bone 0 and three of the
    bones 1..4 by longitude -- with weights by height and longitude (they do not sum to one: used as given)."""
    pos = np.asarray(mesh["pos"], np.float32).reshape(-1, 3)
    n = pos.shape[0]
    y = pos[:, 1].astype(np.float64)
    lon = (np.arctan2(pos[:, 0].astype(np.float64), pos[:, 2].astype(np.float64)) + np.pi) / (2.0 * np.pi) * 4.0
    k = np.minimum(lon.astype(np.int64), 3)
    f = lon - k
    bones = np.zeros((n, 4), np.uint32)
    weights = np.zeros((n, 4), np.float32)
    s = np.clip((y + 0.5) / 1.3, 0.0, 1.0)
    mid = (y >= -0.5) & (y <= 0.8)
    bones[mid] = np.stack([np.zeros_like(k), 1 + k, 1 + (k + 1) % 4, 1 + (k + 2) % 4], axis=1)[mid]
    weights[mid] = np.stack([1.0 - 0.8 * s, 0.1 + 0.6 * s * (1.0 - f), 0.05 + 0.6 * s * f, 0.02 + 0.25 * s], axis=1)[mid]
    base = y < -0.5
    bones[base] = np.stack([1 + k, np.full_like(k, 3), np.zeros_like(k), np.full_like(k, 4)], axis=1)[base]
    weights[base, 0] = np.float32(1.0)
    four = int((weights != 0).all(1).sum())
    one = int(((weights != 0).sum(1) == 1).sum())
    none = int((~(weights != 0).any(1)).sum())
    assert four > 0 and one > 0 and none > 0 and four + one + none == n
    assert set(np.unique(bones[weights != 0])) == set(range(N_BONES))
    return bones, weights


def _palette(turn=0.0, scale=1.0):
    """Five bones: 0 a yaw, 1 a general rotation with an offset, 2 a shear, 3 a mirror (det < 0), 4 a non-uniform scale
    under a rotation.  `turn` (degrees) moves every bone, `scale` enlarges all of them."""
    import tiny_renderer_amd as T
    lin = [_rot(20 + turn),
           _rot(35 - turn, 10, -15),
           np.array([[1.0, 0.25, 0.0], [0.0, 1.0, 0.1], [0.0, 0.0, 1.0]]) @ _rot(turn / 2),
           _rot(15 + turn, -10, 5) @ np.diag([-1.0, 1.0, 1.0]),
           _rot(-30, 20 + turn, 0) @ np.diag([0.9, 1.1, 0.8])]
    off = [[0.0, 0.0, 0.0], [0.1, 0.0, 0.0], [0.0, -0.05, 0.0], [0.0, 0.0, 0.05], [0.0, 0.05, 0.0]]
    t = T.instance_transforms(np.array(lin) * scale, np.array(off))
    assert np.linalg.det(t[3, 0:12].reshape(3, 4)[:, :3].astype(np.float64)) < 0
    return t


PAL_BIG = 2.2        # the mesh about 2.2 times as large: many more (polygon, tile) pairs


def _palettes(n):
    """A palette per frame: every bone turns a little further each frame."""
    return np.stack([_palette(turn=7.0 * i) for i in range(n)])


def _skinned(mesh, pal, rig=None):
    import tiny_renderer_amd as T
    bones, weights = rig if rig is not None else _rig(mesh)
    return T.skin_mesh(mesh, bones, weights, pal)


def _skinning(T, w, h, mesh, texs, pipe, **kw):
    s = T.Scene(w, h, mesh, texs, pipe, **kw)
    s.set_skin(*_rig(mesh), n_bones=N_BONES)
    return s


def _wide_rig(mesh, n_bones):
    """A rig over n_bones bones: every position index has four non-zero influences on scattered bones; the highest
    bone index occurs."""
    n = np.asarray(mesh["pos"]).reshape(-1, 3).shape[0]
    i = np.arange(n, dtype=np.int64)[:, None]
    j = np.arange(4, dtype=np.int64)[None, :]
    bones = ((i * 37 + j * 11 + (i * j) % 5) % n_bones).astype(np.uint32)
    bones[n // 2, 2] = n_bones - 1
    weights = (0.1 + ((i * 7 + j * 3) % 9) / 16.0).astype(np.float32)
    assert int(bones.max()) == n_bones - 1 and (weights != 0).all()
    return bones, weights


def _wide_palette(n_bones):
    import tiny_renderer_amd as T
    lin = np.array([_rot(2.5 * k, 10 * np.sin(k), -0.7 * k) * (0.25 + 0.01 * (k % 7)) for k in range(n_bones)])
    off = np.array([[0.02 * np.sin(k), 0.02 * np.cos(k), 0.0] for k in range(n_bones)])
    return T.instance_transforms(lin, off)


def _edge_case(mesh, n_bones):
    """(rig, palette, the palette reversed) of the bone-count edges: 1 bone and 128."""
    rig = _wide_rig(mesh, n_bones)
    pal = _wide_palette(128)[-n_bones:] * np.float32(1.0 if n_bones > 1 else 2.0)
    assert int(rig[0].max()) == n_bones - 1
    return rig, pal, np.ascontiguousarray(pal[::-1])


LONG_CALL = 400


def _long_call(n):
    p = np.zeros((n, 12), np.float32)
    for i in range(n):
        p[i, 0:3] = H.light(0.7)
        p[i, 3:6], p[i, 6:9], p[i, 9:12] = H.camera(0.3 + 0.01 * i)
    return p


def _long_palette(i):
    return _palette(turn=0.5 * i)


# --- CPU ----------------------------------------------------------------------------------------

def test_skin_symbols_declared_exported_typed(built):
    import tiny_renderer_amd as T
    from tiny_renderer_amd import _lib
    hdr = open(os.path.join(H.REPO, "include", "tiny_renderer.h")).read()
    lib = C.CDLL(T.library_path())
    want = {
        "tr_scene_set_skin": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]),
        "tr_scene_set_bone_palette": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p]),
        "tr_scene_render_frames_skinned": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]),
        "tr_skin_mesh": (C.c_int, [C.POINTER(_lib.Mesh), C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_void_p]),
    }
    for name, sig in want.items():
        assert name + "(" in hdr.replace(" (", "(")
        assert hasattr(lib, name)
        assert _lib.SYMBOLS[name] == sig
    assert "#define TR_SKIN_INFLUENCES 4" in hdr and _lib.TR_SKIN_INFLUENCES == 4
    assert "#define TR_SKIN_MAX_BONES 128" in hdr and _lib.TR_SKIN_MAX_BONES == 128
    assert T.load_library().tr_abi_version() == 3
    assert "#define TR_ABI_VERSION 3 " in hdr


def _f32(x):
    return np.asarray(x, np.float32)


def _xform(e, v, normal):
    """xform_position / xform_normal restated in numpy float32 for vectors v [n, 3] under entries e [n, 24]: every product
    and every sum one float32 operation, left to right."""
    out = np.empty_like(v)
    with np.errstate(all="ignore"):
        for r in range(3):
            if normal:
                m = e[:, 12 + 3 * r:15 + 3 * r]
                out[:, r] = _f32(_f32(_f32(m[:, 0] * v[:, 0]) + _f32(m[:, 1] * v[:, 1])) + _f32(m[:, 2] * v[:, 2]))
            else:
                m = e[:, 4 * r:4 * r + 4]
                out[:, r] = _f32(_f32(_f32(_f32(m[:, 0] * v[:, 0]) + _f32(m[:, 1] * v[:, 1])) + _f32(m[:, 2] * v[:, 2])) + m[:, 3])
    return out


def _xform64(e, v, normal):
    """The same in float64 without intermediate rounding (what contraction into fused operations tends to)."""
    e, v = e.astype(np.float64), v.astype(np.float64)
    out = np.empty_like(v)
    with np.errstate(all="ignore"):
        for r in range(3):
            if normal:
                out[:, r] = (e[:, 12 + 3 * r:15 + 3 * r] * v).sum(1)
            else:
                out[:, r] = (e[:, 4 * r:4 * r + 3] * v).sum(1) + e[:, 4 * r + 3]
    return out


def _corners(mesh):
    idx = np.asarray(mesh["idx"], np.uint32).reshape(-1, 3, 3)
    P, N = idx[:, :, 0].reshape(-1), idx[:, :, 2].reshape(-1)
    pos = np.asarray(mesh["pos"], np.float32).reshape(-1, 3)
    nrm = np.asarray(mesh["nrm"], np.float32).reshape(-1, 3)
    return P, pos[P], nrm[N]


def _rule(mesh, bones, weights, pal, order=range(4), how="rule"):
    """The rule restated in numpy over the unrolled corners: (pos [n_tri * 3, 3], nrm [n_tri * 3, 3]).
    how: "rule" as the header states it; "contracted": products enter the sums unrounded (float64), one rounding per
    influence; "matrix": the four weighted entries are blended first and applied once."""
    P, p, a = _corners(mesh)
    b, w = bones[P], weights[P]
    out = []
    with np.errstate(all="ignore"):
        for v, normal in ((p, False), (a, True)):
            if how == "matrix":
                e = np.zeros((len(P), 24), np.float32)
                for j in order:
                    e = _f32(e + _f32(w[:, j:j + 1] * pal[b[:, j]]))
                acc = _xform(e, v, normal)
                have = (w != 0).any(1)
            else:
                acc = np.zeros_like(v, dtype=np.float64 if how == "contracted" else np.float32)
                have = np.zeros(len(P), bool)
                for j in order:
                    on = w[:, j] != 0
                    if how == "contracted":
                        t = w[:, j:j + 1].astype(np.float64) * _xform64(pal[b[:, j]], v, normal)
                        new = np.where(have[:, None], acc + t, t).astype(np.float32).astype(np.float64)
                    else:
                        t = _f32(w[:, j:j + 1] * _xform(pal[b[:, j]], v, normal))
                        new = np.where(have[:, None], _f32(acc + t), t)
                    acc = np.where(on[:, None], new, acc)
                    have = have | on
            out.append(np.where(have[:, None], acc.astype(np.float32), v))
    return out[0], out[1]


def _zero_mesh(mesh):
    """The mesh with -0.0 components in positions and normals."""
    mz = dict(mesh, pos=np.array(mesh["pos"], np.float32, copy=True).reshape(-1, 3),
              nrm=np.array(mesh["nrm"], np.float32, copy=True).reshape(-1, 3))
    mz["pos"][::3, 0] = np.float32(-0.0)
    mz["nrm"][::5, 2] = np.float32(-0.0)
    return mz


def test_host_rule_equals_numpy_bit_for_bit(small_synthetic):
    import tiny_renderer_amd as T
    mesh = small_synthetic[0]
    cases = [("the rig", mesh, _rig(mesh), _palette()),
             ("the rig, turned", _zero_mesh(mesh), _rig(mesh), _palette(turn=21.0)),
             ("128 bones", mesh, _wide_rig(mesh, 128), _wide_palette(128))]
    differs = {"contracted": 0, "matrix": 0, "reversed": 0}
    for name, m, (bones, weights), pal in cases:
        got = T.skin_mesh(m, bones, weights, pal)
        want = _rule(m, bones, weights, pal)
        idx = np.asarray(m["idx"], np.uint32).reshape(-1, 9)
        n3 = np.arange(idx.shape[0] * 3, dtype=np.uint32).reshape(-1, 3)
        assert np.array_equal(got["idx"][:, 0::3], n3) and np.array_equal(got["idx"][:, 2::3], n3)
        assert np.array_equal(got["idx"][:, 1::3], idx[:, 1::3]) and got["tex"] is m["tex"]
        for k, key in enumerate(("pos", "nrm")):
            assert np.array_equal(_bits(got[key]), _bits(want[k])), "%s, %s: %d words differ" % (name, key, int((_bits(got[key]) != _bits(want[k])).sum()))
            differs["contracted"] += int((_bits(got[key]) != _bits(_rule(m, bones, weights, pal, how="contracted")[k])).sum())
            differs["matrix"] += int((_bits(got[key]) != _bits(_rule(m, bones, weights, pal, how="matrix")[k])).sum())
            differs["reversed"] += int((_bits(got[key]) != _bits(_rule(m, bones, weights, pal, order=(3, 2, 1, 0))[k])).sum())
    # a contracted evaluation, blending the matrices first, and the reverse influence order would all be noticed
    assert all(v > 0 for v in differs.values()), differs


def test_single_influence_corners_equal_the_instance_transform(small_synthetic):
    import tiny_renderer_amd as T
    mesh = small_synthetic[0]
    bones, weights = _rig(mesh)
    pal = _palette()
    got = T.skin_mesh(mesh, bones, weights, pal)
    P, _, _ = _corners(mesh)
    N = np.asarray(mesh["idx"], np.uint32).reshape(-1, 3, 3)[:, :, 2].reshape(-1)
    single = ((weights[P] != 0).sum(1) == 1) & (weights[P, 0] == 1.0)
    assert single.sum() > 0
    tp, tn = T.transform_mesh(mesh, pal)   # instance-major: entry k's positions at [k * n_pos, (k + 1) * n_pos)
    n_pos, n_nrm = np.asarray(mesh["pos"]).reshape(-1, 3).shape[0], np.asarray(mesh["nrm"]).reshape(-1, 3).shape[0]
    k = bones[P, 0].astype(np.int64)
    assert len(np.unique(k[single])) > 1
    assert np.array_equal(_bits(got["pos"][single]), _bits(tp[k * n_pos + P][single]))
    assert np.array_equal(_bits(got["nrm"][single]), _bits(tn[k * n_nrm + N][single]))


def test_all_zero_corners_keep_their_bits_under_nan(small_synthetic):
    import tiny_renderer_amd as T
    mz = _zero_mesh(small_synthetic[0])
    bones, weights = _rig(mz)
    weights = weights.copy()
    weights[::7][~(weights[::7] != 0).any(1), 1] = np.float32(-0.0)   # zeros of either sign
    pal = np.full((N_BONES, 24), np.nan, np.float32)
    got = T.skin_mesh(mz, bones, weights, pal)
    P, p, a = _corners(mz)
    zero = ~(weights[P] != 0).any(1)
    assert zero.sum() > 0 and (~zero).sum() > 0
    assert np.array_equal(_bits(got["pos"][zero]), _bits(p[zero])) and np.array_equal(_bits(got["nrm"][zero]), _bits(a[zero]))
    kept = np.concatenate([got["pos"][zero].reshape(-1), got["nrm"][zero].reshape(-1)])
    assert np.signbit(kept[kept == 0.0]).any()
    assert np.isnan(got["pos"][~zero]).all() and np.isnan(got["nrm"][~zero]).all()


def test_oracle_draws_every_skinned_mesh_of_the_gpu_tests(small_synthetic):
    import tiny_renderer_amd as T
    from tests.test_instancing import TABLE
    mesh, texs = small_synthetic
    rig = _rig(mesh)
    sk = _skinned(mesh, _palette(), rig)
    for pipe in ALL:
        _check_posed_frame(mesh, sk, texs, pipe, _default_q())
    n = 9
    p, pals = _params(n), _palettes(n)
    for pipe in ("phong", "shadow"):
        for i in range(n - 4, n):
            _check_posed_frame(mesh, _skinned(mesh, pals[i], rig), texs, pipe, p[i], 320, 256)
    _check_posed_frame(mesh, _skinned(mesh, pals[n - 3], rig), texs, "phong", _default_q(0.2, 0.1), 320, 256)
    # one bone of weight one, and the kernel's edges: 1 and 128 bones
    one = (np.zeros_like(rig[0]), np.tile(np.array([1, 0, 0, 0], np.float32), (rig[0].shape[0], 1)))
    for pipe in ("phong", "darboux"):
        _check_posed_frame(mesh, _skinned(mesh, _table()[6:7], one), texs, pipe, _default_q(), 320, 256)
    for n_bones in (1, 128):
        edge_rig, pal, pal2 = _edge_case(mesh, n_bones)
        for q in (pal, pal2):
            _check_posed_frame(mesh, _skinned(mesh, q, edge_rig), texs, "phong", _default_q(), 320, 256)
    # composition: morph, then skin, then each kind of table
    both = _skinned(_posed(mesh, POSE), _palette(), rig)
    _check_posed_frame(mesh, both, texs, "phong", _default_q())
    _check_posed_frame(T.apply_instances(mesh, TABLE), T.apply_instances(both, TABLE), texs, "phong", _default_q())
    _check_posed_frame(T.apply_instance_transforms(mesh, _table()), T.apply_instance_transforms(both, _table()), texs, "phong",
                       _default_q())
    # the held-back test's palettes at 320 x 256, the errors test's frame at 256 x 256, the long call's frames at 128 x 64
    for turn in (0.0, 30.0, 60.0):
        _check_posed_frame(mesh, _skinned(mesh, _palette(turn=turn), rig), texs, "phong", _default_q(), 320, 256)
    _check_posed_frame(mesh, sk, texs, "phong", _default_q(), 256, 256)
    pl = _long_call(LONG_CALL)
    for i in (LONG_CALL - 1, LONG_CALL - 3):
        _check_posed_frame(mesh, _skinned(mesh, _long_palette(i), rig), texs, "phong", pl[i], 128, 64)
    # the enlarging test needs every frame of its group to want more than its 64 records: one per kept polygon at least
    for pal in (_palette(), _palette(turn=30.0), _palette(scale=PAL_BIG)):
        cpu, status = _oracle_frame(_skinned(mesh, pal, rig), texs, "phong", _default_q(), 320, 256)
        assert status == 0 and max(st["tri_kept"] for st in cpu.stats()) > 64, cpu.stats()
        cpu.close()
    assert len(mesh["idx"]) % 256 != 0   # the kernel's last workgroup is partial


def test_python_layer_rejects_bad_skins(small_synthetic):
    import tiny_renderer_amd as T
    from tiny_renderer_amd import _lib
    from tiny_renderer_amd.scene import _mesh_struct
    mesh = small_synthetic[0]
    bones, weights = _rig(mesh)
    pal = _palette()
    with pytest.raises(ValueError):
        T.skin_mesh(mesh, bones[:-1], weights[:-1], pal)
    with pytest.raises(ValueError):
        T.skin_mesh(mesh, bones[:, :3], weights[:, :3], pal)
    with pytest.raises(ValueError):
        T.skin_mesh(mesh, bones, weights[:, :3], pal)
    with pytest.raises(ValueError):
        T.skin_mesh(mesh, bones, weights, pal[:, :23])
    with pytest.raises(ValueError):
        T.skin_mesh(mesh, bones, weights, pal[:4])          # bone index 4 of a palette of four
    with pytest.raises(ValueError):
        T.skin_mesh(mesh, bones.astype(np.int64) - 1, weights, pal)
    with pytest.raises(ValueError):
        T.skin_mesh(mesh, bones, weights, np.zeros((129, 24), np.float32))
    # the C entry point itself
    L = _lib.load_library()
    keep = []
    m = _mesh_struct(mesh, keep)
    n9 = m.n_tri * 9
    op, on, oi = np.full(n9, 7, np.float32), np.full(n9, 7, np.float32), np.full(n9, 7, np.uint32)
    big = np.zeros((129, 24), np.float32)

    def call(n_bones, b, w, q, mm=m):
        return L.tr_skin_mesh(C.byref(mm) if mm is not None else None, n_bones, b.ctypes.data if b is not None else None,
                              w.ctypes.data if w is not None else None, q.ctypes.data if q is not None else None,
                              op.ctypes.data, on.ctypes.data, oi.ctypes.data)
    assert call(129, bones, weights, big) == _lib.TR_E_INVALID
    assert call(0, bones, weights, pal) == _lib.TR_E_INVALID
    assert call(4, bones, weights, pal) == _lib.TR_E_INVALID
    assert call(5, None, weights, pal) == _lib.TR_E_INVALID
    assert call(5, bones, None, pal) == _lib.TR_E_INVALID
    assert call(5, bones, weights, None) == _lib.TR_E_INVALID
    assert call(5, bones, weights, pal, None) == _lib.TR_E_INVALID
    assert (op == 7).all() and (on == 7).all() and (oi == 7).all()   # nothing written
    assert call(5, bones, weights, pal) == 0


# --- GPU ----------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("pipe", ALL)
def test_skinned_scene_equals_skinned_mesh_and_oracle(small_synthetic, pipe):
    import tiny_renderer_amd as T
    from tests.test_gpu_parity import assert_parity
    mesh, texs = small_synthetic
    sk = _skinned(mesh, _palette())
    s = _skinning(T, W, HH, mesh, texs, pipe, winner_tap=True)
    s.set_bone_palette(_palette())
    ref = T.Scene(W, HH, sk, texs, pipe, winner_tap=True)
    for q in (s, ref):
        _frame(q)
    _assert_same(s, ref, pipe, winner=True)
    cpu, status = _oracle_frame(sk, texs, pipe, _default_q())
    assert status == 0
    assert_parity(s, cpu, pipe)
    cpu.close()
    for q in (s, ref):
        q.close()


@pytest.mark.gpu
@pytest.mark.parametrize("pipe", ["phong", "shadow"])
def test_render_frames_skinned_groups(small_synthetic, pipe):
    import tiny_renderer_amd as T
    mesh, texs = small_synthetic
    w, h, n = 320, 256, 9   # 2 x frames_per_launch + 1: the last group is partial
    p, pals = _params(n), _palettes(n)
    rig = _rig(mesh)
    fused = _skinning(T, w, h, mesh, texs, pipe, frames_per_launch=4)
    fused.render_frames(p, bone_palettes=pals)
    assert fused.frames_kept() == 4
    loop = _skinning(T, w, h, mesh, texs, pipe)
    for back in range(fused.frames_kept()):
        i = n - 1 - back
        sk = _skinned(mesh, pals[i], rig)
        fused.select_frame(back)
        loop.set_bone_palette(pals[i])
        _frame_p(loop, p[i])
        ref = T.Scene(w, h, sk, texs, pipe)
        _frame_p(ref, p[i])
        cpu, status = _oracle_frame(sk, texs, pipe, p[i], w, h)
        assert status == 0
        _assert_oracle(fused, cpu, pipe)
        _assert_same(fused, ref, pipe)
        _assert_same(loop, ref, pipe)
        cpu.close()
        ref.close()
    # a kept frame's palette comes back with it: a later render without a clear accumulates under it
    fused.select_frame(2)
    ref2 = T.Scene(w, h, _skinned(mesh, pals[n - 3], rig), texs, pipe)
    _frame_p(ref2, p[n - 3])
    for s in (fused, ref2):
        s.set_light_direction(H.light(0.1))
        s.set_camera(*H.camera(0.2))
        s.render()
    _assert_same(fused, ref2, pipe)
    # plain render_frames draws the current palette in every frame
    fused.set_bone_palette(pals[1])
    fused.render_frames(p)
    ref3 = T.Scene(w, h, _skinned(mesh, pals[1], rig), texs, pipe)
    for back in (0, 3):
        fused.select_frame(back)
        _frame_p(ref3, p[n - 1 - back])
        _assert_same(fused, ref3, pipe)
    for s in (fused, loop, ref2, ref3):
        s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("pipe", ["phong", "darboux"])
def test_one_bone_of_weight_one_is_an_instance_transform(small_synthetic, pipe):
    import tiny_renderer_amd as T
    mesh, texs = small_synthetic
    n_pos = np.asarray(mesh["pos"]).reshape(-1, 3).shape[0]
    entry = _table()[6:7]   # the mirror
    s = T.Scene(320, 256, mesh, texs, pipe)
    s.set_skin(np.zeros((n_pos, 4), np.uint32), np.tile(np.array([1, 0, 0, 0], np.float32), (n_pos, 1)))
    assert s.n_bones == 1
    s.set_bone_palette(entry)
    ref = T.Scene(320, 256, mesh, texs, pipe, instance_transforms=entry)
    for q in (s, ref):
        _frame(q)
    _assert_same(s, ref, pipe)
    for q in (s, ref):
        q.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["none", "offset_scale", "transform"])
def test_morph_then_skin_then_table(small_synthetic, kind):
    import tiny_renderer_amd as T
    from tests.test_instancing import TABLE
    mesh, texs = small_synthetic
    pipe = "phong"
    both = _skinned(_posed(mesh, POSE), _palette(), _rig(mesh))   # (the rig is the mesh's, not the morphed positions')
    s = _skinning(T, W, HH, mesh, texs, pipe, winner_tap=True)
    s.set_morph_targets(*_targets(mesh))   # (leaves the skin alone)
    if kind == "offset_scale":
        s.set_bone_palette(_palette())
        s.set_morph_weights(POSE)
        s.set_instances(TABLE)
        both = T.apply_instances(both, TABLE)
    elif kind == "transform":
        s.set_instance_transforms(_table())
        s.set_morph_weights(POSE)
        s.set_bone_palette(_palette())
        both = T.apply_instance_transforms(both, _table())
    else:
        s.set_morph_weights(POSE)
        s.set_bone_palette(_palette())
    ref = T.Scene(W, HH, both, texs, pipe, winner_tap=True)
    for q in (s, ref):
        _frame(q)
    _assert_same(s, ref, pipe, winner=True)
    if kind == "none":
        # the halves are independent: new weights keep the palette, no palette keeps the weights, new targets keep the palette
        s.set_morph_weights(None)
        r = T.Scene(W, HH, _skinned(mesh, _palette()), texs, pipe, winner_tap=True)
        for q in (s, r):
            _frame(q)
        _assert_same(s, r, pipe, winner=True)
        r.close()
        s.set_morph_weights(POSE)
        s.set_bone_palette(None)
        r = T.Scene(W, HH, _posed(mesh, POSE), texs, pipe, winner_tap=True)
        for q in (s, r):
            _frame(q)
        _assert_same(s, r, pipe, winner=True)
        r.close()
        # through the fused path: a palette per frame under the current morph pose
        g = _skinning(T, 320, 256, mesh, texs, pipe, frames_per_launch=4)
        g.set_morph_targets(*_targets(mesh))
        g.set_morph_weights(POSE)
        p, pals = _params(5), _palettes(5)
        g.render_frames(p, bone_palettes=pals)
        for back in (0, 2):
            g.select_frame(back)
            r = T.Scene(320, 256, _skinned(_posed(mesh, POSE), pals[4 - back], _rig(mesh)), texs, pipe)
            _frame_p(r, p[4 - back])
            _assert_same(g, r, pipe)
            r.close()
        g.close()
    for q in (s, ref):
        q.close()


@pytest.mark.gpu
def test_held_back_frames_keep_their_palette(small_synthetic):
    import torch
    import tiny_renderer_amd as T
    mesh, texs = small_synthetic
    w, h, pipe = 320, 256, "phong"
    steps = [0.0, None, 30.0, None, 0.0, 60.0]
    s = _skinning(T, w, h, mesh, texs, pipe)
    assert s.frames_per_launch > 1
    bufs = [torch.zeros(h * w * 3, dtype=torch.uint8, device="cuda") for _ in steps]
    for turn, buf in zip(steps, bufs):
        s.set_bone_palette(None if turn is None else _palette(turn=turn))
        s.set_frame_buffer_device(buf.data_ptr())
        _frame(s)
    s.set_bone_palette(_palette(turn=30.0))   # (changes nothing of what was issued)
    s.sync()
    torch.cuda.synchronize()
    base = T.Scene(w, h, mesh, texs, pipe)
    _frame(base)
    for turn, buf in zip(steps, bufs):
        got = buf.cpu().numpy().reshape(h, w, 3)
        assert got.any()
        if turn is None:
            assert np.array_equal(got, base.get_frame_buffer())
            continue
        ref = T.Scene(w, h, _skinned(mesh, _palette(turn=turn)), texs, pipe)
        _frame(ref)
        assert np.array_equal(got, ref.get_frame_buffer())
        assert not np.array_equal(got, base.get_frame_buffer())
        ref.close()
    s.close()
    base.close()


@pytest.mark.gpu
@pytest.mark.parametrize("fused", [False, True])
def test_enlarging_palette_under_a_small_bin_capacity(small_synthetic, fused):
    """Skinned frames that want more records than the pools hold (64; the CPU test asserts from the oracle that every one
    keeps more polygons): the internal re-render draws the same rows again -- skinned once."""
    import tiny_renderer_amd as T
    mesh, texs = small_synthetic
    w, h, pipe = 320, 256, "phong"
    big = _palette(scale=PAL_BIG)
    order = [_palette(), _palette(turn=30.0), big] if fused else [big]
    s = _skinning(T, w, h, mesh, texs, pipe, bin_capacity=64, frames_per_launch=4 if fused else 0)
    s.profile_enable(True)
    if fused:
        s.render_frames(np.stack([_default_q()] * 3), bone_palettes=np.stack(order))
    else:
        s.set_bone_palette(big)
        _frame(s)
    assert s.sync() == 0
    prof = s.profile_read()
    s.profile_enable(False)
    assert prof["k_tile"]["frames"] > len(order), prof["k_tile"]    # frames were rendered again ...
    assert prof["k_skin"]["frames"] == len(order), prof["k_skin"]   # ... from the rows skinned once
    for back, pal in enumerate(reversed(order)):
        if fused:
            s.select_frame(back)
        cpu, status = _oracle_frame(_skinned(mesh, pal), texs, pipe, _default_q(), w, h)
        assert status == 0
        _assert_oracle(s, cpu, pipe)
        cpu.close()
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n_bones", [1, 128])
def test_kernel_edges_of_the_bone_count(small_synthetic, n_bones):
    """One bone, and 128: the palette's 768 pieces are more than the workgroup's 256 lanes, and bone 127 is drawn.  The
    mesh's polygon count is no multiple of 256 (asserted on the CPU): the last workgroup is partial."""
    import tiny_renderer_amd as T
    mesh, texs = small_synthetic
    w, h, pipe = 320, 256, "phong"
    rig, pal, pal2 = _edge_case(mesh, n_bones)
    sk = _skinned(mesh, pal, rig)
    s = T.Scene(w, h, mesh, texs, pipe)
    s.set_skin(*rig, n_bones=n_bones)
    s.set_bone_palette(pal)
    ref = T.Scene(w, h, sk, texs, pipe)
    for q in (s, ref):
        _frame(q)
    _assert_same(s, ref, pipe)
    # ... and through the fused launch, two frames of different palettes
    g = T.Scene(w, h, mesh, texs, pipe, frames_per_launch=4)
    g.set_skin(*rig, n_bones=n_bones)
    g.render_frames(np.stack([_default_q()] * 2), bone_palettes=np.stack([pal2, pal]))
    _assert_same(g, ref, pipe)
    g.select_frame(1)
    ref2 = T.Scene(w, h, _skinned(mesh, pal2, rig), texs, pipe)
    _frame(ref2)
    _assert_same(g, ref2, pipe)
    for q in (s, ref, g, ref2):
        q.close()


@pytest.mark.gpu
def test_a_long_skinned_call_does_not_grow_the_row_pool(small_synthetic):
    """The bound of the morph pool holds for skinned rows: at most one set per frame slot (<= 32), per frame of the groups
    in flight (4 sets of groups x 4) and for the current state."""
    import tiny_renderer_amd as T
    mesh, texs = small_synthetic
    w, h, pipe, n = 128, 64, "phong", LONG_CALL
    p = _long_call(n)
    pals = np.stack([_long_palette(i) for i in range(n)])
    s = _skinning(T, w, h, mesh, texs, pipe, frames_per_launch=4)
    assert s.debug_morph_rows() == 0
    s.render_frames(p, bone_palettes=pals)
    bound = 32 + 4 * 4 + 1
    during = s.debug_morph_rows()
    assert 0 < during <= bound, during
    s.sync()
    s.render_frames(p, bone_palettes=pals)   # a second call takes its rows from the pool
    assert s.debug_morph_rows() <= bound
    rig = _rig(mesh)
    for back in (0, 2):
        s.select_frame(back)
        i = n - 1 - back
        ref = T.Scene(w, h, _skinned(mesh, pals[i], rig), texs, pipe)
        _frame_p(ref, p[i])
        _assert_same(s, ref, pipe)
        ref.close()
    held = s.debug_morph_rows()
    s.set_skin(None)    # waits for the device: what nobody holds goes back
    assert s.debug_morph_rows() <= min(held, 32 + 1)
    s.close()


@pytest.mark.gpu
def test_skin_errors_leave_skin_palette_and_frame(small_synthetic):
    import tiny_renderer_amd as T
    from tiny_renderer_amd import _lib
    mesh, texs = small_synthetic
    w, h, pipe = 256, 256, "phong"
    L = _lib.load_library()
    bones, weights = _rig(mesh)
    pal = _palette()
    s = _skinning(T, w, h, mesh, texs, pipe)
    s.set_bone_palette(pal)
    _frame(s)
    before = (s.get_frame_buffer(), s.read_z_f32().view(np.uint32))
    assert before[0].any()
    p = _params(1)
    bad = bones.copy()
    bad[3, 1] = N_BONES
    big = np.zeros((129, 24), np.float32)
    assert L.tr_scene_set_skin(s._h, 129, bones.ctypes.data, weights.ctypes.data) == _lib.TR_E_INVALID
    assert L.tr_scene_set_skin(s._h, N_BONES, bad.ctypes.data, weights.ctypes.data) == _lib.TR_E_INVALID
    assert L.tr_scene_set_skin(s._h, N_BONES, None, weights.ctypes.data) == _lib.TR_E_INVALID
    assert L.tr_scene_set_skin(s._h, N_BONES, bones.ctypes.data, None) == _lib.TR_E_INVALID
    assert L.tr_scene_set_skin(None, N_BONES, bones.ctypes.data, weights.ctypes.data) == _lib.TR_E_INVALID
    assert L.tr_scene_set_bone_palette(s._h, 4, pal.ctypes.data) == _lib.TR_E_INVALID
    assert L.tr_scene_set_bone_palette(s._h, 6, big.ctypes.data) == _lib.TR_E_INVALID
    assert L.tr_scene_set_bone_palette(s._h, N_BONES, None) == _lib.TR_E_INVALID
    assert L.tr_scene_set_bone_palette(None, N_BONES, pal.ctypes.data) == _lib.TR_E_INVALID
    assert L.tr_scene_render_frames_skinned(s._h, 1, p.ctypes.data, 4, pal.ctypes.data, None) == _lib.TR_E_INVALID
    assert L.tr_scene_render_frames_skinned(s._h, 1, p.ctypes.data, N_BONES, None, None) == _lib.TR_E_INVALID
    assert L.tr_scene_render_frames_skinned(None, 1, p.ctypes.data, N_BONES, pal.ctypes.data, None) == _lib.TR_E_INVALID
    with pytest.raises(ValueError):
        s.set_bone_palette(pal[:4])
    with pytest.raises(ValueError):
        s.set_skin(bad, weights, n_bones=N_BONES)
    with pytest.raises(ValueError):
        s.set_skin(bones, weights, n_bones=129)
    with pytest.raises(ValueError):
        s.set_skin(bones[:-1], weights[:-1])
    with pytest.raises(ValueError):
        s.render_frames(p, bone_palettes=np.stack([pal, pal]))
    with pytest.raises(ValueError):
        s.render_frames(p, bone_palettes=pal[None], morph_weights=np.zeros((1, 4), np.float32))
    assert s.n_bones == N_BONES
    _frame(s)
    assert np.array_equal(s.get_frame_buffer(), before[0]) and np.array_equal(s.read_z_f32().view(np.uint32), before[1])
    ref = T.Scene(w, h, _skinned(mesh, pal), texs, pipe)
    _frame(ref)
    _assert_same(s, ref, pipe)
    # dropping the skin drops the palette: the mesh itself, and a palette is then an error
    s.set_skin(None)
    assert L.tr_scene_set_bone_palette(s._h, N_BONES, pal.ctypes.data) == _lib.TR_E_INVALID
    base = T.Scene(w, h, mesh, texs, pipe)
    for q in (s, base):
        _frame(q)
    _assert_same(s, base, pipe)
    for q in (s, ref, base):
        q.close()


@pytest.mark.gpu
def test_a_skin_without_a_palette_runs_no_kernel(small_synthetic):
    import tiny_renderer_amd as T
    mesh, texs = small_synthetic
    w, h, pipe = 256, 256, "phong"
    s = _skinning(T, w, h, mesh, texs, pipe)
    base = T.Scene(w, h, mesh, texs, pipe)
    s.profile_enable(True)
    _frame(s)
    s.render_frames(_params(3))
    s.select_frame(2)
    assert s.sync() == 0
    prof = s.profile_read()
    assert prof.get("k_skin", {"launches": 0})["launches"] == 0, prof
    assert prof["k_tile"]["launches"] > 0
    _frame_p(base, _params(3)[0])
    _assert_same(s, base, pipe)
    # with a palette it does run; set and then dropped again it does not
    s.set_bone_palette(_palette())
    _frame(s)
    assert s.sync() == 0
    assert s.profile_read()["k_skin"]["launches"] == 1
    s.set_bone_palette(None)
    _frame(s)
    _frame(base)
    assert s.sync() == 0
    assert s.profile_read()["k_skin"]["launches"] == 1   # (the counts accumulate: no second launch)
    s.profile_enable(False)
    _assert_same(s, base, pipe)
    for q in (s, base):
        q.close()
