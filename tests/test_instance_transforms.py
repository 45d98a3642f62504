"""Instance transforms (tr_scene_set_instance_transforms, tr_scene_render_frames_transformed,
tr_instance_transform_mesh): a scene drawing a transform table must render bit for bit what a scene created from the
concatenated mesh transformed on the host renders -- rgb, z bits, shadow bits, winner index.  Everything here is exact
equality of bits; no tolerance appears anywhere."""
import ctypes as C
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from tests import helpers as H

ALL = ("default", "phong", "normal_map", "specular", "darboux", "shadow", "occlusion")
W, HH = 640, 480


def _rot(yaw, pitch=0.0, roll=0.0):
    """Ry(yaw) Rx(pitch) Rz(roll), degrees, float64."""
    y, p, r = np.deg2rad([yaw, pitch, roll])
    ry = np.array([[np.cos(y), 0, np.sin(y)], [0, 1, 0], [-np.sin(y), 0, np.cos(y)]])
    rx = np.array([[1, 0, 0], [0, np.cos(p), -np.sin(p)], [0, np.sin(p), np.cos(p)]])
    rz = np.array([[np.cos(r), -np.sin(r), 0], [np.sin(r), np.cos(r), 0], [0, 0, 1]])
    return ry @ rx @ rz


def _table():
    """The table of the GPU tests: 0 a yaw, 1 a general rotation, 2 identical to 1 (z ties across instances), 3 entirely
    off screen, 4 a non-uniform scale under a rotation, 5 a shear, 6 a mirror (det < 0: the winding flips)."""
    import tiny_renderer_amd as T
    lin = [_rot(40) * 0.45,
           _rot(70, 25, -15) * 0.5,
           _rot(70, 25, -15) * 0.5,
           _rot(10) * 0.5,
           _rot(-30, 20, 0) @ np.diag([0.5, 0.3, 0.4]),
           np.array([[0.4, 0.15, 0.0], [0.0, 0.4, 0.1], [0.0, 0.0, 0.4]]),
           _rot(15, -10, 5) @ np.diag([-0.35, 0.35, 0.35])]
    off = [[-0.45, -0.30, 0.00], [0.35, 0.20, 0.10], [0.35, 0.20, 0.10], [6.00, 5.00, 0.00], [-0.25, 0.45, -0.20],
           [0.50, -0.45, 0.00], [-0.55, 0.50, 0.10]]
    t = T.instance_transforms(np.array(lin), np.array(off))
    assert np.linalg.det(t[6, 0:12].reshape(3, 4)[:, :3].astype(np.float64)) < 0
    assert np.array_equal(t[1].view(np.uint32), t[2].view(np.uint32))
    return t


OFF_SCREEN = 3


def _wrong_normals_table():
    """A 90 degree yaw whose `n` is the identity instead of the inverse transpose, and the proper table beside it."""
    import tiny_renderer_amd as T
    proper = T.instance_transforms(np.array([_rot(90) * 0.8]), np.array([[0.05, -0.02, 0.0]]))
    wrong = proper.copy()
    wrong[0, 12:21] = np.eye(3, dtype=np.float32).reshape(9)
    return wrong, proper


def _crowd(n_frames, n=5):
    """A crowd turning by four degrees per frame: [n_frames, n, 24]."""
    import tiny_renderer_amd as T
    off = np.array([[-0.5, -0.3, 0.0], [0.0, 0.35, 0.1], [0.5, -0.3, -0.1], [-0.2, 0.1, 0.2], [0.3, 0.0, 0.0]])[:n]
    scale = np.array([0.4, 0.45, 0.35, 0.3, 0.5])[:n]
    return np.stack([T.rotation_instances(np.deg2rad(20.0 * np.arange(n) + 4.0 * f), np.deg2rad(3.0 * f), 0.0, off, scale)
                     for f in range(n_frames)])


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


def _assert_same(a, b, pipe, winner=False):
    za, zb = a.read_z_f32().view(np.uint32), b.read_z_f32().view(np.uint32)
    assert np.array_equal(za, zb), "z bits differ at %d pixels" % int((za != zb).sum())
    if pipe in ("shadow", "occlusion"):
        sa, sb = a.read_shadow_f32().view(np.uint32), b.read_shadow_f32().view(np.uint32)
        assert np.array_equal(sa, sb), "shadow bits differ at %d pixels" % int((sa != sb).sum())
    if winner:
        wa, wb = a.read_winner_u32(), b.read_winner_u32()
        assert np.array_equal(wa, wb), "winner differs at %d pixels" % int((wa != wb).sum())
        assert (wa != 0xFFFFFFFF).any()
    fa, fb = a.get_frame_buffer(), b.get_frame_buffer()
    assert np.array_equal(fa, fb), "rgb differs at %d pixels" % int((fa != fb).any(-1).sum())
    assert fa.any(), "empty frame"


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _oracle_frame(mesh, texs, pipe, q, w=W, h=HH):
    from oracle import oracle as O
    cpu = O.Scene(w, h, mesh, texs, pipe)
    cpu.clear()
    cpu.set_light_direction(q[0:3])
    cpu.set_camera(q[3:6], q[6:9], q[9:12])
    status = cpu.render()
    return cpu, status


def _default_q(cam=0.3, light=0.7):
    return np.concatenate([np.asarray(H.light(light), np.float32)] + [np.asarray(v, np.float32) for v in H.camera(cam)])


# --- CPU ----------------------------------------------------------------------------------------

def test_transform_symbols_declared_exported_typed(built):
    import tiny_renderer_amd as T
    from tiny_renderer_amd import _lib
    assert C.sizeof(_lib.InstanceXform) == 96
    assert [f[0] for f in _lib.InstanceXform._fields_] == ["m", "n", "pad"]
    hdr = open(os.path.join(H.REPO, "include", "tiny_renderer.h")).read()
    assert "typedef struct tr_instance_xform" in hdr and "float m[12];" in hdr and "float n[9];" in hdr
    lib = C.CDLL(T.library_path())
    want = {
        "tr_scene_set_instance_transforms": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p]),
        "tr_scene_render_frames_transformed": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]),
        "tr_instance_transform_mesh": (C.c_int, [C.POINTER(_lib.Mesh), C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
    }
    for name, sig in want.items():
        assert name + "(" in hdr.replace(" (", "(")
        assert hasattr(lib, name)
        assert _lib.SYMBOLS[name] == sig
    assert T.load_library().tr_abi_version() == 3
    assert "#define TR_ABI_VERSION 3 " in hdr


def _rule_table():
    """The GPU tests' table (rotations, a non-uniform scale, a shear, a mirror) plus entries containing -0.0 and an entry
    whose products cancel exactly (x' = 0.5 x - 0.5 y: +0.0 wherever x == y, and z' = -0.0 * ... sums of signed zeros)."""
    t = _table()
    extra = np.zeros((3, 24), np.float32)
    extra[0, 0:12] = [1.0, -0.0, 0.0, -0.0, -0.0, 1.0, -0.0, 0.0, 0.0, 0.0, -1.0, -0.0]
    extra[0, 12:21] = [1.0, -0.0, -0.0, 0.0, 1.0, 0.0, -0.0, -0.0, -1.0]
    extra[1, 0:12] = [0.5, -0.5, 0.0, 0.0, 0.25, 0.25, -0.5, 0.0, -0.0, -0.0, -0.0, -0.0]
    extra[1, 12:21] = [0.5, -0.5, 0.0, 1.0, 1.0, -2.0, -0.0, -0.0, -0.0]
    extra[2, 0:12] = [3.0, 0.0, 0.0, -3.0, 0.0, -2.0, 0.0, 2.0, 0.0, 0.0, 1.0, -1.0]   # x' = 3x - 3: 0 at x = 1
    extra[2, 12:21] = np.eye(3, dtype=np.float32).reshape(9)
    return np.concatenate([t, extra])


def _cancel_mesh():
    """Vertices on which _rule_table's last entries cancel exactly: x == y, x + y == 2 z, x == 1, signed zeros."""
    pos = np.array([[0.3, 0.3, 0.3], [-0.7, -0.7, -0.7], [1.0, -1.0, 1.0], [-0.0, 0.0, -0.0], [0.0, -0.0, 0.0],
                    [0.1, 0.5, 0.3], [1.0, 1.0, 1.0], [-0.0, -0.0, -0.0]], np.float32)
    nrm = np.array([[0.6, 0.6, 0.6], [-0.0, 0.0, 1.0], [0.0, -1.0, -0.0], [0.25, 0.25, 0.25]], np.float32)
    idx = np.array([[0, 0, 0, 1, 0, 1, 2, 0, 2], [3, 0, 3, 4, 0, 0, 5, 0, 1], [5, 0, 2, 6, 0, 3, 7, 0, 0]], np.uint32)
    return {"pos": pos, "tex": np.zeros((1, 3), np.float32), "nrm": nrm, "idx": idx}


def _rule_meshes(small_synthetic):
    meshes = {"small_synthetic": small_synthetic[0], "cancel": _cancel_mesh()}
    src = os.path.join(H.FIXTURES, "diablo.obj.xz")
    assert os.path.isfile(src), "the diablo fixture is part of the repository"
    import lzma
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        with lzma.open(src, "rb") as fi, open(os.path.join(d, "model.obj"), "wb") as fo:
            fo.write(fi.read())
        meshes["diablo"] = H.load_obj_py(os.path.join(d, "model.obj"))
    return meshes


def test_host_rule_equals_numpy_bit_for_bit(small_synthetic):
    import tiny_renderer_amd as T
    table = _rule_table()
    assert np.signbit(table[table == 0.0]).any()
    for name, mesh in _rule_meshes(small_synthetic).items():
        pos, nrm = T.transform_mesh(mesh, table)
        cat = T.apply_instance_transforms(mesh, table)
        assert pos.shape == cat["pos"].shape and nrm.shape == cat["nrm"].shape, name
        assert np.array_equal(_bits(pos), _bits(cat["pos"])), "%s: %d position words differ" % (name, int((_bits(pos) != _bits(cat["pos"])).sum()))
        assert np.array_equal(_bits(nrm), _bits(cat["nrm"])), "%s: %d normal words differ" % (name, int((_bits(nrm) != _bits(cat["nrm"])).sum()))
        n_pos, n_nrm, n_tri = len(mesh["pos"]), len(mesh["nrm"]), len(mesh["idx"])
        idx = np.asarray(mesh["idx"], np.uint32)
        for k in range(len(table)):
            got = cat["idx"][k * n_tri:(k + 1) * n_tri]
            assert np.array_equal(got[:, 0::3], idx[:, 0::3] + k * n_pos)
            assert np.array_equal(got[:, 1::3], idx[:, 1::3])
            assert np.array_equal(got[:, 2::3], idx[:, 2::3] + k * n_nrm)
    # the exact cancellations really happen on the cancel mesh: +0.0 from x == y under (0.5, -0.5, 0)
    pos, _ = T.transform_mesh(_cancel_mesh(), table)
    k, n_pos = len(table) - 2, len(_cancel_mesh()["pos"])
    assert _bits(pos[k * n_pos + 0, 0:1])[0] == 0 and _bits(pos[k * n_pos + 1, 0:1])[0] == 0
    assert _bits(pos[(k + 1) * n_pos + 6, 0:1])[0] == 0   # 3 * 1 - 3


def _fused_like(mesh, table):
    """The rule evaluated as a fusing implementation would: each product enters its sum unrounded (the product of two
    float32 is exact in float64), one rounding to float32 per step."""
    pos = np.asarray(mesh["pos"], np.float32).astype(np.float64)
    out = []
    for e in np.asarray(table, np.float32):
        m = e[0:12].astype(np.float64)
        p = np.empty((len(pos), 3), np.float32)
        for r in range(3):
            t = (m[4 * r] * pos[:, 0]).astype(np.float32)
            t = (m[4 * r + 1] * pos[:, 1] + t.astype(np.float64)).astype(np.float32)
            t = (m[4 * r + 2] * pos[:, 2] + t.astype(np.float64)).astype(np.float32)
            p[:, r] = (t.astype(np.float64) + m[4 * r + 3]).astype(np.float32)
        out.append(p)
    return np.concatenate(out)


def test_a_fusing_implementation_would_be_noticed(small_synthetic):
    """The companion of the case above: for the chosen table and mesh, contracting products into sums changes bits, so
    bit equality with apply_instance_transforms does pin the absence of FMA."""
    import tiny_renderer_amd as T
    mesh, table = small_synthetic[0], _table()
    pos, _ = T.transform_mesh(mesh, table)
    fused = _fused_like(mesh, table)
    differ = int((_bits(pos) != _bits(fused)).sum())
    assert differ > 0
    # ... and by rounding only: the two stay within a few ulps of each other
    assert np.allclose(pos, fused, rtol=0, atol=1e-5)


def _signed_zero_mesh(mesh):
    m = dict(mesh)
    pos = np.array(mesh["pos"], np.float32, copy=True)
    pos[:, 0][pos[:, 0] == 0.0] = np.float32(-0.0)
    assert np.signbit(pos[:, 0]).any()
    m["pos"] = pos
    return m


def _as_transforms(table4):
    """An offset/scale table as a transform table: linear part scale * I with off-diagonals +0.0, n = I."""
    t = np.zeros((len(table4), 24), np.float32)
    for k, (ox, oy, oz, sc) in enumerate(np.asarray(table4, np.float32)):
        t[k, 0:12] = [sc, 0, 0, ox, 0, sc, 0, oy, 0, 0, sc, oz]
        t[k, 12:21] = np.eye(3, dtype=np.float32).reshape(9)
    return t


def test_identity_and_pure_placements_reproduce_apply_instances(small_synthetic):
    """Where the two rules coincide.  With off-diagonals +0.0 the transform rule is ((s p + (+-0)) + (+-0)) + o: the signed
    zeros leave a non-zero s p alone, and a zero s p of either sign plus o gives o for o != 0 and +0.0 for o = +0.0 -- what
    fl(fl(p s) + o) gives too.  Only o = -0.0 could tell them apart (-0 + -0 = -0 against +0 + -0 = +0), so the inputs
    are: finite meshes (zeros of both signs included), finite tables whose offsets are not -0.0."""
    import tiny_renderer_amd as T
    from tests.test_instancing import TABLE
    mesh = _signed_zero_mesh(small_synthetic[0])
    for table4 in (np.array([[0.0, 0.0, 0.0, 1.0]], np.float32), TABLE, T.grid_instances(3)):
        assert not np.signbit(table4[:, 0:3][table4[:, 0:3] == 0.0]).any()
        want = T.apply_instances(mesh, table4)
        got = T.apply_instance_transforms(mesh, _as_transforms(table4))
        assert np.array_equal(_bits(got["pos"]), _bits(want["pos"]))
        assert np.array_equal(got["idx"][:, 0::3], want["idx"][:, 0::3])
        assert np.array_equal(got["idx"][:, 1::3], want["idx"][:, 1::3])
        pos, nrm = T.transform_mesh(mesh, _as_transforms(table4))
        assert np.array_equal(_bits(pos), _bits(want["pos"]))
        # n = I leaves every normal's value (a -0.0 component may come out as +0.0: (1 a + 0 b) + 0 c)
        assert np.array_equal(nrm, np.tile(np.asarray(mesh["nrm"], np.float32), (len(table4), 1)))
    # the -0.0 -> +0.0 behaviour of {0, 0, 0, 1} itself
    one = T.apply_instance_transforms(mesh, _as_transforms(np.array([[0.0, 0.0, 0.0, 1.0]], np.float32)))
    zeros = mesh["pos"] == 0.0
    assert np.signbit(mesh["pos"][zeros]).any() and not np.signbit(one["pos"][zeros]).any()
    assert np.array_equal(one["pos"], mesh["pos"])


def test_python_table_builders():
    import tiny_renderer_amd as T
    lin = np.array([_rot(30, 10, 5) * 0.5, np.diag([2.0, 1.0, -0.5])])
    t = T.instance_transforms(lin, [[1, 2, 3], [4, 5, 6]])
    assert t.shape == (2, 24) and t.dtype == np.float32
    for k in range(2):
        m = t[k, 0:12].reshape(3, 4)
        assert np.array_equal(m[:, :3], lin[k].astype(np.float32)) and np.array_equal(m[:, 3], np.float32([1, 2, 3]) + 3 * k)
        want = np.linalg.inv(lin[k].astype(np.float32).astype(np.float64)).T.astype(np.float32)
        assert np.array_equal(_bits(t[k, 12:21]), _bits(want.reshape(9)))
        assert not t[k, 21:].any()
    with pytest.raises(ValueError):
        T.instance_transforms(np.array([[[1.0, 2.0, 3.0], [2.0, 4.0, 6.0], [0.0, 0.0, 1.0]]]), [[0, 0, 0]])
    r = T.rotation_instances(np.deg2rad([0.0, 90.0]), 0.0, 0.0, [[0, 0, 0], [1, 0, 0]], [1.0, 2.0])
    assert np.allclose(r[0, 0:12].reshape(3, 4), np.eye(3, 4), atol=1e-7)
    assert np.allclose(r[1, 0:12].reshape(3, 4), [[0, 0, 2, 1], [0, 2, 0, 0], [-2, 0, 0, 0]], atol=1e-6)   # +z turns to +x
    assert np.allclose(r[1, 12:21].reshape(3, 3), [[0, 0, 0.5], [0, 0.5, 0], [-0.5, 0, 0]], atol=1e-6)
    from tiny_renderer_amd.cli import yawed_grid
    g = yawed_grid(T, 2, 30.0)
    grid = T.grid_instances(2)
    assert g.shape == (4, 24) and np.array_equal(g[:, [3, 7, 11]], grid[:, 0:3])
    assert np.allclose(g[3, 0:12].reshape(3, 4)[:, :3], _rot(90) * 0.5, atol=1e-6)


def test_scene_rejects_two_tables_and_bad_shapes(small_synthetic):
    """What the Python layer rules out before anything reaches the GPU."""
    import tiny_renderer_amd as T
    mesh, texs = small_synthetic
    with pytest.raises(ValueError):
        T.Scene(64, 64, mesh, texs, "phong", instances=T.grid_instances(2), instance_transforms=_table())
    with pytest.raises(ValueError):
        T.transform_mesh(mesh, np.zeros((2, 12), np.float32))


def _winning_instances(cpu, n_tri):
    w = cpu.winner_u32()
    return np.unique(w[w != 0xFFFFFFFF] // n_tri)


def test_oracle_draws_every_table_of_the_gpu_tests(small_synthetic, synthetic):
    """A GPU parity test could pass on two empty frames: every table the GPU tests draw gives the oracle, on the
    concatenated mesh, status 0 and a frame with pixels.  The main table: at least four instances own winning pixels,
    one lies entirely off screen, two entries are identical."""
    import tiny_renderer_amd as T
    mesh, texs = small_synthetic
    n_tri = len(mesh["idx"])
    table = _table()
    for pipe in ("phong", "darboux", "shadow"):
        cpu, status = _oracle_frame(T.apply_instance_transforms(mesh, table), texs, pipe, _default_q())
        assert status == 0
        who = _winning_instances(cpu, n_tri)
        assert len(who) >= 4 and OFF_SCREEN not in who, who
        assert 6 in who, "the mirrored instance draws nothing"
        assert cpu.get_frame_buffer().any()
        cpu.close()
    assert np.array_equal(table[1], table[2])
    for t in _wrong_normals_table():
        for pipe in ("phong", "darboux"):
            cpu, status = _oracle_frame(T.apply_instance_transforms(mesh, t), texs, pipe, _default_q())
            assert status == 0 and cpu.get_frame_buffer().any() and len(_winning_instances(cpu, n_tri)) == 1
            cpu.close()
    n = 9
    p, crowd = _params(n), _crowd(n)
    for i in range(n):
        cpu, status = _oracle_frame(T.apply_instance_transforms(mesh, crowd[i]), texs, "phong", p[i], 320, 256)
        assert status == 0 and len(_winning_instances(cpu, n_tri)) >= 4
        cpu.close()
    big, big_texs = synthetic
    cpu, status = _oracle_frame(T.apply_instance_transforms(big, table), big_texs, "phong", _default_q(0.0, 0.0), 1024, 512)
    assert status == 0 and len(_winning_instances(cpu, len(big["idx"]))) >= 4
    cpu.close()


# --- GPU ----------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("pipe", ALL)
def test_transformed_equals_concatenated_mesh(small_synthetic, pipe):
    import tiny_renderer_amd as T
    mesh, texs = small_synthetic
    table = _table()
    cat = T.apply_instance_transforms(mesh, table)
    inst = T.Scene(W, HH, mesh, texs, pipe, winner_tap=True, instance_transforms=table)
    ref = T.Scene(W, HH, cat, texs, pipe, winner_tap=True)
    for s in (inst, ref):
        _frame(s)
    _assert_same(inst, ref, pipe, winner=True)
    who = np.unique(inst.read_winner_u32()[inst.read_winner_u32() != 0xFFFFFFFF] // len(mesh["idx"]))
    assert len(who) >= 4 and 6 in who
    if pipe in ("phong", "darboux", "shadow"):
        from tests.test_gpu_parity import assert_parity
        cpu, status = _oracle_frame(cat, texs, pipe, _default_q())
        assert status == 0
        assert_parity(inst, cpu, pipe)
        cpu.close()
    inst.close()
    ref.close()


@pytest.mark.gpu
@pytest.mark.parametrize("pipe", ["phong", "darboux"])
def test_the_callers_normal_transform_is_what_is_drawn(small_synthetic, pipe):
    """`n` is the caller's: a table whose n is the identity under a 90 degree yaw draws the concatenated mesh built with
    THAT n -- and not the one built with the inverse transpose (an implementation that ignored n, or derived it)."""
    import tiny_renderer_amd as T
    mesh, texs = small_synthetic
    wrong, proper = _wrong_normals_table()
    s = T.Scene(W, HH, mesh, texs, pipe, winner_tap=True, instance_transforms=wrong)
    ref = T.Scene(W, HH, T.apply_instance_transforms(mesh, wrong), texs, pipe, winner_tap=True)
    other = T.Scene(W, HH, T.apply_instance_transforms(mesh, proper), texs, pipe, winner_tap=True)
    for q in (s, ref, other):
        _frame(q)
    _assert_same(s, ref, pipe, winner=True)
    assert np.array_equal(s.read_z_f32().view(np.uint32), other.read_z_f32().view(np.uint32))   # the same geometry ...
    assert not np.array_equal(s.get_frame_buffer(), other.get_frame_buffer())                   # ... lit differently
    s.set_instance_transforms(proper)
    _frame(s)
    _assert_same(s, other, pipe, winner=True)
    for q in (s, ref, other):
        q.close()


@pytest.mark.gpu
@pytest.mark.parametrize("pipe", ["phong", "shadow"])
def test_render_frames_transformed_groups(small_synthetic, pipe):
    import tiny_renderer_amd as T
    mesh, texs = small_synthetic
    w, h, n = 320, 256, 9   # 2 x frames_per_launch + 1
    p, crowd = _params(n), _crowd(n)
    fused = T.Scene(w, h, mesh, texs, pipe, frames_per_launch=4)
    fused.render_frames(p, instance_transforms=crowd)
    assert fused.frames_kept() == 4
    loop = T.Scene(w, h, mesh, texs, pipe)
    for back in range(fused.frames_kept()):
        i = n - 1 - back
        fused.select_frame(back)
        loop.set_instance_transforms(crowd[i])
        _frame_p(loop, p[i])
        ref = T.Scene(w, h, T.apply_instance_transforms(mesh, crowd[i]), texs, pipe)
        _frame_p(ref, p[i])
        _assert_same(fused, ref, pipe)
        _assert_same(loop, ref, pipe)
        ref.close()
    # a group followed by a plain render() without clear: the last frame's table is current, the frame accumulates
    fused.render_frames(p, instance_transforms=crowd)
    ref = T.Scene(w, h, T.apply_instance_transforms(mesh, crowd[n - 1]), texs, pipe)
    _frame_p(ref, p[n - 1])
    for s in (fused, ref):
        s.set_camera(*H.camera(1.1))
        s.render()
    _assert_same(fused, ref, pipe)
    # a kept frame's table comes back with it
    fused.render_frames(p, instance_transforms=crowd)
    fused.select_frame(2)
    _frame(fused, cam=0.2, light=0.1)
    ref2 = T.Scene(w, h, T.apply_instance_transforms(mesh, crowd[n - 3]), texs, pipe)
    _frame(ref2, cam=0.2, light=0.1)
    _assert_same(fused, ref2, pipe)
    for s in (fused, loop, ref, ref2):
        s.close()


@pytest.mark.gpu
def test_table_kinds_alternate_with_held_back_frames(small_synthetic):
    """Offset/scale and transform tables from one call to the next, on a scene that holds cleared frames back to fuse
    them: every frame keeps the table, and the kind of table, it was issued with."""
    import torch
    import tiny_renderer_amd as T
    from tests.test_instancing import TABLE
    mesh, texs = small_synthetic
    w, h, pipe = 320, 256, "phong"
    table = _table()
    steps = [("x", table), ("o", TABLE), ("x", table[[6, 0, 5]]), ("o", TABLE[[4, 0]]), ("x", _crowd(1)[0]), ("none", None)]
    s = T.Scene(w, h, mesh, texs, pipe)
    assert s.frames_per_launch > 1
    s.set_instance_transforms(table)   # (the largest table first: nothing grows later, frames stay held back)
    bufs = [torch.zeros(h * w * 3, dtype=torch.uint8, device="cuda") for _ in steps]
    for (kind, t), buf in zip(steps, bufs):
        if kind == "x":
            s.set_instance_transforms(t)
        else:
            s.set_instances(t)
        s.set_frame_buffer_device(buf.data_ptr())
        _frame(s)
    s.sync()
    torch.cuda.synchronize()
    for (kind, t), buf in zip(steps, bufs):
        cat = T.apply_instance_transforms(mesh, t) if kind == "x" else T.apply_instances(mesh, t) if kind == "o" else mesh
        ref = T.Scene(w, h, cat, texs, pipe)
        _frame(ref)
        got = buf.cpu().numpy().reshape(h, w, 3)
        assert np.array_equal(got, ref.get_frame_buffer()), kind
        assert got.any()
        ref.close()
    # and through the fused path: a transformed call, an offset/scale call, a plain call drawing the table left current
    p = _params(5)
    g = T.Scene(w, h, mesh, texs, pipe, frames_per_launch=4)
    g.render_frames(p, instance_transforms=_crowd(5))
    g.render_frames(p, instances=np.stack([TABLE] * 5))
    ref = T.Scene(w, h, T.apply_instances(mesh, TABLE), texs, pipe)
    _frame_p(ref, p[4])
    _assert_same(g, ref, pipe)
    g.set_instance_transforms(table)
    g.render_frames(p)
    ref3 = T.Scene(w, h, T.apply_instance_transforms(mesh, table), texs, pipe)
    _frame_p(ref3, p[4])
    _assert_same(g, ref3, pipe)
    for q in (s, g, ref, ref3):
        q.close()


@pytest.mark.gpu
def test_transformed_band_scenes(synthetic):
    import tiny_renderer_amd as T
    mesh, texs = synthetic
    w, h, table = 1024, 512, _table()
    full = T.Scene(w, h, mesh, texs, "phong", instance_transforms=table)
    _frame(full, cam=0.0, light=0.0)
    want = full.get_frame_buffer()
    cat = T.Scene(w, h, T.apply_instance_transforms(mesh, table), texs, "phong")
    _frame(cat, cam=0.0, light=0.0)
    assert np.array_equal(want, cat.get_frame_buffer()) and want.any()
    full.close()
    cat.close()
    for band in ((0, 128), (256, 512)):
        b = T.Scene(w, h, mesh, texs, "phong", band_rows=band, instance_transforms=table)
        _frame(b, cam=0.0, light=0.0)
        got = b.get_frame_buffer()[band[0]:band[1]]
        assert np.array_equal(got, want[band[0]:band[1]]) and got.any()
        b.close()


@pytest.mark.gpu
def test_sharded_transformed_two_ranks_one_gpu(built):
    """Two rank processes of a ShardedScene on one GPU (the library's peer transport) draw transform tables -- per frame
    and through groups of frames -- and every rank compares the assembled frame with a single-GPU scene's:
    tests/sharded_xform_worker.py."""
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                        "--master-port", str(port), os.path.join(H.REPO, "tests", "sharded_xform_worker.py"), "peer"],
                       env=env, cwd=H.REPO, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "rank 0 OK" in r.stdout and "rank 1 OK" in r.stdout, (r.stdout[-1500:] + r.stderr[-4000:])


@pytest.mark.gpu
def test_transform_errors_leave_the_table(small_synthetic):
    import tiny_renderer_amd as T
    from tiny_renderer_amd import _lib
    mesh, texs = small_synthetic
    w, h, pipe = 256, 256, "phong"
    L = _lib.load_library()
    table = _table()
    s = T.Scene(w, h, mesh, texs, pipe, instance_transforms=table)
    _frame(s)
    before = (s.get_frame_buffer(), s.read_z_f32().view(np.uint32))
    assert before[0].any()
    n_tri = mesh["idx"].shape[0]
    too_many = 0xFFFFFFF0 // n_tri + 1
    one = np.zeros((1, 24), np.float32)
    p = _params(1)
    assert L.tr_scene_set_instance_transforms(s._h, 3, None) == _lib.TR_E_INVALID
    assert L.tr_scene_set_instance_transforms(s._h, too_many, one.ctypes.data) == _lib.TR_E_INVALID
    assert L.tr_scene_set_instance_transforms(None, 1, one.ctypes.data) == _lib.TR_E_INVALID
    assert L.tr_scene_render_frames_transformed(s._h, 1, p.ctypes.data, 3, None, None) == _lib.TR_E_INVALID
    assert L.tr_scene_render_frames_transformed(s._h, 1, p.ctypes.data, too_many, one.ctypes.data, None) == _lib.TR_E_INVALID
    assert L.tr_scene_render_frames_transformed(None, 1, p.ctypes.data, 1, one.ctypes.data, None) == _lib.TR_E_INVALID
    with pytest.raises(ValueError):
        s.set_instance_transforms(np.zeros((3, 4), np.float32))
    with pytest.raises(ValueError):
        s.render_frames(p, instances=np.zeros((1, 1, 4), np.float32), instance_transforms=np.zeros((1, 1, 24), np.float32))
    _frame(s)
    assert np.array_equal(s.get_frame_buffer(), before[0]) and np.array_equal(s.read_z_f32().view(np.uint32), before[1])
    ref = T.Scene(w, h, T.apply_instance_transforms(mesh, table), texs, pipe)
    _frame(ref)
    _assert_same(s, ref, pipe)
    s.close()
    ref.close()


@pytest.mark.gpu
def test_resolve_of_a_transformed_frame(small_synthetic):
    import tiny_renderer_amd as T
    mesh, texs = small_synthetic
    s = T.Scene(W, HH, mesh, texs, "phong", instance_transforms=_table())
    _frame(s)
    fb = s.get_frame_buffer()
    assert fb.any()
    want = ((fb.astype(np.uint32).reshape(HH // 2, 2, W // 2, 2, 3).sum(axis=(1, 3)) + 2) // 4).astype(np.uint8)
    assert np.array_equal(s.resolve(2), want)
    s.close()
