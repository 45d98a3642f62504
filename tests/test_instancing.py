"""Instanced rendering (tr_scene_set_instances, tr_scene_render_frames_instanced): a scene drawing an instance table
must render bit for bit what a scene created from the host-transformed, concatenated mesh renders -- rgb, z bits,
shadow bits, winner index."""
import ctypes as C

import numpy as np
import pytest

from tests import helpers as H

ALL = ("default", "phong", "normal_map", "specular", "darboux", "shadow", "occlusion")
# non-uniform offsets, scales other than 1/n, instances 1 and 2 identical (z ties across instances), instance 3 off
# screen, instance 4 overlapping instance 0
TABLE = np.array([[-0.45, -0.30, 0.00, 0.45],
                  [0.35, 0.20, 0.10, 0.60],
                  [0.35, 0.20, 0.10, 0.60],
                  [6.00, 5.00, 0.00, 0.50],
                  [-0.25, -0.15, -0.20, 0.33]], np.float32)


def _signed_zero_mesh(mesh):
    """The mesh with every zero x coordinate written as -0.0 (what a table of {0, 0, 0, 1} turns into +0.0)."""
    m = dict(mesh)
    pos = np.array(mesh["pos"], np.float32, copy=True)
    pos[:, 0][pos[:, 0] == 0.0] = np.float32(-0.0)
    assert np.signbit(pos[:, 0]).any()
    m["pos"] = pos
    return m


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


# --- CPU ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 3, 8])
def test_grid_instances_reproduce_instanced_grid(small_synthetic, n):
    import tiny_renderer_amd as T
    mesh, _ = small_synthetic
    table = T.grid_instances(n)
    assert table.dtype == np.float32 and table.shape == (n * n, 4)
    for i in range(n):
        for j in range(n):
            want = np.array([(2 * i + 1) / n - 1.0, (2 * j + 1) / n - 1.0, 0.0, 1.0 / n], np.float32)
            assert np.array_equal(table[i * n + j].view(np.uint32), want.view(np.uint32))
    grid = T.instanced_grid(mesh, n)
    # the library's rule, p * scale + offset with two float32 roundings, on the host
    pos = np.asarray(mesh["pos"], np.float32)
    rule = np.concatenate([(pos * t[3]).astype(np.float32) + t[:3] for t in table]).astype(np.float32)
    assert np.array_equal(rule.view(np.uint32), grid["pos"].view(np.uint32))
    cat = T.apply_instances(mesh, table)
    assert np.array_equal(cat["pos"].view(np.uint32), grid["pos"].view(np.uint32))
    assert np.array_equal(cat["idx"], grid["idx"])


def test_instancing_symbols_declared_exported_typed(built):
    import tiny_renderer_amd as T
    from tiny_renderer_amd import _lib
    assert C.sizeof(_lib.Instance) == 16
    assert [f[0] for f in _lib.Instance._fields_] == ["offset", "scale"]
    hdr = open(H.os.path.join(H.REPO, "include", "tiny_renderer.h")).read()
    assert "typedef struct tr_instance" in hdr
    lib = C.CDLL(T.library_path())
    want = {
        "tr_scene_set_instances": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p]),
        "tr_scene_render_frames_instanced": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p,
                                                       C.c_void_p]),
    }
    for name, sig in want.items():
        assert name + "(" in hdr.replace(" (", "(")
        assert hasattr(lib, name)
        assert _lib.SYMBOLS[name] == sig


# --- GPU ----------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("pipe", ALL)
def test_instanced_equals_concatenated_mesh(small_synthetic, pipe):
    import tiny_renderer_amd as T
    mesh, texs = small_synthetic
    cat = T.apply_instances(mesh, TABLE)
    W, Hh = 640, 480
    inst = T.Scene(W, Hh, mesh, texs, pipe, winner_tap=True, instances=TABLE)
    ref = T.Scene(W, Hh, cat, texs, pipe, winner_tap=True)
    for s in (inst, ref):
        _frame(s)
    _assert_same(inst, ref, pipe, winner=True)
    if pipe in ("phong", "shadow"):
        from oracle import oracle as O
        from tests.test_gpu_parity import assert_parity
        cpu = O.Scene(W, Hh, cat, texs, pipe)
        cpu.clear()
        cpu.set_light_direction(H.light(0.7))
        cpu.set_camera(*H.camera(0.3))
        assert cpu.render() == 0
        assert_parity(inst, cpu, pipe)
    inst.close()
    ref.close()


@pytest.mark.gpu
@pytest.mark.parametrize("store_depth", [False, True])
@pytest.mark.parametrize("pipe", ["phong", "shadow"])
def test_render_frames_instanced_groups(small_synthetic, pipe, store_depth):
    import tiny_renderer_amd as T
    mesh, texs = small_synthetic
    W, Hh, n = 320, 256, 11
    rng = np.random.default_rng(7)
    tables = np.empty((n, 4, 4), np.float32)
    tables[:, :, 0:2] = rng.uniform(-0.6, 0.6, (n, 4, 2))
    tables[:, :, 2] = rng.uniform(-0.2, 0.2, (n, 4))
    tables[:, :, 3] = rng.uniform(0.3, 0.7, (n, 4))
    p = _params(n)
    fused = T.Scene(W, Hh, mesh, texs, pipe, frames_per_launch=4, store_depth=store_depth)
    fused.render_frames(p, instances=tables)
    assert fused.frames_kept() == 4  # (11 frames: three groups)
    loop = T.Scene(W, Hh, mesh, texs, pipe, store_depth=store_depth)
    for back in range(fused.frames_kept()):
        i = n - 1 - back
        fused.select_frame(back)
        loop.set_instances(tables[i])
        loop.clear()
        loop.set_light_direction(p[i, 0:3])
        loop.set_camera(p[i, 3:6], p[i, 6:9], p[i, 9:12])
        loop.render()
        ref = T.Scene(W, Hh, T.apply_instances(mesh, tables[i]), texs, pipe)
        ref.clear()
        ref.set_light_direction(p[i, 0:3])
        ref.set_camera(p[i, 3:6], p[i, 6:9], p[i, 9:12])
        ref.render()
        _assert_same(fused, ref, pipe)
        _assert_same(loop, ref, pipe)
        ref.close()
    # the scene is left with the selected frame's table current: a render without a new table draws it
    fused.select_frame(0)
    _frame(fused, cam=0.2, light=0.1)
    ref = T.Scene(W, Hh, T.apply_instances(mesh, tables[n - 1]), texs, pipe)
    _frame(ref, cam=0.2, light=0.1)
    _assert_same(fused, ref, pipe)
    for s in (fused, loop, ref):
        s.close()


@pytest.mark.gpu
def test_held_back_frames_keep_their_table(small_synthetic):
    import torch
    import tiny_renderer_amd as T
    mesh, texs = small_synthetic
    W, Hh, pipe = 320, 256, "phong"
    a, b = TABLE, TABLE[[4, 0, 3]] * np.float32(1.25)
    s = T.Scene(W, Hh, mesh, texs, pipe)
    assert s.frames_per_launch > 1  # (cleared frames on the scene's own stream are held back to fuse them)
    x = torch.zeros(Hh * W * 3, dtype=torch.uint8, device="cuda")
    y = torch.zeros(Hh * W * 3, dtype=torch.uint8, device="cuda")
    s.set_instances(a)
    s.set_frame_buffer_device(x.data_ptr())
    _frame(s)
    s.set_frame_buffer_device(y.data_ptr())
    s.set_instances(b)  # (smaller than a: nothing grows, the first frame stays held back)
    _frame(s)
    s.sync()
    torch.cuda.synchronize()
    for buf, table in ((x, a), (y, b)):
        ref = T.Scene(W, Hh, T.apply_instances(mesh, table), texs, pipe)
        _frame(ref)
        got = buf.cpu().numpy().reshape(Hh, W, 3)
        assert np.array_equal(got, ref.get_frame_buffer())
        ref.close()
    s.close()


@pytest.mark.gpu
def test_tables_grow_and_shrink(small_synthetic):
    import tiny_renderer_amd as T
    mesh, texs = small_synthetic
    mesh = _signed_zero_mesh(mesh)
    W, Hh, pipe = 512, 384, "shadow"
    s = T.Scene(W, Hh, mesh, texs, pipe)
    grid8 = T.grid_instances(8)
    grid8[:, 3] = np.float32(0.11)
    for table in (np.array([[0.0, 0.0, 0.0, 1.0]], np.float32), grid8, TABLE[:4], None):
        s.set_instances(table)
        _frame(s)
        ref = T.Scene(W, Hh, mesh if table is None else T.apply_instances(mesh, table), texs, pipe)
        _frame(ref)
        _assert_same(s, ref, pipe)
        ref.close()
    s.close()


@pytest.mark.gpu
def test_instanced_band_scenes(synthetic):
    import tiny_renderer_amd as T
    mesh, texs = synthetic
    W, Hh = 1024, 512
    full = T.Scene(W, Hh, T.instanced_grid(mesh, 4), texs, "specular")
    _frame(full, cam=0.0, light=0.0)
    want = full.get_frame_buffer()
    full.close()
    for band in ((0, 128), (256, 512)):
        b = T.Scene(W, Hh, mesh, texs, "specular", band_rows=band, instances=T.grid_instances(4))
        _frame(b, cam=0.0, light=0.0)
        assert np.array_equal(b.get_frame_buffer()[band[0]:band[1]], want[band[0]:band[1]])
        b.close()


@pytest.mark.gpu
def test_configs4_full_size_instanced_vs_replicated(built):
    """BASELINE.json configs[4] (diablo x64 grid, -s specular, 8192^2): instanced against replicated, GPU vs GPU."""
    import tiny_renderer_amd as T
    loaded = H.load_assets_py("diablo")
    mesh, texs = loaded if loaded is not None else T.synthetic_scene()
    out = []
    for form in ("replicated", "instanced"):
        if form == "replicated":
            s = T.Scene(8192, 8192, T.instanced_grid(mesh, 8), texs, "specular")
        else:
            s = T.Scene(8192, 8192, mesh, texs, "specular", instances=T.grid_instances(8))
        _frame(s, cam=0.0, light=0.0)
        out.append((s.get_frame_buffer(), s.read_z_f32().view(np.uint32)))
        s.close()
    assert np.array_equal(out[0][1], out[1][1]), "z bits differ at %d pixels" % int((out[0][1] != out[1][1]).sum())
    assert np.array_equal(out[0][0], out[1][0])


@pytest.mark.gpu
def test_instance_errors_leave_the_table(small_synthetic):
    import tiny_renderer_amd as T
    from tiny_renderer_amd import _lib
    mesh, texs = small_synthetic
    W, Hh, pipe = 256, 256, "phong"
    L = _lib.load_library()
    s = T.Scene(W, Hh, mesh, texs, pipe, instances=TABLE)
    n_tri = mesh["idx"].shape[0]
    too_many = 0xFFFFFFF0 // n_tri + 1
    one = np.zeros((1, 4), np.float32)
    p = _params(1)
    assert L.tr_scene_set_instances(s._h, 3, None) == _lib.TR_E_INVALID
    assert L.tr_scene_set_instances(s._h, too_many, one.ctypes.data) == _lib.TR_E_INVALID
    assert L.tr_scene_render_frames_instanced(s._h, 1, p.ctypes.data, 3, None, None) == _lib.TR_E_INVALID
    assert L.tr_scene_render_frames_instanced(s._h, 1, p.ctypes.data, too_many, one.ctypes.data, None) == _lib.TR_E_INVALID
    with pytest.raises(ValueError):
        s.set_instances(np.zeros((3, 3), np.float32))
    _frame(s)
    ref = T.Scene(W, Hh, T.apply_instances(mesh, TABLE), texs, pipe)
    _frame(ref)
    _assert_same(s, ref, pipe)
    s.close()
    ref.close()
