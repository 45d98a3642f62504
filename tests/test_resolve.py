"""Supersampled output: tr_scene_resolve / tr_scene_get_resolved (k_resolve) against four lines of numpy.

The contract is integer and exact -- a box filter over f x f stored u8 values per channel, rounded half up -- so
every comparison is np.array_equal.  The oracle is `box` applied to the FULL-SIZE frame the scene itself returns
(tr_scene_get_frame_buffer), which the parity tests pin against the CPU oracle."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import helpers as H

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIPELINES = ("default", "phong", "normal_map", "specular", "darboux", "shadow", "occlusion")
FACTORS = (2, 4, 8)


def box(F, f):  # F: (H, W, 3) uint8
    H_, W, _ = F.shape
    s = F.reshape(H_ // f, f, W // f, f, 3).astype(np.uint32).sum((1, 3))
    return ((s + f * f // 2) // (f * f)).astype(np.uint8)


def box_rows(F, f, rows=512):
    """`box` in slabs of rows (a multiple of every factor): the same values without an 800 MB temporary at 8192^2."""
    return np.concatenate([box(F[r:r + rows], f) for r in range(0, F.shape[0], rows)])


def frame(s, cam=0.3, light=0.7):
    s.clear(), s.set_light_direction(H.light(light)), s.set_camera(*H.camera(cam)), s.render()


def clean_flags(s):
    """The colour-clean flags of the scene's current frame buffer, [tiles_y, tiles_x] (row 0 = first_tile_row, y up)."""
    import torch
    assert s.sync() == 0
    t = s.band_tiles()
    n = t.tiles_x * t.tiles_y

    class Flags:
        __cuda_array_interface__ = {"shape": (n,), "typestr": "<u4", "data": (int(t.clean_device), False), "version": 2}

    flags = torch.as_tensor(Flags(), device="cuda").cpu().numpy().reshape(t.tiles_y, t.tiles_x) != 0
    return flags, t


def lit_tiles(fb, t):
    """[tiles_y, tiles_x] bool: does the tile hold a non-zero byte of `fb` (the whole-frame image, row 0 = top)?"""
    up = fb[::-1].any(-1)    # row 0 = bottom, as the tiles count
    out = np.zeros((t.tiles_y, t.tiles_x), bool)
    for ty in range(t.tiles_y):
        for tx in range(t.tiles_x):
            y0 = (t.first_tile_row + ty) * 16
            out[ty, tx] = up[y0:y0 + 16, tx * 128:tx * 128 + 128].any()
    return out


# ------------------------------------------------------------------------------------------------------------------
# CPU
# ------------------------------------------------------------------------------------------------------------------

def test_entry_points_declared_exported_and_typed(built):
    import tiny_renderer_amd as T
    from tiny_renderer_amd import _lib
    header = open(os.path.join(REPO, "include", "tiny_renderer.h")).read()
    assert re.search(r"int\s+tr_scene_resolve\(tr_scene \*s, uint32_t factor, void \*out\);", header)
    assert re.search(r"int\s+tr_scene_get_resolved\(tr_scene \*s, uint32_t factor, uint8_t \*rgb\);", header)
    assert "#define TR_ABI_VERSION 3" in header
    raw = C.CDLL(_lib.library_path())
    for name in ("tr_scene_resolve", "tr_scene_get_resolved"):
        assert hasattr(raw, name), name + " is not exported"
        res, args = _lib.SYMBOLS[name]
        assert res is C.c_int and args == [C.c_void_p, C.c_uint32, C.c_void_p]
    L = T.load_library()
    assert L.tr_abi_version() == 3
    # a null scene is refused on the host, with a text
    assert L.tr_scene_resolve(None, 2, None) == _lib.TR_E_INVALID and L.tr_last_error()
    assert L.tr_scene_get_resolved(None, 2, None) == _lib.TR_E_INVALID


@pytest.mark.parametrize("f", FACTORS)
def test_box_is_the_contract(f):
    """Pins the test's own oracle: `box` against the formula as a double loop, random values and blocks whose sum sits
    exactly on the rounding step (f*f*k + f*f/2 rounds up to k + 1; one below stays k)."""
    rng = np.random.default_rng(f)
    Hh, W = 3 * f, 5 * f
    F = rng.integers(0, 256, (Hh, W, 3), dtype=np.uint8)
    k = 100
    # block (0, 0): channel 0 sums to f*f*k + f*f/2, channel 1 to one less, channel 2 is all 255
    F[:f, :f, :] = k
    half = f * f // 2
    flat0 = F[:f, :f, 0].reshape(-1)
    flat0[:half] = k + 1
    F[:f, :f, 0] = flat0.reshape(f, f)
    flat1 = F[:f, :f, 1].reshape(-1)
    flat1[:half - 1] = k + 1
    F[:f, :f, 1] = flat1.reshape(f, f)
    F[:f, :f, 2] = 255
    assert int(F[:f, :f, 0].sum()) == f * f * k + half and int(F[:f, :f, 1].sum()) == f * f * k + half - 1
    want = np.zeros((Hh // f, W // f, 3), np.uint8)
    for Y in range(Hh // f):
        for X in range(W // f):
            for c in range(3):
                total = 0
                for dy in range(f):
                    for dx in range(f):
                        total += int(F[f * Y + dy, f * X + dx, c])
                want[Y, X, c] = (total + f * f // 2) // (f * f)
    got = box(F, f)
    assert np.array_equal(got, want)
    assert tuple(got[0, 0]) == (k + 1, k, 255)
    assert np.array_equal(box_rows(F, f, rows=f), want)


def test_python_methods_reject_what_the_host_can_decide():
    """Scene.resolve / resolve_into / pinned_resolved exist and refuse a bad factor or a frame the factor does not
    divide with ValueError, before anything reaches the library (the scene below has no handle at all)."""
    import tiny_renderer_amd as T
    s = T.Scene.__new__(T.Scene)
    s.width, s.height, s._h, s._pinned = 642, 480, None, []
    for name in ("resolve", "resolve_into", "pinned_resolved"):
        assert callable(getattr(T.Scene, name))
    for f in (0, 1, 3, 16, -2, 2.5):
        with pytest.raises(ValueError):
            s.resolve(f)
        with pytest.raises(ValueError):
            s.resolve_into(f, 4096)
        with pytest.raises(ValueError):
            s.pinned_resolved(f)
    with pytest.raises(ValueError):
        s.resolve(4)             # 642 is not a multiple of 4
    s.width = 640
    with pytest.raises(ValueError):
        s.resolve(2, out=np.zeros((240, 320, 4), np.uint8))
    assert s._resolved_shape(8) == (60, 80, 3)


# ------------------------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------------------------

SHAPES = ((640, 480, True), (1040, 488, True), (1000, 488, False))


@pytest.mark.gpu
@pytest.mark.parametrize("W,Hh,flagged", SHAPES, ids=["640x480", "1040x488", "1000x488"])
@pytest.mark.parametrize("pipe", PIPELINES)
def test_resolve_equals_box_of_the_frame(small_synthetic, pipe, W, Hh, flagged):
    import tiny_renderer_amd as T
    mesh, texs = small_synthetic
    s = T.Scene(W, Hh, mesh, texs, pipe)
    frame(s)
    full = s.get_frame_buffer()
    if flagged:
        flags, _ = clean_flags(s)
        assert flags.any() and not flags.all(), "both kinds of tile must exist (%d of %d clean)" % (flags.sum(), flags.size)
    for f in FACTORS:
        got = s.resolve(f)
        assert got.shape == (Hh // f, W // f, 3) and got.dtype == np.uint8
        assert got.any(), "resolved image is all zeros"
        assert np.array_equal(got, box(full, f)), "factor %d" % f
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("f", FACTORS)
def test_tiles_flagged_clean_resolve_to_zeros_whatever_came_before(small_synthetic, f):
    """A frame that covers the screen, then clear and the small model: tiles lit in the first frame and flagged clean in
    the second must come out as the second frame's zeros."""
    import tiny_renderer_amd as T
    mesh, texs = small_synthetic
    W, Hh = 640, 480
    s = T.Scene(W, Hh, mesh, texs, "phong")
    s.set_instances(np.array([[0.0, 0.0, 0.0, 3.0]], np.float32))
    frame(s, 0.0, 0.0)
    one = s.get_frame_buffer()
    flags_one, t = clean_flags(s)
    lit_one = lit_tiles(one, t)
    assert lit_one.mean() > 0.9, "frame one should cover the screen (%.2f of the tiles lit)" % lit_one.mean()
    s.set_instances(None)
    frame(s)
    two = s.get_frame_buffer()
    flags_two, _ = clean_flags(s)
    assert (lit_one & ~flags_one & flags_two).any(), "no tile lit in frame one is flagged clean in frame two"
    assert not np.array_equal(one, two)
    assert np.array_equal(s.resolve(f), box(two, f))
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("f", FACTORS)
def test_device_and_pinned_targets(small_synthetic, f):
    """resolve_into a torch tensor and a tr_host_alloc buffer, both pre-filled with 0xAA: every byte of a whole-frame
    scene's output is written.  A device pointer off by one byte takes the narrow path and gives the same image."""
    import torch
    import tiny_renderer_amd as T
    mesh, texs = small_synthetic
    W, Hh = 640, 480
    s = T.Scene(W, Hh, mesh, texs, "specular")
    frame(s)
    want = box(s.get_frame_buffer(), f)
    assert (want == 0).all(-1).any() and want.any()
    n = want.size
    dev = torch.full((n + 16,), 0xAA, dtype=torch.uint8, device="cuda")
    pinned = s.pinned_resolved(f)
    pinned[...] = 0xAA
    torch.cuda.synchronize()
    s.resolve_into(f, dev.data_ptr())
    assert s.resolve_into(f, pinned) is pinned
    assert s.sync() == 0
    torch.cuda.synchronize()
    host = dev.cpu().numpy()
    assert np.array_equal(host[:n].reshape(want.shape), want) and (host[n:] == 0xAA).all()
    assert np.array_equal(pinned, want)
    dev.fill_(0xAA)
    torch.cuda.synchronize()
    s.resolve_into(f, dev.data_ptr() + 1)
    assert s.sync() == 0
    torch.cuda.synchronize()
    host = dev.cpu().numpy()
    assert host[0] == 0xAA and (host[n + 1:] == 0xAA).all()
    assert np.array_equal(host[1:n + 1].reshape(want.shape), want)
    s.close()


def _params(n):
    p = np.zeros((n, 12), np.float32)
    for k in range(n):
        p[k, 0:3] = H.light(0.1 * k)
        p[k, 3:6], p[k, 6:9], p[k, 9:12] = H.camera(0.35 * k)
    return p


@pytest.mark.gpu
@pytest.mark.parametrize("buffers", ["own", "callers", "callers_trusted"])
def test_kept_frames_of_a_group_resolve_one_by_one(small_synthetic, buffers):
    import torch
    import tiny_renderer_amd as T
    mesh, texs = small_synthetic
    W, Hh, n = 640, 480, 11
    p = _params(n)
    s = T.Scene(W, Hh, mesh, texs, "phong", frames_per_launch=4, trust_frame_buffers=buffers == "callers_trusted")
    bufs = None
    if buffers != "own":
        bufs = [torch.zeros(Hh * W * 3, dtype=torch.uint8, device="cuda") for _ in range(n)]
        torch.cuda.synchronize()
    for rep in range(2):       # (the second call finds the buffers, and what the scene remembers of them, in use)
        s.render_frames(p, None if bufs is None else [b.data_ptr() for b in bufs])
        kept = s.frames_kept()
        assert kept >= 1
        seen = []
        for back in range(kept):
            s.select_frame(back)
            got = s.resolve(2)
            full = s.get_frame_buffer()
            assert full.any()
            assert np.array_equal(got, box(full, 2)), "call %d, frame %d back" % (rep, back)
            if bufs is not None:
                torch.cuda.synchronize()
                assert np.array_equal(bufs[n - 1 - back].cpu().numpy().reshape(Hh, W, 3), full)
            seen.append(full)
        for a in range(1, kept):
            assert not np.array_equal(seen[0], seen[a]), "kept frames should differ"
    s.close()


@pytest.mark.gpu
def test_resolve_submits_held_back_frames_and_orders_later_renders_behind_it(small_synthetic):
    import torch
    import tiny_renderer_amd as T
    mesh, texs = small_synthetic
    W, Hh, f = 640, 480, 2
    s = T.Scene(W, Hh, mesh, texs, "phong")
    frame(s, 0.3, 0.7)
    first = s.get_frame_buffer()
    frame(s, 1.1, 0.2)
    second = s.get_frame_buffer()
    assert not np.array_equal(first, second)
    a = torch.full((Hh // f * (W // f) * 3,), 0xAA, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    frame(s, 0.3, 0.7)          # may be held back on the host: no getter follows
    s.resolve_into(f, a.data_ptr())
    frame(s, 1.1, 0.2)          # overwrites the frame buffer the resolve reads: must run after it
    assert s.sync() == 0
    torch.cuda.synchronize()
    assert np.array_equal(a.cpu().numpy().reshape(Hh // f, W // f, 3), box(first, f))
    assert np.array_equal(s.resolve(f), box(second, f))
    assert np.array_equal(s.get_frame_buffer(), second)
    # a render without a clear, on top of the frame: what the getters show is what is resolved
    s.set_camera(*H.camera(-0.9)), s.render()
    on_top = s.get_frame_buffer()
    assert not np.array_equal(on_top, second)
    assert np.array_equal(s.resolve(4), box(on_top, 4))
    s.close()


@pytest.mark.gpu
def test_band_scenes_resolve_into_one_buffer(small_synthetic):
    import torch
    import tiny_renderer_amd as T
    from tiny_renderer_amd import _lib
    mesh, texs = small_synthetic
    W, Hh, f = 1024, 512, 4
    whole = T.Scene(W, Hh, mesh, texs, "specular")
    frame(whole)
    want = box(whole.get_frame_buffer(), f)
    whole.close()
    out = torch.full((Hh // f, W // f, 3), 0xAA, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for band in ((0, 128), (256, 512)):
        s = T.Scene(W, Hh, mesh, texs, "specular", band_rows=band)
        frame(s)
        s.resolve_into(f, out.data_ptr())
        assert s.sync() == 0
        # the synchronous getter: the band's rows, zeros elsewhere
        own = s.resolve(f)
        r0, r1 = band[0] // f, band[1] // f
        assert np.array_equal(own[r0:r1], want[r0:r1]) and not own[:r0].any() and not own[r1:].any()
        s.close()
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert want[0:32].any() and want[64:128].any()
    assert np.array_equal(got[0:32], want[0:32]) and np.array_equal(got[64:128], want[64:128])
    assert (got[32:64] == 0xAA).all()
    s = T.Scene(W, Hh, mesh, texs, "specular", band_rows=(0, 130))
    frame(s)
    L = T.load_library()
    assert L.tr_scene_resolve(s._h, f, out.data_ptr()) == _lib.TR_E_INVALID
    assert b"band" in L.tr_last_error()
    host = np.zeros((Hh // f, W // f, 3), np.uint8)
    assert L.tr_scene_get_resolved(s._h, f, host.ctypes.data) == _lib.TR_E_INVALID
    assert s.sync() == 0
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), got), "a refused resolve wrote something"
    assert np.array_equal(s.resolve(2)[:65], box(s.get_frame_buffer(), 2)[:65])    # 130 is a multiple of 2
    s.close()


@pytest.mark.gpu
def test_errors_leave_the_scene_alone(small_synthetic):
    import torch
    import tiny_renderer_amd as T
    from tiny_renderer_amd import _lib
    mesh, texs = small_synthetic
    L = T.load_library()
    s = T.Scene(640, 480, mesh, texs, "phong")
    frame(s)
    dev = torch.full((320 * 240 * 3,), 0xAA, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    host = np.full((240, 320, 3), 0xAA, np.uint8)
    for f in (0, 1, 3, 16):
        assert L.tr_scene_resolve(s._h, f, dev.data_ptr()) == _lib.TR_E_INVALID, f
        assert b"factor" in L.tr_last_error()
        assert L.tr_scene_get_resolved(s._h, f, host.ctypes.data) == _lib.TR_E_INVALID, f
    assert L.tr_scene_resolve(s._h, 2, None) == _lib.TR_E_INVALID
    assert L.tr_scene_get_resolved(s._h, 2, None) == _lib.TR_E_INVALID
    # ordinary host memory: only tr_scene_get_resolved takes it
    assert L.tr_scene_resolve(s._h, 2, host.ctypes.data) == _lib.TR_E_INVALID
    assert b"tr_host_alloc" in L.tr_last_error()
    # a page-locked buffer too small for the resolved frame
    small = L.tr_host_alloc(1000)
    assert small
    assert L.tr_scene_resolve(s._h, 2, small) == _lib.TR_E_INVALID
    L.tr_host_free(small)
    assert s.sync() == 0
    torch.cuda.synchronize()
    assert (dev.cpu().numpy() == 0xAA).all() and (host == 0xAA).all()
    odd = T.Scene(642, 480, mesh, texs, "phong")
    frame(odd)
    assert L.tr_scene_resolve(odd._h, 4, dev.data_ptr()) == _lib.TR_E_INVALID
    assert b"multiples" in L.tr_last_error()
    assert np.array_equal(odd.resolve(2), box(odd.get_frame_buffer(), 2))     # 642 = 2 * 321: the narrow path
    odd.close()
    # the scene goes on as if nothing had been asked
    frame(s, 0.5, 0.1)
    full = s.get_frame_buffer()
    assert np.array_equal(s.resolve(2), box(full, 2))
    s.resolve_into(2, dev.data_ptr())
    assert s.sync() == 0
    torch.cuda.synchronize()
    assert np.array_equal(dev.cpu().numpy().reshape(240, 320, 3), box(full, 2))
    s.close()


@pytest.mark.gpu
def test_full_size_frame_mostly_skipped(built, synthetic):
    """8192 x 8192 phong, camera and light angle 0, resolved by 2 to 4096 x 4096.  More than half of the tiles must be
    flagged clean: a condition on the input -- the kernel is seen skipping most of a real frame -- not a measurement."""
    import tiny_renderer_amd as T
    assets = H.load_assets_py("diablo")
    mesh, texs = assets if assets is not None else synthetic
    W = Hh = 8192
    s = T.Scene(W, Hh, mesh, texs, "phong")
    frame(s, 0.0, 0.0)
    flags, _ = clean_flags(s)
    share = float(flags.mean())
    assert share > 0.5, "only %.3f of the %d tiles are flagged clean" % (share, flags.size)
    got = s.resolve(2)
    full = s.get_frame_buffer()
    assert full.any()
    assert np.array_equal(got, box_rows(full, 2)), "8192^2 -> 4096^2 (%.3f of the tiles flagged clean)" % share
    s.close()


@pytest.mark.gpu
def test_cli_ssaa_writes_the_resolved_picture(synthetic, tmp_path):
    import tiny_renderer_amd as T
    from tiny_renderer_amd import cli
    mesh, texs = synthetic
    out = str(tmp_path / "ssaa.ppm")
    assert cli.main(["--synthetic", "-s", "phong", "--width", "160", "--height", "120", "--ssaa", "4",
                     "--camera-angle", "0.3", "--light-angle", "0.7", "--out", out]) == 0
    raw = open(out, "rb").read()
    head = b"P6\n160 120\n255\n"
    assert raw.startswith(head)
    got = np.frombuffer(raw[len(head):], np.uint8).reshape(120, 160, 3)
    s = T.Scene(640, 480, mesh, texs, "phong")
    frame(s)
    assert got.any() and np.array_equal(got, box(s.get_frame_buffer(), 4))
    s.close()
