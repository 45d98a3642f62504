"""Frame accumulation: tr_scene_accumulate / tr_scene_get_accumulated average the last n kept frames of a
render_frames call on the device (k_accumulate), tr_accumulate_host is the same rule on the host.  Every comparison is
byte for byte against the numpy restatement below, applied to the frames the scene itself returns through
select_frame(k) + get_frame_buffer."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import helpers as H

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_FRAMES, MAX_D = 32, 32 * 255
MAX_NUM = 255 * MAX_D + MAX_D // 2
F32_MIN_BITS = np.uint32(0xFF7FFFFF)
# (W, H): one tile; 2 x 2 whole tiles; partial tiles in x and y, still 16-byte shares; the narrow form; 3 x 3 tiles
SHAPES = [(128, 16), (256, 32), (208, 40), (200, 40), (384, 48)]


def oracle(frames, weights=None):
    """(sum of w_k * F_k + D // 2) // D on the stored bytes, D = sum of w_k."""
    w = [1] * len(frames) if weights is None else [int(v) for v in weights]
    D = sum(w)
    assert len(w) == len(frames) and D >= 1
    num = np.zeros(np.asarray(frames[0]).shape, np.uint32)
    for wk, f in zip(w, frames):
        num += np.uint32(wk) * np.asarray(f).astype(np.uint32)
    return ((num + np.uint32(D // 2)) // np.uint32(D)).astype(np.uint8)


def box(F, f):
    H_, W, _ = F.shape
    s = F.reshape(H_ // f, f, W // f, f, 3).astype(np.uint32).sum((1, 3))
    return ((s + f * f // 2) // (f * f)).astype(np.uint8)


def views(n, first=0.75, rest=1.35):
    """n frames in render order: the camera turns by 0.35 rad a frame, the light stays within 0.4 rad of it, and the
    view point is moved along the camera's right vector, which puts the model to the left of the picture: by `first` in
    the oldest frame, by rest + 0.03 k in frame k >= 1.  The frames so cover different tiles -- the oldest the most --
    and every frame shows lit pixels.  Chosen with the CPU oracle so that no tile depends on a few pixels (the
    fast-clear flags go by the polygons' boxes, not by covered pixels): at 384 x 48 the oldest frame draws the two left
    tile columns and stays 10 pixels clear of the third, every later frame draws the left column alone and stays 10
    pixels clear of the second.  At 200 x 40 the same holds for first = 0.375, rest = 0.85 (two columns, then one)."""
    p = np.zeros((n, 12), np.float32)
    for k in range(n):
        a = 0.35 * k
        off = (first if k == 0 else rest + 0.03 * k) * np.array([np.cos(a), 0.0, -np.sin(a)], np.float32)
        frm, _, up = H.camera(a)
        p[k, 0:3] = H.light(a + 0.4 - 0.1 * k)
        p[k, 3:6], p[k, 6:9], p[k, 9:12] = np.array(frm, np.float32) + off, off, up
    return p


def kept(s, n):
    """F_k, k = 0 .. n - 1: what get_frame_buffer returns after select_frame(k); the selection goes back to frame 0."""
    out = []
    for k in range(n):
        s.select_frame(k)
        out.append(s.get_frame_buffer())
    s.select_frame(0)
    return out


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


def kept_flags(s, n):
    out = []
    for k in range(n):
        s.select_frame(k)
        out.append(clean_flags(s)[0])
    s.select_frame(0)
    return np.array(out)


def tile_rows(t, ty, tx, Hh):
    """Image rows and columns (row 0 = top) of tile (ty, tx) of band-tile record t."""
    y0 = (t.first_tile_row + ty) * 16
    return slice(max(Hh - y0 - 16, 0), Hh - y0), slice(tx * 128, tx * 128 + 128)


def group(T, W, Hh, mesh, texs, pipe, n, at=(), **kw):
    """A scene that has rendered views(n, *at) by one call and keeps all n frames."""
    kw.setdefault("frames_per_launch", max(n, 1))
    s = T.Scene(W, Hh, mesh, texs, pipe, **kw)
    s.render_frames(views(n, *at))
    assert s.frames_kept() == n
    return s


# ------------------------------------------------------------------------------------------------------------------
# CPU
# ------------------------------------------------------------------------------------------------------------------

def test_entry_points_declared_exported_and_typed(built):
    import tiny_renderer_amd as T
    from tiny_renderer_amd import _lib
    header = open(os.path.join(REPO, "include", "tiny_renderer.h")).read()
    assert "#define TR_ACCUMULATE_MAX_FRAMES 32" in header
    assert re.search(r"int\s+tr_scene_accumulate\(tr_scene \*s, uint32_t n_frames, const uint32_t \*weights( /\*.*?\*/)?, void \*out( /\*.*?\*/)?\);", header)
    assert re.search(r"int\s+tr_scene_get_accumulated\(tr_scene \*s, uint32_t n_frames, const uint32_t \*weights, uint8_t \*rgb\);", header)
    assert re.search(r"int\s+tr_accumulate_host\(size_t n_bytes, uint32_t n_frames, const uint8_t \*const \*frames, "
                     r"const uint32_t \*weights, uint8_t \*out\);", header)
    exports = open(os.path.join(REPO, "tiny_renderer_amd", "csrc", "exports.map")).read()
    assert re.search(r"global:\s*tr_\*;", exports)       # every tr_ symbol is listed by the pattern
    raw = C.CDLL(_lib.library_path())
    for name in ("tr_scene_accumulate", "tr_scene_get_accumulated", "tr_accumulate_host"):
        assert hasattr(raw, name), name + " is not exported"
        assert name in _lib.SYMBOLS
    assert _lib.SYMBOLS["tr_scene_accumulate"] == (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p])
    assert _lib.SYMBOLS["tr_scene_get_accumulated"] == (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p])
    assert _lib.SYMBOLS["tr_accumulate_host"] == (C.c_int, [C.c_size_t, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p])
    L = T.load_library()
    assert L.tr_abi_version() == 3
    buf = np.zeros(12, np.uint8)
    assert L.tr_scene_accumulate(None, 1, None, None) == _lib.TR_E_INVALID and b"null scene" in L.tr_last_error()
    assert L.tr_scene_get_accumulated(None, 1, None, buf.ctypes.data) == _lib.TR_E_INVALID and b"null scene" in L.tr_last_error()
    for name in ("accumulate", "accumulate_into", "accumulate_in_place"):
        assert callable(getattr(T.Scene, name))
    assert callable(T.accumulate_host)


def test_the_numpy_oracle_is_the_formula():
    """The restatement above against the issue's formula as a plain loop over bytes, with sums exactly on the rounding
    step (2 * sum + D an exact multiple of 2 * D upward) and one below it."""
    rng = np.random.default_rng(5)
    cases = [([np.array([3], np.uint8), np.array([4], np.uint8)], None),             # 7 + 1 = 8: 3.5 rounds up to 4
             ([np.array([3], np.uint8), np.array([3], np.uint8)], None),             # 3
             ([np.array([0], np.uint8), np.array([1], np.uint8), np.array([0], np.uint8)], None),   # 1/3 -> 0
             ([np.array([1], np.uint8), np.array([1], np.uint8), np.array([0], np.uint8)], None),   # 2/3 -> 1
             ([np.array([10], np.uint8), np.array([11], np.uint8)], [3, 1]),         # 41 / 4 = 10.25 -> 10
             ([np.array([10], np.uint8), np.array([12], np.uint8)], [1, 1]),         # 11 exactly
             ([np.array([10], np.uint8), np.array([11], np.uint8)], [1, 3]),         # 43 / 4 = 10.75 -> 11
             ([np.array([10], np.uint8), np.array([11], np.uint8)], [2, 2]),         # 10.5 -> 11: on the step
             ([np.array([255], np.uint8)] * 32, [255] * 32)]
    want = [4, 3, 0, 1, 10, 11, 11, 11, 255]
    for (fr, w), v in zip(cases, want):
        assert oracle(fr, w)[0] == v, (fr, w)
    for n in (1, 2, 5, 32):
        fr = [rng.integers(0, 256, 97, dtype=np.uint8) for _ in range(n)]
        w = [int(v) for v in rng.integers(0, 256, n)]
        w[0] = max(w[0], 1)
        D = sum(w)
        loop = [(sum(w[k] * int(fr[k][b]) for k in range(n)) + D // 2) // D for b in range(97)]
        assert oracle(fr, w).tolist() == loop
    # D = 4: numerators 4q + 2 (on the step) and 4q + 1 (one below) for every q the bytes allow
    for q in (0, 1, 100, 254):
        on = [np.array([q + 1], np.uint8), np.array([q], np.uint8)]
        assert oracle(on, [2, 2])[0] == q + 1 and oracle(on, [1, 3])[0] == q


def test_division_by_multiplier_is_exact_and_the_host_program_runs(built, tmp_path):
    """scripts/accumulate_host_check.cpp, built for the host without a sanitizer: for every D in 1..8160 accumulate_div
    equals `/` at every multiple of D and one below it up to the largest numerator and at that numerator itself, and
    the host rule equals the formula on arrays of exactly the frames' size.  (The same program is what runs under
    -fsanitize=address,undefined by hand: its header has the line.)"""
    exe = str(tmp_path / "accumulate_host_check")
    subprocess.check_call([os.environ.get("CXX", "c++"), "-std=c++17", "-O1", "-I" + os.path.join(REPO, "include"),
                           "-I" + os.path.join(REPO, "tiny_renderer_amd", "csrc"),
                           os.path.join(REPO, "scripts", "accumulate_host_check.cpp"), "-o", exe])
    done = subprocess.run([exe], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout + done.stderr
    m = re.search(r"division: (\d+) points, 0 mismatches", done.stdout)
    assert m and int(m.group(1)) >= 2 * 255 * MAX_D, done.stdout
    assert done.stdout.strip().endswith("\n0 mismatches") or done.stdout.strip().endswith("0 mismatches")
    # the same through the library, where the numerator can be steered: one frame of weight 1 beside others of one value
    import tiny_renderer_amd as T
    for D in (1, 2, 3, 255, 256, 257, 4095, 4096, 4097, 7906):
        w = [1] + [255] * ((D - 1) // 255) + ([(D - 1) % 255] if (D - 1) % 255 else [])
        assert sum(w) == D and len(w) <= MAX_FRAMES
        first = np.arange(256, dtype=np.uint8)
        for v in (0, 1, 127, 254, 255):
            fr = [first] + [np.full(256, v, np.uint8)] * (len(w) - 1)
            assert np.array_equal(T.accumulate_host(fr, w), oracle(fr, w)), (D, v)


@pytest.mark.parametrize("n", [1, 2, 3, 7, 8, 32])
def test_host_rule_equals_the_oracle(built, n):
    import tiny_renderer_amd as T
    rng = np.random.default_rng(100 + n)
    n_bytes = 3 * 37 * 29 + 1              # not a multiple of 4
    fills = {"random": [rng.integers(0, 256, n_bytes, dtype=np.uint8) for _ in range(n)],
             "white": [np.full(n_bytes, 255, np.uint8)] * n,
             "black": [np.zeros(n_bytes, np.uint8)] * n}
    mixed = rng.integers(0, 256, n)
    mixed[rng.integers(0, n)] = 255
    if n > 1:
        mixed[(int(np.argmax(mixed)) + 1) % n] = 0
    for name, fr in fills.items():
        for w in (None, [1] * n, [7] * n, [255] * n, mixed.tolist(), list(range(1, n + 1))):
            got = T.accumulate_host(fr, w)
            assert got.dtype == np.uint8 and np.array_equal(got, oracle(fr, w)), (name, w)
        for hot in range(n):                # one-hot: that frame byte for byte
            w = [0] * n
            w[hot] = 1 + (37 * hot) % 255
            assert np.array_equal(T.accumulate_host(fr, w), fr[hot]), (name, hot)
        assert np.array_equal(T.accumulate_host([fr[0]] * n), fr[0])
    shaped = [f.reshape(-1)[:3 * 37 * 29].reshape(29, 37, 3) for f in fills["random"]]
    assert T.accumulate_host(shaped).shape == (29, 37, 3)


def test_refusals_of_the_host_function_and_the_wrappers(built):
    import tiny_renderer_amd as T
    from tiny_renderer_amd import _lib
    L = T.load_library()
    a = np.full(8, 9, np.uint8)
    out = np.full(8, 0xAB, np.uint8)

    def host(n, frames, weights, n_bytes=8, o=out):
        ptrs = (C.c_void_p * max(len(frames), 1))(*[f.ctypes.data if f is not None else None for f in frames])
        w = np.asarray(weights, np.uint32) if weights is not None else None
        return L.tr_accumulate_host(n_bytes, n, ptrs, w.ctypes.data if w is not None else None, o.ctypes.data if o is not None else None)

    assert host(1, [a], None) == 0 and (out == 9).all()
    out[:] = 0xAB
    for n, frames, weights, text in ((0, [a], None, b"n_frames"), (33, [a] * 33, None, b"n_frames"),
                                     (2, [a, a], [1, 256], b"255"), (2, [a, a], [0, 0], b"zero"),
                                     (2, [a, None], None, b"null")):
        assert host(n, frames, weights) == _lib.TR_E_INVALID, (n, weights)
        assert text in L.tr_last_error(), L.tr_last_error()
    assert host(1, [a], None, o=None) == _lib.TR_E_INVALID
    assert L.tr_accumulate_host(8, 1, None, None, out.ctypes.data) == _lib.TR_E_INVALID
    assert (out == 0xAB).all()
    assert L.tr_accumulate_host(0, 1, None, None, None) == 0          # nothing to do
    assert L.tr_accumulate_host(0, 0, None, None, None) == _lib.TR_E_INVALID
    for frames, weights in (([], None), ([a] * 33, None), ([a, a], [1, 256]), ([a, a], [0, 0]), ([a, a], [1, -1]),
                            ([a, a], [1.0, 2.0]), ([a, a], [1]), ([a, a[:4]], None)):
        with pytest.raises(ValueError):
            T.accumulate_host(frames, weights)
    from tiny_renderer_amd.scene import accumulate_weights
    for n, w in ((0, None), (33, None), (2.0, None), (True, None), (2, [1, 256]), (2, [0, 0]), (2, [1, 2, 3]), (2, [[1, 2]])):
        with pytest.raises(ValueError):
            accumulate_weights(n, w)
    n, w = accumulate_weights(3, [0, 255, 7])
    assert n == 3 and w.dtype == np.uint32 and w.tolist() == [0, 255, 7]
    assert accumulate_weights(32) == (32, None)


def test_cli_refuses_shutter_with_what_it_does_not_compose_with(capsys):
    from tiny_renderer_amd import cli
    base = ["--synthetic", "--frames", "8", "--shutter", "4"]
    for extra in (["--gpus", "2"], ["--ao", "4"], ["--with", "somewhere"], ["--frames", "3"], ["--shutter", "33"], ["--shutter", "-1"]):
        with pytest.raises(SystemExit):
            cli.main(base + extra)
    capsys.readouterr()


# ------------------------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------------------------

CASES = [(1, None), (2, [1, 3]), (3, [2, 0, 5]), (8, None), (8, [0, 1, 2, 3, 4, 5, 6, 255])]


@pytest.mark.gpu
@pytest.mark.parametrize("pipe,W,Hh", [("phong", w, h) for w, h in SHAPES] + [("shadow", 384, 48), ("shadow", 200, 40)])
def test_out_of_place_equals_the_oracle(small_synthetic, pipe, W, Hh):
    """Device memory and tr_host_alloc memory prefilled with 0xAB (a tile skipped instead of zeroed shows), and
    get_accumulated into ordinary host memory, against the oracle over the frames read afterwards."""
    import torch
    import tiny_renderer_amd as T
    mesh, texs = small_synthetic
    nb = W * Hh * 3
    for n, w in CASES:
        s = group(T, W, Hh, mesh, texs, pipe, n)
        dev = torch.full((nb + 32,), 0xAB, dtype=torch.uint8, device="cuda")
        pinned = s.pinned_frame()
        pinned[...] = 0xAB
        torch.cuda.synchronize()
        s.accumulate_into(n, dev.data_ptr() + 16, w)
        assert s.accumulate_into(n, pinned, w) is pinned
        assert s.sync() == 0
        torch.cuda.synchronize()
        host = s.accumulate(n, w)
        frames = kept(s, n)
        want = oracle(frames, w)
        assert want.any() and (n == 1 or not np.array_equal(frames[0], frames[1]))
        raw = dev.cpu().numpy()
        assert (raw[:16] == 0xAB).all() and (raw[16 + nb:] == 0xAB).all()
        assert np.array_equal(raw[16:16 + nb].reshape(Hh, W, 3), want), (n, w)
        assert np.array_equal(pinned, want), (n, w)
        assert np.array_equal(host, want), (n, w)
        s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [2, 3, 4, 8])
def test_coverage_preconditions_and_untouched_inputs(small_synthetic, n):
    """At 384 x 48 the frames of views(n) leave a tile clean in every frame, one clean in some and drawn in others, and
    one drawn in all; and accumulating out of place changes no kept frame, no z and no flag."""
    import torch
    import tiny_renderer_amd as T
    mesh, texs = small_synthetic
    W, Hh = 384, 48
    s = group(T, W, Hh, mesh, texs, "phong", n, store_depth=True)
    flags = kept_flags(s, n)
    up = flags.sum(0)
    assert flags.shape == (n, 3, 3)
    assert (up == n).any(), "no tile is clean in every frame"
    assert ((up > 0) & (up < n)).any(), "no tile is clean in some frames and drawn in others"
    assert (up == 0).any(), "no tile is drawn in every frame"
    frames = kept(s, n)
    zs = []
    for k in range(n):
        s.select_frame(k)
        zs.append(s.read_z_f32())
    s.select_frame(0)
    for k in range(n):      # a flagged tile holds zeros
        for ty, tx in zip(*np.nonzero(flags[k])):
            rows, cols = tile_rows(clean_flags(s)[1], ty, tx, Hh)
            assert not frames[k][rows, cols].any()
    dev = torch.full((W * Hh * 3,), 0xAB, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    w = list(range(1, n + 1))
    s.accumulate_into(n, dev.data_ptr(), w)
    got = s.accumulate(n, w)
    assert s.sync() == 0
    torch.cuda.synchronize()
    assert np.array_equal(got, oracle(frames, w))
    assert np.array_equal(dev.cpu().numpy().reshape(Hh, W, 3), got)
    assert np.array_equal(kept_flags(s, n), flags)
    for k, f in enumerate(kept(s, n)):
        assert np.array_equal(f, frames[k])
    for k in range(n):
        s.select_frame(k)
        assert np.array_equal(s.read_z_f32().view(np.uint32), zs[k].view(np.uint32))
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("W,Hh", [(384, 48), (200, 40)])
def test_in_place_is_what_every_consumer_sees(small_synthetic, W, Hh):
    """In place into the newest frame, which leaves tiles clean that older frames draw: the getters, resolve, the sparse
    read-back and composite (as src) deliver the average, so the destination's flag came down with the stores."""
    import tiny_renderer_amd as T
    mesh, texs = small_synthetic
    n, w = 8, [3, 1, 2, 1, 1, 2, 1, 3]
    at = (0.375, 0.85) if W == 200 else ()
    s = group(T, W, Hh, mesh, texs, "phong", n, at, store_depth=True)
    twin = group(T, W, Hh, mesh, texs, "phong", n, at, store_depth=True)
    frames = kept(twin, n)
    flags = kept_flags(twin, n)
    z_newest = twin.read_z_f32()
    want = oracle(frames, w)
    raised = flags[0] & ~flags[1:].all(0)     # clean in the destination, drawn in another contributing frame
    assert raised.any(), "the destination leaves no tile clean that another frame draws"
    pinned = s.pinned_frame()
    s.get_frame_buffer_async(pinned)          # the host buffer now holds the newest frame, its record the frame's flags
    assert s.sync() == 0 and np.array_equal(pinned, frames[0])
    s.accumulate_in_place(n, w)
    now, t = clean_flags(s)
    for ty, tx in zip(*np.nonzero(raised)):
        rows, cols = tile_rows(t, ty, tx, Hh)
        assert want[rows, cols].any() and not frames[0][rows, cols].any()
        assert not now[ty, tx], "the averaged tile (%d, %d) is still flagged clean" % (ty, tx)
    assert np.array_equal(now, flags.all(0)), "a tile is clean exactly where every contributing frame is"
    assert np.array_equal(s.get_frame_buffer(), want)
    if W % 2 == 0 and Hh % 2 == 0:
        assert np.array_equal(s.resolve(2), box(want, 2))
    s.get_frame_buffer_async(pinned)
    assert s.sync() == 0
    assert np.array_equal(pinned, want)
    other = T.Scene(W, Hh, mesh, texs, "phong", store_depth=True)
    other.clear()
    other.composite(s)
    drawn = (z_newest.view(np.uint32) != F32_MIN_BITS)[::-1]
    assert drawn.any() and np.array_equal(other.get_frame_buffer(), np.where(drawn[..., None], want, 0).astype(np.uint8))
    # z is the selected frame's, and the other kept frames are as they were
    assert np.array_equal(s.read_z_f32().view(np.uint32), z_newest.view(np.uint32))
    after = kept(s, n)
    assert np.array_equal(after[0], want)
    for k in range(1, n):
        assert np.array_equal(after[k], frames[k])
    for x in (s, twin, other):
        x.close()


@pytest.mark.gpu
def test_in_place_destinations(small_synthetic):
    """select_frame(1) as destination; a destination of weight 0 that alone draws a tile (the tile becomes zeros); a
    destination outside the last n is refused; twice averages twice."""
    import tiny_renderer_amd as T
    from tiny_renderer_amd import _lib
    mesh, texs = small_synthetic
    W, Hh, n = 384, 48, 3
    L = T.load_library()
    twin = group(T, W, Hh, mesh, texs, "phong", n)
    frames = kept(twin, n)
    flags = kept_flags(twin, n)
    twin.close()
    # frame 1 as destination
    s = group(T, W, Hh, mesh, texs, "phong", n)
    s.select_frame(1)
    s.accumulate_in_place(n, [1, 2, 4])
    want = oracle(frames, [1, 2, 4])
    assert np.array_equal(s.get_frame_buffer(), want) and np.array_equal(s.resolve(2), box(want, 2))
    after = kept(s, n)
    assert np.array_equal(after[0], frames[0]) and np.array_equal(after[1], want) and np.array_equal(after[2], frames[2])
    # twice: the second call averages the first call's result
    s.select_frame(1)
    s.accumulate_in_place(n, [1, 2, 4])
    assert np.array_equal(s.get_frame_buffer(), oracle([frames[0], want, frames[2]], [1, 2, 4]))
    s.close()
    # the oldest frame draws tiles the others leave clean; with weight 0 it contributes nothing
    only_oldest = ~flags[2] & flags[0] & flags[1]
    assert only_oldest.any(), "no tile is drawn by the oldest frame alone"
    s = group(T, W, Hh, mesh, texs, "phong", n)
    s.select_frame(2)
    s.accumulate_in_place(n, [1, 1, 0])
    want = oracle(frames, [1, 1, 0])
    got = s.get_frame_buffer()
    rows, cols = tile_rows(clean_flags(s)[1], *[int(v[0]) for v in np.nonzero(only_oldest)], Hh)
    assert frames[2][rows, cols].any() and not got[rows, cols].any()
    assert np.array_equal(got, want) and np.array_equal(s.resolve(2), box(want, 2))
    # the destination must be among the n
    assert L.tr_scene_accumulate(s._h, 2, None, None) == _lib.TR_E_INVALID and b"current frame" in L.tr_last_error()
    assert s.sync() == 0 and np.array_equal(s.get_frame_buffer(), want)
    s.select_frame(1)
    s.accumulate_in_place(2)
    assert np.array_equal(s.get_frame_buffer(), oracle(frames[:2]))
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["morph", "skin"])
def test_frames_with_a_pose_each(small_synthetic, kind):
    """render_frames with a pose (a palette) per frame, n = 4: the average equals the oracle over the frames of scenes
    of the host-deformed meshes."""
    import tiny_renderer_amd as T
    from tests import test_morph as TM
    from tests import test_skin as TS
    mesh, texs = small_synthetic
    W, Hh, n = 384, 48, 4
    p = views(n)
    s = T.Scene(W, Hh, mesh, texs, "phong", frames_per_launch=n)
    if kind == "morph":
        poses = TM._poses(n)
        s.set_morph_targets(*TM._targets(mesh))
        s.render_frames(p, morph_weights=poses)
        twins = [TM._posed(mesh, poses[i]) for i in range(n)]
    else:
        pals = TS._palettes(n)
        s.set_skin(*TS._rig(mesh), n_bones=TS.N_BONES)
        s.render_frames(p, bone_palettes=pals)
        twins = [TS._skinned(mesh, pals[i]) for i in range(n)]
    frames = []
    for i in reversed(range(n)):            # F_0 is the newest
        t = T.Scene(W, Hh, twins[i], texs, "phong")
        t.clear(), t.set_light_direction(p[i, 0:3]), t.set_camera(p[i, 3:6], p[i, 6:9], p[i, 9:12])
        t.render()
        frames.append(t.get_frame_buffer())
        t.close()
    assert not np.array_equal(frames[0], frames[1])
    w = [4, 3, 2, 1]
    want = oracle(frames, w)
    assert want.any() and np.array_equal(s.accumulate(n, w), want)
    s.accumulate_in_place(n, w)
    assert np.array_equal(s.get_frame_buffer(), want)
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("trusted", [False, True])
def test_callers_frame_buffers(small_synthetic, trusted):
    """Frames in the caller's device buffers, one of them at a 4-byte offset (the narrow form), out of place and in
    place; a buffer of the caller's as `out` is refused."""
    import torch
    import tiny_renderer_amd as T
    from tiny_renderer_amd import _lib
    mesh, texs = small_synthetic
    W, Hh, n = 384, 48, 4
    nb = W * Hh * 3
    for shift in (0, 4):
        s = T.Scene(W, Hh, mesh, texs, "phong", frames_per_launch=n, trust_frame_buffers=trusted)
        store = torch.zeros(n * (nb + 64), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ptrs = [store.data_ptr() + k * (nb + 64) + (shift if k == 1 else 0) for k in range(n)]
        for rep in range(2):    # (the second call finds the buffers, and what the scene remembers of them, in use)
            s.render_frames(views(n), ptrs)
            w = [1, 2, 3, 4]
            got = s.accumulate(n, w)
            frames = kept(s, n)
            assert np.array_equal(got, oracle(frames, w)), (shift, rep)
        L = T.load_library()
        assert L.tr_scene_accumulate(s._h, n, None, ptrs[2]) == _lib.TR_E_INVALID and b"overlaps" in L.tr_last_error()
        assert L.tr_scene_accumulate(s._h, n, None, ptrs[0] + nb - 1) == _lib.TR_E_INVALID
        s.accumulate_in_place(n, w)
        want = oracle(frames, w)
        assert np.array_equal(s.get_frame_buffer(), want)
        torch.cuda.synchronize()
        off = (n - 1) * (nb + 64)
        assert np.array_equal(store[off:off + nb].cpu().numpy().reshape(Hh, W, 3), want)
        s.close()


@pytest.mark.gpu
def test_band_scene_writes_its_rows_only(small_synthetic):
    import torch
    import tiny_renderer_amd as T
    mesh, texs = small_synthetic
    W, Hh, n = 256, 48, 3
    s = group(T, W, Hh, mesh, texs, "phong", n, band_rows=(16, 32))
    out = torch.full((Hh, W, 3), 0xAB, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    w = [5, 1, 2]
    s.accumulate_into(n, out.data_ptr(), w)
    assert s.sync() == 0
    torch.cuda.synchronize()
    own = s.accumulate(n, w)
    want = oracle([f[16:32] for f in kept(s, n)], w)
    got = out.cpu().numpy()
    assert want.any()
    assert np.array_equal(got[16:32], want) and (got[:16] == 0xAB).all() and (got[32:] == 0xAB).all()
    assert np.array_equal(own[16:32], want) and not own[:16].any() and not own[32:].any()
    s.accumulate_in_place(n, w)
    assert np.array_equal(s.get_frame_buffer()[16:32], want)
    s.close()


@pytest.mark.gpu
def test_winner_tap_scene_keeps_one_frame(small_synthetic):
    import tiny_renderer_amd as T
    from tiny_renderer_amd import _lib
    mesh, texs = small_synthetic
    W, Hh = 384, 48
    s = T.Scene(W, Hh, mesh, texs, "phong", winner_tap=True)
    s.render_frames(views(3))
    assert s.frames_kept() == 1
    frame = s.get_frame_buffer()
    win = s.read_winner_u32()
    assert frame.any() and np.array_equal(s.accumulate(1, [9]), frame)
    s.accumulate_in_place(1)
    assert np.array_equal(s.get_frame_buffer(), frame) and np.array_equal(s.read_winner_u32(), win)
    L = T.load_library()
    assert L.tr_scene_accumulate(s._h, 2, None, None) == _lib.TR_E_INVALID
    s.close()


@pytest.mark.gpu
def test_refusals_change_and_queue_nothing(small_synthetic):
    import torch
    import tiny_renderer_amd as T
    from tiny_renderer_amd import _lib
    mesh, texs = small_synthetic
    W, Hh, n = 256, 32, 3
    nb = W * Hh * 3
    L = T.load_library()
    s = group(T, W, Hh, mesh, texs, "phong", n)
    s.profile_enable(True)
    frames = kept(s, n)
    dev = torch.full((nb,), 0xAB, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    host = np.full((Hh, W, 3), 0xAB, np.uint8)
    u32 = lambda v: np.asarray(v, np.uint32)
    bad = [(0, None, b"n_frames"), (33, None, b"n_frames"), (4, None, b"frames_kept"), (3, u32([1, 256, 1]), b"255"),
           (3, u32([0, 0, 0]), b"zero")]
    for k, w, text in bad:
        wp = w.ctypes.data if w is not None else None
        for target in (dev.data_ptr(), None):
            assert L.tr_scene_accumulate(s._h, k, wp, target) == _lib.TR_E_INVALID, (k, w)
            assert text in L.tr_last_error(), L.tr_last_error()
        assert L.tr_scene_get_accumulated(s._h, k, wp, host.ctypes.data) == _lib.TR_E_INVALID, (k, w)
    assert L.tr_scene_get_accumulated(s._h, 3, None, None) == _lib.TR_E_INVALID
    # ordinary host memory: only tr_scene_get_accumulated takes it; a pinned buffer that is too small; a frame of the scene
    assert L.tr_scene_accumulate(s._h, 3, None, host.ctypes.data) == _lib.TR_E_INVALID and b"tr_host_alloc" in L.tr_last_error()
    small = L.tr_host_alloc(1000)
    assert small and L.tr_scene_accumulate(s._h, 3, None, small) == _lib.TR_E_INVALID and b"smaller" in L.tr_last_error()
    L.tr_host_free(small)
    s.select_frame(1)
    own = s.frame_buffer_device()
    s.select_frame(0)
    assert L.tr_scene_accumulate(s._h, 3, None, own) == _lib.TR_E_INVALID and b"overlaps" in L.tr_last_error()
    assert L.tr_scene_accumulate(s._h, 3, None, s.frame_buffer_device() + 3) == _lib.TR_E_INVALID
    with pytest.raises(ValueError):
        s.accumulate(0)
    with pytest.raises(ValueError):
        s.accumulate_into(3, None)
    with pytest.raises(ValueError):
        s.accumulate_into(3, np.zeros((Hh, W), np.uint8))
    with pytest.raises(ValueError):
        s.accumulate_in_place(3, [1, 2])
    assert s.sync() == 0
    torch.cuda.synchronize()
    assert (dev.cpu().numpy() == 0xAB).all() and (host == 0xAB).all()
    assert "k_accumulate" not in s.profile_read()
    for k, f in enumerate(kept(s, n)):
        assert np.array_equal(f, frames[k])
    # after a plain render nothing is kept
    s.clear(), s.set_light_direction(H.light(0.7)), s.set_camera(*H.camera(0.3)), s.render()
    assert s.frames_kept() == 0
    assert L.tr_scene_accumulate(s._h, 1, None, None) == _lib.TR_E_INVALID and b"frames_kept" in L.tr_last_error()
    with pytest.raises(T.TinyRendererError):
        s.accumulate(1)
    # the scene goes on as if nothing had been asked
    s.render_frames(views(n))
    assert np.array_equal(s.accumulate(n), oracle(kept(s, n)))
    s.close()


@pytest.mark.gpu
def test_profile_lists_one_launch(small_synthetic):
    import torch
    import tiny_renderer_amd as T
    mesh, texs = small_synthetic
    W, Hh, n = 256, 32, 2
    s = group(T, W, Hh, mesh, texs, "phong", n)
    assert s.sync() == 0
    dev = torch.zeros(W * Hh * 3, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    s.profile_enable(True)
    s.accumulate_into(n, dev.data_ptr())
    assert s.sync() == 0
    prof = s.profile_read()
    assert prof["k_accumulate"]["launches"] == 1 and prof["k_accumulate"]["total_ms"] > 0.0
    s.close()


@pytest.mark.gpu
def test_a_larger_frame(small_synthetic):
    import tiny_renderer_amd as T
    mesh, texs = small_synthetic
    W = Hh = 1024
    n, w = 8, [1, 2, 3, 4, 4, 3, 2, 1]
    s = group(T, W, Hh, mesh, texs, "phong", n)
    got = s.accumulate(n, w)
    frames = kept(s, n)
    want = oracle(frames, w)
    assert want.any() and (want == 0).all(-1).any()
    assert np.array_equal(got, want)
    s.accumulate_in_place(n, w)
    assert np.array_equal(s.get_frame_buffer(), want) and np.array_equal(s.resolve(4), box(want, 4))
    s.close()


@pytest.mark.gpu
def test_cli_shutter_under_supersampling(synthetic, tmp_path):
    import tiny_renderer_amd as T
    from tiny_renderer_amd import cli
    mesh, texs = synthetic
    out = str(tmp_path / "blur.ppm")
    assert cli.main(["--synthetic", "-s", "phong", "--width", "160", "--height", "120", "--ssaa", "2", "--frames", "8",
                     "--shutter", "4", "--camera-angle", "0.3", "--light-angle", "0.7", "--out", out]) == 0
    raw = open(out, "rb").read()
    head = b"P6\n160 120\n255\n"
    assert raw.startswith(head)
    got = np.frombuffer(raw[len(head):], np.uint8).reshape(120, 160, 3)
    p = np.zeros((8, 12), np.float32)
    for f in range(8):
        ca = np.float32(0.3 + 2.0 * np.pi * f / 8)
        p[f, 0:3] = H.light(0.7)
        p[f, 3:6], p[f, 6:9], p[f, 9:12] = [float(np.sin(ca)), 0.0, float(np.cos(ca))], [0, 0, 0], [0, 1, 0]
    s = T.Scene(320, 240, mesh, texs, "phong", frames_per_launch=4)
    s.render_frames(p)
    frames = kept(s, 4)
    assert not np.array_equal(frames[0], frames[3])
    assert got.any() and np.array_equal(got, box(oracle(frames), 2))
    s.close()
