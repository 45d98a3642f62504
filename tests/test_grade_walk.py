"""k_grade's persistent walk beyond a workgroup's first tile (tr_scene_debug_grade_grid).

k_grade's workgroups are persistent: the launcher starts G = min(CUs x per_cu, tiles) of them and workgroup b takes the
slots b, b + G, b + 2 G, ...  On an MI355X G is 512 to 2048, and the frames of tests/test_grade.py have at most 12 tiles:
there every workgroup runs the loop's body once.  Here the diagnostic caps G, so that frames of 25 to 36 tiles take up
to 36 rounds, and one frame is large enough for the launcher's own G to go round.

The rules of tests/test_grade.py hold: the expectation is tr_grade_host of a snapshot of the very frame that is then
rendered again and graded, every case first asserts ON THE EXPECTATION that a byte changes, and every comparison is
np.array_equal.  Out-of-place targets are filled with 0xAB first, so a tile the walk never reaches shows as fill; in
place a tile visited twice shows because grading twice is not grading once (asserted of these tables below).

What the placement of the model guarantees (asserted on the flag snapshot, not on the kernel): the first and the last
tile row are flagged clean, at least two tiles in between are drawn and at least one is flagged.  Rows are walked in the
order k / ntx and only the column within a row is permuted, so with one workgroup (cap 1) that workgroup meets, whatever
the permutation: flagged tiles before its table is staged (late staging), a second drawn tile (the staged table
reused), and a flagged tile after staging (in place with c0 != 0: the flag lowered behind a barrier, and round again)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import test_composite as TC
from tests import test_grade as TG

from tiny_renderer_amd import grade_host

REPO = TG.REPO
scene, drive, snap, clean_flags, tiles_any = TC.scene, TC.drive, TC.snap, TC.clean_flags, TC.tiles_any
random_lut, lut_c0, expectation, device_buffer = TG.random_lut, TG.lut_c0, TG.expectation, TG.device_buffer
PIPE = TG.PIPE
C0S = ((0, 0, 0), (9, 0, 200))


# ------------------------------------------------------------------------------------------------------------------
# CPU
# ------------------------------------------------------------------------------------------------------------------

def test_diagnostic_declared_exported_and_typed(built):
    import tiny_renderer_amd as T
    from tiny_renderer_amd import _lib
    header = open(os.path.join(REPO, "include", "tiny_renderer.h")).read()
    assert re.search(r"int\s+tr_scene_debug_grade_grid\(tr_scene \*s, uint32_t cap\);", header)
    assert "#define TR_ABI_VERSION 3" in header, "the addition is additive"
    raw = C.CDLL(_lib.library_path())
    assert hasattr(raw, "tr_scene_debug_grade_grid"), "tr_scene_debug_grade_grid is not exported"
    assert _lib.SYMBOLS["tr_scene_debug_grade_grid"] == (C.c_int, [C.c_void_p, C.c_uint32])
    assert T.load_library().tr_abi_version() == 3
    assert callable(T.Scene.debug_grade_grid)
    integration = open(os.path.join(REPO, "INTEGRATION.md")).read()
    assert "fn tr_scene_debug_grade_grid(s: *mut TrScene, cap: u32) -> i32;" in integration


def test_diagnostic_refuses_a_null_scene(built):
    import tiny_renderer_amd as T
    from tiny_renderer_amd import _lib
    L = T.load_library()
    for cap in (0, 1, 0xFFFFFFFF):
        assert L.tr_scene_debug_grade_grid(None, cap) == _lib.TR_E_INVALID
        assert L.tr_last_error() == b"tr_scene_debug_grade_grid: null scene"
    # python: ValueError before anything reaches the library
    s = T.Scene.__new__(T.Scene)
    s.width, s.height, s._h, s._pinned = 64, 64, None, []
    for cap in (-1, 1 << 32, 2.0, True, None, "3"):
        with pytest.raises(ValueError):
            s.debug_grade_grid(cap)


# ------------------------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------------------------

# the model in tile columns 1 and 2 of tile rows 1..3; at 642 x 81 a second one across the right edge, so that the tile
# column of two pixels holds drawn pixels too
WALK_AT = {(640, 80): np.array([[-0.25, 0.0, 0.0, 0.4]], np.float32),
           (642, 81): np.array([[-0.25, 0.0, 0.0, 0.4], [1.1, 0.0, 0.0, 0.25]], np.float32)}
CAPS = lambda n_tiles: (1, 2, 3, 7, 16, n_tiles - 1)


def grid_after(s, cap):
    """The grid of the scene's most recent k_grade launch; the cap stays what it is."""
    return s.debug_grade_grid(cap)


def differing(got, want):
    return "%d bytes differ, %d hold the fill" % (int((got != want).sum()), int(((got == 0xAB) & (want != 0xAB)).sum()))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [17, 26])
@pytest.mark.parametrize("W,Hh", [(640, 80), (642, 81)])
def test_capped_walk_equals_the_host_rule(small_synthetic, W, Hh, n):
    """640 x 80: 5 x 5 tiles, whole words.  642 x 81: 6 x 6 tiles, guarded bytes, rows of 1926 bytes, a tile column two
    pixels wide and a tile row one row high.  n = 17 stages the table in LDS, n = 26 gathers from global memory.  The
    caps: G = 1; G < ntx; G coprime to ntx (2, 3, 7 against 5 and 6); G > ntx and no multiple of it (7, 16); a last
    round that one workgroup alone takes (n_tiles - 1)."""
    ntx, nty = (W + 127) // 128, (Hh + 15) // 16
    n_tiles = ntx * nty
    assert (ntx, nty) == {(640, 80): (5, 5), (642, 81): (6, 6)}[(W, Hh)]
    s = scene(W, Hh, small_synthetic, PIPE, WALK_AT[(W, Hh)], tap=True)
    assert s.debug_grade_grid(0) == 0, "no k_grade launch yet"
    drive(s)
    f, flags, before = snap(s), clean_flags(s), TG.state(s)
    assert flags.shape == (nty, ntx)
    assert flags[0].all() and flags[-1].all(), "the first and the last tile row must be flagged clean"
    assert (~flags[1:-1]).sum() >= 2, "two drawn tiles in between: the staged table is reused"
    assert flags[1:-1].any(), "a flagged tile in between"
    assert not (flags & tiles_any((f["fb"] != 0).any(-1)[::-1])).any()
    if W % 128:
        assert (f["fb"][:, W // 128 * 128:] != 0).any(), "nothing drawn in the partial tile column"
    for c0 in C0S:
        for cap in CAPS(n_tiles):
            where = "c0 %r, cap %d" % (c0, cap)
            # another table for every launch pair: what an earlier launch left in LDS is never the table wanted now
            lut = lut_c0(n, c0, 1000 * cap + 5 * n + W)
            want = expectation(f["fb"], lut)
            assert not np.array_equal(grade_host(want, lut), want), "grading twice must not be grading once"
            s.set_lut(lut)
            s.debug_grade_grid(cap)
            # out of place: every byte is stored over the fill, the frame and its flags stay
            drive(s)
            dev = device_buffer(W * Hh * 3)
            s.grade(out=dev.data_ptr())
            assert s.sync() == 0
            assert grid_after(s, cap) == min(cap, n_tiles), where
            got = dev.cpu().numpy().reshape(Hh, W, 3)
            assert np.array_equal(got, want), "out of place, %s: %s" % (where, differing(got, want))
            assert np.array_equal(clean_flags(s), flags), "an out-of-place call changed the frame's flags, " + where
            assert np.array_equal(s.get_frame_buffer(), f["fb"]), "an out-of-place call changed the frame, " + where
            # in place
            drive(s)
            assert np.array_equal(clean_flags(s), flags)
            s.grade()
            assert s.sync() == 0
            assert grid_after(s, cap) == min(cap, n_tiles), where
            after = clean_flags(s)
            if c0 == (0, 0, 0):
                assert np.array_equal(after, flags), "flagged tiles keep their flags where c0 is black, " + where
            else:
                assert not after.any(), "a tile that holds c0 != 0 is still flagged clean, " + where
            got = s.get_frame_buffer()
            assert np.array_equal(got, want), "in place, %s: %s" % (where, differing(got, want))
            if (W, Hh) == (640, 80):
                assert np.array_equal(s.resolve(2), TG.box(want, 2)), "resolve reads the flags, " + where
            TG.same_state(TG.state(s), before)
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [25, 33])
def test_noise_through_every_round(small_synthetic, n):
    """A caller's buffer of random bytes, rendered into without a clear and graded in place by three workgroups: 25 tiles,
    up to nine rounds a workgroup.  n = 25 is the largest table LDS holds, staged once and read in every round; n = 33
    the largest of the global form."""
    import torch
    W, Hh, cap = 640, 80, 3
    guard, nb = 64, W * Hh * 3
    noise = np.random.default_rng(n).integers(0, 256, nb, dtype=np.uint8)
    lut = random_lut(n, n + Hh)
    raw = np.concatenate([np.full(guard, 0xAA, np.uint8), noise, np.full(guard, 0xAA, np.uint8)])
    buf = torch.from_numpy(raw).cuda()
    torch.cuda.synchronize()
    s = scene(W, Hh, small_synthetic, PIPE, WALK_AT[(W, Hh)])
    s.set_lut(lut)
    s.debug_grade_grid(cap)
    s.set_frame_buffer_device(buf.data_ptr() + guard)
    drive(s, clear=False)
    fb = s.get_frame_buffer()
    assert len(np.unique(fb.reshape(-1, 3), axis=0)) > nb // 6, "the frame is not noise"
    assert not np.array_equal(fb.reshape(-1), noise), "nothing was drawn over the noise"
    want = expectation(fb, lut)
    assert not np.array_equal(grade_host(want, lut), want), "grading twice must not be grading once"
    s.grade()
    assert s.sync() == 0
    assert grid_after(s, cap) == cap
    got = buf.cpu().numpy()
    assert np.array_equal(got[guard:guard + nb].reshape(Hh, W, 3), want), "%d bytes differ" % int((got[guard:guard + nb] != want.reshape(-1)).sum())
    assert (got[:guard] == 0xAA).all() and (got[guard + nb:] == 0xAA).all(), "a guard byte changed"
    assert np.array_equal(s.get_frame_buffer(), want)
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("cap", [2, 4])
def test_band_scene_under_a_cap(small_synthetic, cap):
    """640 x 96, band rows (32, 80): three tile rows of five tiles behind a first tile row of 1 (ty_base != 0), walked by
    two workgroups (eight rounds) and by four."""
    W, Hh, band, c0 = 640, 96, (32, 80), (9, 0, 200)
    at = np.array([[-0.25, 0.0, 0.0, 0.7]], np.float32)
    whole = scene(W, Hh, small_synthetic, PIPE, at)
    drive(whole)
    ref = whole.get_frame_buffer()
    whole.close()
    assert ref[band[0]:band[1]].any()
    for n in (17, 26):
        lut = lut_c0(n, c0, 3 + n)
        want = expectation(ref[band[0]:band[1]], lut)
        s = scene(W, Hh, small_synthetic, PIPE, at, band_rows=band)
        s.set_lut(lut)
        s.debug_grade_grid(cap)
        drive(s)
        fb, flags = s.get_frame_buffer(), clean_flags(s)
        assert s.band_tiles().first_tile_row != 0 and flags.shape == (3, 5)
        assert flags.any() and (~flags).sum() >= 2, "the band needs flagged tiles and drawn ones"
        assert np.array_equal(fb[band[0]:band[1]], ref[band[0]:band[1]])
        out = device_buffer(W * Hh * 3)
        s.grade(out=out.data_ptr())
        assert s.sync() == 0
        assert grid_after(s, cap) == cap
        got = out.cpu().numpy().reshape(Hh, W, 3)
        assert np.array_equal(got[band[0]:band[1]], want), "n %d: %s" % (n, differing(got[band[0]:band[1]], want))
        assert (got[:band[0]] == 0xAB).all() and (got[band[1]:] == 0xAB).all(), "a row outside the band was written"
        assert np.array_equal(clean_flags(s), flags) and np.array_equal(s.get_frame_buffer(), fb)
        s.grade()
        assert s.sync() == 0
        assert grid_after(s, cap) == cap
        assert not clean_flags(s).any(), "a tile that holds c0 != 0 is still flagged clean"
        got = s.get_frame_buffer()
        assert np.array_equal(got[band[0]:band[1]], want), "in place, n %d: %s" % (n, differing(got[band[0]:band[1]], want))
        assert np.array_equal(got[:band[0]], fb[:band[0]]) and np.array_equal(got[band[1]:], fb[band[1]:]), "rows outside the band changed"
        s.close()


@pytest.mark.gpu
def test_the_uncapped_grid_takes_several_rounds(small_synthetic):
    """The launcher's own G, which nothing else checks: a frame 640 wide with 8 * CUs + 1 tiles or a few more -- the
    smallest that exceeds the bound GRADE_MAX_PER_CU puts on the grid (640 x 6560, 2050 tiles, on 256 CUs) -- so without
    a cap at least one workgroup goes round, at n = 25 (two workgroups a CU by the table's LDS) every one four times."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    W, c0 = 640, (9, 0, 200)
    Hh = 16 * -(-(8 * cus + 1) // 5)
    n_tiles = 5 * (Hh // 16)
    assert 8 * cus + 1 <= n_tiles < 8 * cus + 6
    s = scene(W, Hh, small_synthetic, PIPE)
    drive(s)
    fb, flags = s.get_frame_buffer(), clean_flags(s)
    assert flags.shape == (Hh // 16, 5) and flags.any() and (~flags).any(), "the frame needs flagged tiles and drawn ones"
    grids = {}
    for n in (17, 25, 33):
        lut = lut_c0(n, c0, n)
        want = expectation(fb, lut)
        s.set_lut(lut)
        drive(s)
        dev = device_buffer(W * Hh * 3)
        s.grade(out=dev.data_ptr())
        assert s.sync() == 0
        grids[n] = grid_after(s, 0)
        print("n %d: %d workgroups, %d tiles, %d CUs" % (n, grids[n], n_tiles, cus))
        assert 0 < grids[n] < n_tiles, "n %d: no workgroup went round (%d workgroups, %d tiles)" % (n, grids[n], n_tiles)
        got = dev.cpu().numpy().reshape(Hh, W, 3)
        assert np.array_equal(got, want), "out of place, n %d: %s" % (n, differing(got, want))
        assert np.array_equal(clean_flags(s), flags)
        s.grade()
        assert s.sync() == 0
        assert grid_after(s, 0) == grids[n]
        assert not clean_flags(s).any(), "a tile that holds c0 != 0 is still flagged clean"
        got = s.get_frame_buffer()
        assert np.array_equal(got, want), "in place, n %d: %s" % (n, differing(got, want))
    assert grids[25] < grids[17], "the LDS limit is not in force at n = 25: %r" % (grids,)
    s.close()
