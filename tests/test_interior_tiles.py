"""The interior form of the fused tile kernels (k_tile, INTERIOR -- csrc/tr_kernels.hip): compiled for frames made of whole
tiles only (width a multiple of TILE_W = 128, the band whole rows of TILE_H = 16 pixel high tiles inside the frame), without
the per-pixel frame and band tests of the general kernels.  Two things can go wrong: the launcher picks the form for a frame
that is not interior (the selection predicate), or a deleted test was needed after all (a store outside the frame or the
band).  So every case states which form must have run -- Scene.interior_tiles(), tr_scene_interior_tiles -- and compares every
byte with the CPU oracle; the band and the edge cases render into a caller's buffer that is filled with a sentinel and has
guard bytes on both sides.

The form exists for the four-wave column kernels, which a scene chooses by itself from 4096^2 up; the small frames here pin
that layout (tile_waves=4, tile_mode=1).  Three frames of different cameras by one render_frames call: the fused MODE 2
kernel (transient depth); `shadow` adds the depth pass and, with store_depth, MODE 1.
PARITY UNPINNED upstream: the oracle is the normative restatement (oracle/tr_oracle.h)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import helpers as H
from tests.test_frame_groups import oracle_frames
from tests.test_fused_parity import _grab, assert_fused_parity, oracle_views, view

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE_W, TILE_H = 128, 16            # csrc/tr_types.h
LAYOUT = dict(tile_waves=4, tile_mode=1, frames_per_launch=3)
VIEWS = np.stack([view(0.0, 0.0), view(0.4, -0.3), view(-0.7, 0.5)])
SENTINEL, GUARD = 0xA5, 4096
BIG_SCALE = 3.0   # (radius 0.8 -> 2.4: the frame lies inside the outline in all three views; asserted from the oracle)


def render_kept(W, Hh, mesh, texs, pipe, views=VIEWS, **opts):
    """One render_frames call of three frames into the scene's own targets: (interior?, the kept frames newest first)."""
    import tiny_renderer_amd as T
    gpu = T.Scene(W, Hh, mesh, texs, pipe, **dict(LAYOUT, **opts))
    assert gpu.frames_per_launch == 3
    assert not gpu.interior_tiles(), "nothing has been launched yet"
    gpu.render_frames(views)
    assert gpu.sync() == 0
    interior = gpu.interior_tiles()
    kept = []
    for back in range(gpu.frames_kept()):
        gpu.select_frame(back)
        kept.append(_grab(gpu, pipe))
    gpu.close()
    assert len(kept) == 3
    return interior, kept


def check_against_oracle(W, Hh, mesh, texs, pipe, want_interior, **opts):
    interior, kept = render_kept(W, Hh, mesh, texs, pipe, **opts)
    assert interior == want_interior, "%dx%d: the %s kernels ran" % (W, Hh, "interior" if interior else "general")
    want = oracle_views(W, Hh, mesh, texs, pipe, VIEWS)[::-1]
    assert_fused_parity(kept, want, pipe)


def render_into_guarded(W, Hh, mesh, texs, pipe, views=VIEWS, **opts):
    """The same call into a caller's buffers: each 3 W Hh bytes between two guards of GUARD bytes, everything filled with
    SENTINEL first.  Returns (interior?, [frame as [Hh, W, 3]], [guards of the frame, both concatenated])."""
    import torch
    import tiny_renderer_amd as T
    n, size = len(views), 3 * W * Hh
    bufs = [torch.full((GUARD + size + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda") for _ in range(n)]
    torch.cuda.synchronize()
    gpu = T.Scene(W, Hh, mesh, texs, pipe, frame_buffer_device=bufs[0].data_ptr() + GUARD, **dict(LAYOUT, **opts))
    gpu.render_frames(views, [b.data_ptr() + GUARD for b in bufs])
    assert gpu.sync() == 0
    interior = gpu.interior_tiles()
    torch.cuda.synchronize()
    host = [b.cpu().numpy() for b in bufs]
    gpu.close()
    return interior, [h[GUARD:GUARD + size].reshape(Hh, W, 3) for h in host], [np.concatenate([h[:GUARD], h[GUARD + size:]]) for h in host]


# ---- interior frames ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pipe", ["phong", "default"])
@pytest.mark.parametrize("size", [(2 * TILE_W, 2 * TILE_H), (TILE_W, 3 * TILE_H)])
def test_interior_frames_match_the_oracle(small_synthetic, size, pipe):
    """2 x 2 tiles and 1 x 3 tiles: the interior kernels run, and every frame is the oracle's byte for byte."""
    mesh, texs = small_synthetic
    check_against_oracle(size[0], size[1], mesh, texs, pipe, True)


@pytest.mark.parametrize("store_depth", [False, True])
def test_interior_shadow_passes_match_the_oracle(small_synthetic, store_depth):
    """shadow: the depth pass (FS_DEPTH, MODE 1) and the colour pass (FS_SHADOW2; MODE 2, with store_depth MODE 1) -- the
    query says interior only when every pass of the group ran the interior form; z and shadow bits are compared too."""
    mesh, texs = small_synthetic
    check_against_oracle(2 * TILE_W, 2 * TILE_H, mesh, texs, "shadow", True, store_depth=store_depth)


def test_other_layouts_keep_the_general_kernels(small_synthetic):
    """The form exists for the four-wave column kernels only: an interior frame in another layout runs the general ones."""
    mesh, texs = small_synthetic
    check_against_oracle(2 * TILE_W, 2 * TILE_H, mesh, texs, "phong", False, tile_waves=8)
    check_against_oracle(2 * TILE_W, 2 * TILE_H, mesh, texs, "phong", False, tile_mode=2)


# ---- the selection predicate: one pixel short or over ------------------------------------------------------------------

@pytest.mark.parametrize("pipe", ["phong", "default"])
@pytest.mark.parametrize("size", [(2 * TILE_W - 1, 2 * TILE_H), (2 * TILE_W - 4, 2 * TILE_H), (2 * TILE_W, 2 * TILE_H - 1),
                                  (2 * TILE_W + 1, 2 * TILE_H), (2 * TILE_W, 2 * TILE_H + 1)])
def test_frames_with_partial_tiles_keep_the_general_kernels(small_synthetic, size, pipe):
    """255 wide (byte stores), 252 wide (whole dwords, a partial last column), a row short, and a column or a row over:
    the general kernels, and the oracle's frames."""
    mesh, texs = small_synthetic
    check_against_oracle(size[0], size[1], mesh, texs, pipe, False)


# ---- bands ---------------------------------------------------------------------------------------------------------------

def check_band(mesh, texs, W, Hh, band, want_interior, pipe="phong"):
    interior, frames, guards = render_into_guarded(W, Hh, mesh, texs, pipe, band_rows=band)
    assert interior == want_interior, "band %r: the %s kernels ran" % (band, "interior" if interior else "general")
    expect = oracle_frames(W, Hh, mesh, texs, pipe, VIEWS, band=band)
    for i, (got, guard) in enumerate(zip(frames, guards)):
        want = expect[i][0]
        assert want[band[0]:band[1]].any(), "an empty band proves nothing"
        assert np.array_equal(got[band[0]:band[1]], want[band[0]:band[1]]), "frame %d: the band's rows differ" % i
        assert (got[:band[0]] == SENTINEL).all() and (got[band[1]:] == SENTINEL).all(), "frame %d: rows outside the band were written" % i
        assert (guard == SENTINEL).all(), "frame %d: bytes outside the frame buffer were written" % i


def test_band_of_whole_tile_rows_is_interior(small_synthetic):
    """Four tile rows, the band tile rows 1 and 2: interior -- and the rows of tile rows 0 and 3 stay as they were, which
    is what a missing row test would break if the band's tile grid were taken wrong."""
    mesh, texs = small_synthetic
    check_band(mesh, texs, 2 * TILE_W, 4 * TILE_H, (TILE_H, 3 * TILE_H), True)


def test_band_with_an_edge_inside_a_tile_row_is_general(small_synthetic):
    """The product's own partition (tr_band_rows) of four tile rows over three ranks, the middle rank: both band edges lie
    inside a tile row, whose other rows belong to the neighbours."""
    import tiny_renderer_amd as T
    mesh, texs = small_synthetic
    Hh = 4 * TILE_H
    band = T.band_rows(Hh, 3, 1)
    assert band[0] % TILE_H and band[1] % TILE_H
    check_band(mesh, texs, 2 * TILE_W, Hh, tuple(band), False)


def test_shadow_band_of_whole_tile_rows(small_synthetic):
    """shadow in a band: the colour pass covers the band, the depth pass the light's whole view."""
    mesh, texs = small_synthetic
    check_band(mesh, texs, 2 * TILE_W, 4 * TILE_H, (TILE_H, 3 * TILE_H), True, pipe="shadow")


# ---- geometry beyond every edge of the frame ----------------------------------------------------------------------------

def test_geometry_beyond_every_edge_of_an_interior_frame(small_synthetic):
    """The sphere enlarged until the frame lies inside its outline: polygons cross all four borders, every edge row and
    column of the frame is covered.  The frames are the oracle's, and the guard bytes before and behind the caller's
    buffers -- where a store for a pixel left of column 0 of the top row, or right of the last column of the bottom row,
    would land -- are untouched."""
    mesh, texs = small_synthetic
    big = dict(mesh, pos=(mesh["pos"] * np.float32(BIG_SCALE)).astype(np.float32))
    W, Hh = 2 * TILE_W, 2 * TILE_H
    interior, frames, guards = render_into_guarded(W, Hh, big, texs, "phong")
    assert interior
    expect = oracle_frames(W, Hh, big, texs, "phong", VIEWS)
    for i, (got, guard) in enumerate(zip(frames, guards)):
        want = expect[i][0]
        lit = want.any(-1)
        assert lit[0].all() and lit[-1].all() and lit[:, 0].all() and lit[:, -1].all(), "the model does not reach every border"
        assert np.array_equal(got, want), "frame %d differs at %d pixels" % (i, int((got != want).any(-1).sum()))
        assert (guard == SENTINEL).all(), "frame %d: bytes outside the frame buffer were written" % i



# ---- TR_INTERIOR=0 ------------------------------------------------------------------------------------------------------

def _child(out_path):
    """(a fresh process: the hook is read once)  The 2 x 2 case's frames and which kernels ran, into an .npz file."""
    import tiny_renderer_amd as T
    mesh, texs = T.synthetic_scene(n_lat=12, n_lon=24, tex_size=256)
    interior, kept = render_kept(2 * TILE_W, 2 * TILE_H, mesh, texs, "phong")
    np.savez(out_path, interior=np.array(interior), rgb=np.stack([k["rgb"] for k in kept]), z=np.stack([k["z"] for k in kept]))


def test_the_switch_forces_the_general_kernels(small_synthetic, tmp_path):
    """TR_INTERIOR=0: the same build runs the general kernels on an interior frame and produces the same bytes."""
    mesh, texs = small_synthetic
    interior, kept = render_kept(2 * TILE_W, 2 * TILE_H, mesh, texs, "phong")
    assert interior
    out = str(tmp_path / "general.npz")
    env = dict(os.environ, TR_INTERIOR="0")
    subprocess.run([sys.executable, "-c", "import sys; from tests.test_interior_tiles import _child; _child(sys.argv[1])", out],
                   cwd=REPO, env=env, check=True, timeout=300)
    got = np.load(out)
    assert not bool(got["interior"]), "TR_INTERIOR=0 did not switch the interior kernels off"
    assert np.array_equal(got["rgb"], np.stack([k["rgb"] for k in kept]))
    assert np.array_equal(got["z"], np.stack([k["z"] for k in kept]))
    assert got["rgb"].any()
