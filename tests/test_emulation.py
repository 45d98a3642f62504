"""The GPU algorithm on the CPU: the product's vertex/fragment/coverage functions
(tiny_renderer_amd/csrc/tr_shaders.h, tr_prepare.cpp, compiled for the host by tests/emul) run
through the kernels' decomposition -- per-tile bins visited in REVERSE order, max over (z, index),
shade the survivors -- must reproduce the oracle's serial loop bit for bit.  Catches arithmetic
and ordering mistakes without a GPU; the GPU tests then only have to confirm the device
arithmetic."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import emul_bind as E
from tests import helpers as H

PIPES = ("default", "phong", "normal_map", "specular", "darboux", "shadow", "occlusion")


def run_both(W, Hh, mesh, texs, pipe, ca, la):
    s = O.Scene(W, Hh, mesh, texs, pipe)
    s.clear()
    s.set_light_direction(H.light(la))
    s.set_camera(*H.camera(ca))
    assert s.render() == 0
    err, z, sh, fb, win = E.render(W, Hh, mesh, texs, pipe, H.light(la), H.camera(ca))
    assert err == 0
    return s, z, sh, fb, win


def assert_same(s, z, sh, fb, win, pipe):
    assert np.array_equal(z.view(np.uint32), s.z_f32().view(np.uint32))
    assert np.array_equal(win, s.winner_u32())
    if pipe in ("shadow", "occlusion"):
        assert np.array_equal(sh.view(np.uint32), s.shadow_f32().view(np.uint32))
    assert np.array_equal(fb, s.get_frame_buffer())   # exact, powf included: same libm on the host


@pytest.mark.parametrize("pipe", PIPES)
def test_synthetic(synthetic, pipe):
    mesh, texs = synthetic
    assert_same(*run_both(400, 300, mesh, texs, pipe, 0.5, -0.8), pipe)


@pytest.mark.parametrize("pipe", PIPES)
def test_diablo_800(diablo, pipe):
    mesh, texs = diablo
    import ctypes as C
    before = (C.c_uint64 * 2)()
    E.lib().tr_emul_pair_counts(before)
    assert_same(*run_both(800, 800, mesh, texs, pipe, 0.7, -1.1), pipe)
    if pipe in ("normal_map", "specular", "darboux"):
        # the two-pixel closures really ran in their fast form (a guard that always failed would leave
        # the comparison above vacuous): more than nine pixel pairs in ten on this model
        after = (C.c_uint64 * 2)()
        E.lib().tr_emul_pair_counts(after)
        fast, plain = after[0] - before[0], after[1] - before[1]
        assert fast > 9 * plain and fast > 10000, (fast, plain)


@pytest.mark.parametrize("pipe", ("phong", "normal_map", "specular", "darboux"))
def test_interleaved_texel_set_is_the_plain_images(synthetic, pipe, monkeypatch):
    """The closures fetch their texels from ONE interleaved, tiled array (tr_texels.h: pack_texels / packed_index /
    fetch_texels) when the four images have one size -- the default above -- and image by image otherwise: both forms
    give the oracle's frame, on images whose sides are not multiples of the 8x4 / 4x4 / 4x2 blocks either."""
    mesh, texs = synthetic
    odd = [np.ascontiguousarray(t[:250, :203]) for t in texs]   # 203 x 250 texels: partial blocks on both sides
    for images in (texs, odd):
        monkeypatch.delenv("TR_EMUL_PLAIN_TEXELS", raising=False)
        assert_same(*run_both(320, 240, mesh, images, pipe, 0.4, -0.7), pipe)
        monkeypatch.setenv("TR_EMUL_PLAIN_TEXELS", "1")
        assert_same(*run_both(320, 240, mesh, images, pipe, 0.4, -0.7), pipe)


def test_african_head_default(african_head):
    mesh, texs = african_head
    assert_same(*run_both(800, 800, mesh, texs, "default", 0.0, 0.0), "default")


def test_accumulate_without_clear(small_synthetic):
    mesh, texs = small_synthetic
    W, Hh = 200, 150
    s = O.Scene(W, Hh, mesh, texs, "shadow")
    s.clear()
    bufs = None
    for i, (ca, la) in enumerate([(0.0, 0.0), (0.6, 0.9)]):
        s.set_light_direction(H.light(la))
        s.set_camera(*H.camera(ca))
        assert s.render() == 0
        err, z, sh, fb, win = E.render(W, Hh, mesh, texs, "shadow", H.light(la), H.camera(ca),
                                       fresh=1 if i == 0 else 0, bufs=bufs)
        bufs = (z, sh, fb, win)
    assert np.array_equal(z.view(np.uint32), s.z_f32().view(np.uint32))
    assert np.array_equal(sh.view(np.uint32), s.shadow_f32().view(np.uint32))
    assert np.array_equal(fb, s.get_frame_buffer())


def test_bands_reassemble(small_synthetic):
    mesh, texs = small_synthetic
    W, Hh = 256, 200
    s, z, sh, fb, win = run_both(W, Hh, mesh, texs, "phong", 0.3, 0.3)
    out = np.zeros_like(fb)
    for r0, r1 in ((0, 37), (37, 120), (120, 200)):
        _, _, _, part, _ = E.render(W, Hh, mesh, texs, "phong", H.light(0.3), H.camera(0.3), band=(r0, r1))
        out[r0:r1] = part[r0:r1]
    assert np.array_equal(out, fb)


MASK_SEEDS = range(6)


@pytest.mark.parametrize("seed", MASK_SEEDS)
def test_pair_masks_never_lose_a_fragment(seed):
    """k_setup stores with every (polygon, tile) pair which cells / block columns of the box can hold a
    fragment (pair_masks, tr_shaders.h) and the tile kernel looks nowhere else.  The emulation skips the
    same pixels: far-away vertices, slivers and nearly collinear triples (edge functions that round in
    f32) are where a margin that is too small would lose fragments -- the frame must stay the oracle's
    and no covered pixel may lie outside the masks."""
    from tests.test_random_meshes import far_case
    (W, Hh), _, _, mesh, texs = far_case(seed, base=7000)
    before = E.mask_counts()
    s = O.Scene(W, Hh, mesh, texs, "phong")
    s.clear()
    s.set_light_direction(H.light(0.4))
    s.set_camera(*H.camera(0.0))
    if s.render() != 0:
        pytest.skip("the reference would panic on this soup")
    err, z, sh, fb, win = E.render(W, Hh, mesh, texs, "phong", H.light(0.4), H.camera(0.0))
    after = E.mask_counts()
    assert after[0] == before[0], "covered pixels outside the pair masks"
    assert np.array_equal(win, s.winner_u32())
    assert np.array_equal(z.view(np.uint32), s.z_f32().view(np.uint32))
    assert np.array_equal(fb, s.get_frame_buffer())


def test_pair_masks_cull_cells(diablo):
    """... and they do cull: on diablo at 800x800 fewer than two thirds of the small pairs' box cells stay."""
    mesh, texs = diablo
    before = E.mask_counts()
    assert_same(*run_both(800, 800, mesh, texs, "phong", 0.7, -1.1), "phong")
    after = E.mask_counts()
    assert after[0] == before[0]
    live, box = after[1] - before[1], after[2] - before[2]
    assert box > 10000 and live < 0.67 * box, (live, box)
