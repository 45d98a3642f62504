"""What can be decided without a GPU about the cases of tests/test_warp_consumers.py: with the CPU oracle's frame and z of
each size and the library's host rules alone, that the `shift` grid reaches the two states of disagreeing fast-clear
flags (tests/warp_consumer_cases.py), that every chained expectation differs from its input and from the same consumer
over the frame no stage touched, and that the mask "z bits changed" decides every pixel of a render without a clear.

(A tile counts as drawn here when the oracle draws a pixel in it; the scene's flags go by the polygons' boxes, which the
GPU cases assert on the device's own flags.)"""
import numpy as np
import pytest

from tests import helpers as H
from tests import test_composite as TC
from tests import test_postprocess_chain as PC
from tests import warp_consumer_cases as K

bits, tiles_any = K.bits, K.tiles_any
_FRAMES = {}


def cpu(ms, W, Hh, at=None, cam=K.CAM, light=K.LIGHT, which="model"):
    """The oracle's snapshot, computed once and left alone."""
    at = K.PLACE[(W, Hh)] if at is None else at
    key = (which, W, Hh, cam, light)
    if key not in _FRAMES:
        f = PC._cpu(W, Hh, ms, at, K.PIPE, cam, light)
        for a in (f["fb"], f["z"]):
            a.setflags(write=False)
        _FRAMES[key] = f
    return _FRAMES[key]


def cpu_pair(ms, W, Hh):
    """The oracle's snapshots after the first render and after a second one, from K.TOP_CAM of the size, without a clear."""
    import tiny_renderer_amd as T
    from oracle import oracle as O
    s = O.Scene(W, Hh, T.apply_instances(ms[0], K.PLACE[(W, Hh)]), ms[1], K.PIPE)
    out = []
    for cam, clear in ((K.CAM, True), (K.TOP_CAM[(W, Hh)], False)):
        TC.drive(s, cam, K.LIGHT, clear)
        out.append({"fb": s.get_frame_buffer(), "z": s.z_f32(), "win": None})
    s.close()
    return out


def test_the_shift_reaches_both_states(built, small_synthetic):
    """384 x 48 under a black border: a tile with drawn z whose output is all zeros and whose footprint -- the bound of
    tr_warp.h restated over the tile's nodes -- lies outside the image or on undrawn source tiles only (state A), and an
    undrawn tile that receives colour (state B).  rotate7 reaches both partially: drawn tiles lose pixels, undrawn ones
    gain some.  Under another border every undrawn tile holds colour.  At both sizes the shifted colour lands on the
    drawn depth of the second instance (K.LANDING), so that the consumers that only work where colour lies over drawn
    depth -- k_ao plain, k_dof with a sharp background -- have work behind the shift."""
    W, Hh = K.MIDDLE
    f = cpu(small_synthetic, W, Hh)
    staged = K.stage_host("shift", f["fb"])
    drawn_tiles = tiles_any(K.drawn(f))
    a, b = K.state_a(f, staged), K.state_b(f, staged)
    assert a.any(), "no drawn tile warps to zeros"
    assert b.any(), "no undrawn tile receives colour"
    proven = K.state_a_by_the_footprint(f, staged)
    assert proven.any(), "no state-A tile has its whole footprint outside the image or on undrawn tiles"
    # (the others are zeros over drawn z too, with a footprint that touches a drawn tile: their flag stays down)
    assert (a & ~proven).any() and proven[:, 0].all(), "the left tile column moves out whole"
    turned = K.stage_host("rotate7", f["fb"])
    moved_out = K.drawn(f) & ~turned[::-1].any(-1)
    moved_in = ~K.drawn(f) & turned[::-1].any(-1)
    assert moved_out.sum() > 50 and moved_in.sum() > 50, "rotate7 moves colour neither out of drawn pixels nor into undrawn ones"
    assert K.state_b(f, turned).any(), "rotate7 turns colour into no undrawn tile"
    paper = K.stage_host("shift_paper", f["fb"])
    assert (K.lit(paper) | drawn_tiles).all() and K.state_b(f, paper).sum() == int((~drawn_tiles).sum())
    for size in (K.MIDDLE, K.NARROW):
        g = cpu(small_synthetic, *size)
        over = K.drawn(g) & K.stage_host("shift", g["fb"])[::-1].any(-1)
        assert over.sum() >= 30, "%r: the shifted colour lands on no drawn depth" % (size,)


def test_the_narrow_frame_has_partial_tiles_and_colour_in_them(built, small_synthetic):
    W, Hh = K.NARROW
    f = cpu(small_synthetic, W, Hh)
    assert W % 128 and Hh % 16
    d = K.drawn(f)
    assert d[:, W // 128 * 128:].any() and d[Hh // 16 * 16:].any(), "the model misses the partial tile column or row"
    for name in ("shift", "rotate7", "gaussian31"):
        staged = K.stage_host(name, f["fb"])
        assert staged.any() and not np.array_equal(staged, f["fb"]), name
    assert K.state_b(f, K.stage_host("shift", f["fb"])).any(), "the shift moves colour into no undrawn tile"


@pytest.mark.parametrize("W,Hh", [K.MIDDLE, K.NARROW])
def test_convolve_cases(built, small_synthetic, W, Hh):
    """gaussian31 under a black border spills into undrawn tiles; emboss with bias 128 under another border leaves no tile
    black; unsharp under clamp changes the frame.  (No flag can stay up far from the model at these sizes: k_convolve
    keeps a tile's flag only where the tile and all its neighbours are flagged, and the drawn centre tile of 3 x 3, or
    the drawn middle row of 2 x 3, neighbours every tile.  The GPU file asserts that none is up.)"""
    f = cpu(small_synthetic, W, Hh)
    blur = K.stage_host("gaussian31", f["fb"])
    spill = ~K.drawn(f) & blur[::-1].any(-1)
    assert spill.sum() > 50, "the blur spills into no undrawn pixel"
    assert K.state_b(f, blur).any(), "the blur spills into no undrawn tile"
    assert K.lit(K.stage_host("emboss", f["fb"])).all()
    assert not np.array_equal(K.stage_host("unsharp", f["fb"]), f["fb"])


CHAINS = [(st, size) for st in ("shift", "rotate7", "shift_paper", "gaussian31", "emboss") for size in (K.MIDDLE, K.NARROW)]


@pytest.mark.parametrize("stage,size", CHAINS, ids=["%s-%dx%d" % (st, sz[0], sz[1]) for st, sz in CHAINS])
def test_every_chained_expectation_tells(built, small_synthetic, stage, size):
    """Each consumer over (staged colour, z of before) differs from its input -- every one, at every stage and size --
    and from the same consumer over the frame no stage touched: a consumer that did nothing or ignored the stage, or a
    stage that did nothing, fails the GPU case.  (K.COLOUR_BLIND, the ink-over-paper outline, reads no colour by its
    rule: it is exempt from the second condition alone.)"""
    W, Hh = size
    f = cpu(small_synthetic, W, Hh)
    staged = K.stage_host(stage, f["fb"])
    assert not np.array_equal(staged, f["fb"]), "the stage changes nothing"
    after = dict(f, fb=staged)
    for name in K.DEPTH_CONSUMERS + K.COLOUR_CONSUMERS:
        host, _ = K.consumer(name, f)
        want, plain = host(after), host(f)
        if K.is_getter(name):
            same = want == plain if name != "yuv" else all(np.array_equal(a, b) for a, b in zip(want, plain))
            assert not same, "%s: the record of the staged frame is that of the frame itself" % name
            continue
        if name not in K.COLOUR_BLIND:
            assert not np.array_equal(want, plain), "%s: the staged frame's expectation is the unstaged one's" % name
        assert not np.array_equal(want, staged), "%s changes nothing" % name


def test_both_orders_differ(built, small_synthetic):
    import tiny_renderer_amd as T
    for W, Hh in (K.MIDDLE, K.NARROW):
        f = cpu(small_synthetic, W, Hh)
        for warp, conv in K.ORDER_PAIRS:
            a = K.stage_host(conv, K.stage_host(warp, f["fb"]))
            b = K.stage_host(warp, K.stage_host(conv, f["fb"]))
            assert not np.array_equal(a, b), (W, Hh, warp, conv)
        p = K.TD.params_for(f, 3, bg=2)
        for warp in ("shift", "rotate7"):
            a = T.depth_of_field_host(f["z"], K.stage_host(warp, f["fb"]), p)
            b = K.stage_host(warp, T.depth_of_field_host(f["z"], f["fb"], p))
            assert not np.array_equal(a, b), (W, Hh, warp, "dof")


@pytest.mark.parametrize("W,Hh", [K.MIDDLE, K.NARROW])
def test_composite_cases(built, small_synthetic, W, Hh):
    """The other scene wins pixels and loses pixels against the model on either side; at 384 x 48 it wins inside a
    state-A tile and leaves pixels of it alone (the warped scene as dst), and the warped scene's drawn depth wins pixels
    of a state-A tile against it (as src): zero colour travels with depth."""
    import tiny_renderer_amd as T
    other = T.synthetic_scene(n_lat=9, n_lon=17, tex_size=128, radius=0.75)
    f = cpu(small_synthetic, W, Hh)
    o = cpu(other, W, Hh, at=K.OTHER_AT[(W, Hh)], light=K.OTHER_LIGHT, which="other")
    staged = K.stage_host("shift", f["fb"])
    warped = dict(f, fb=staged)
    as_dst, wins_d = TC.merge(warped, o)
    as_src, wins_s = TC.merge(o, warped)
    assert wins_d.any() and (K.drawn(o) & ~wins_d).any() and wins_s.any() and (K.drawn(f) & ~wins_s).any()
    assert not np.array_equal(as_dst["fb"], TC.merge(f, o)[0]["fb"]) and not np.array_equal(as_src["fb"], TC.merge(o, f)[0]["fb"])
    if (W, Hh) == K.MIDDLE:
        a = K.tile_pixels(K.state_a_by_the_footprint(f, staged), Hh, W)
        assert (a & wins_d).any() and (a & ~wins_d).any(), "src wins nothing, or everything, inside the state-A tiles"
        assert (a & wins_s).any(), "the warped scene's depth wins no pixel of a state-A tile"
        assert o["fb"][::-1][a & wins_s].any(), "where the state-A tile wins, dst held no colour anyway"


@pytest.mark.parametrize("W,Hh", [K.MIDDLE, K.NARROW])
def test_the_changed_z_bits_decide_every_pixel_of_a_render_without_a_clear(built, small_synthetic, W, Hh):
    """In the oracle's pair of frames -- a render, then another camera without a clear -- no pixel changes colour while
    its z bits stay equal: the mask decides every pixel.  The second render wins pixels inside a state-A tile and leaves
    pixels of it alone, and the expectation differs from both of the twin's frames."""
    first, second = cpu_pair(small_synthetic, W, Hh)
    changed_z = bits(second["z"]) != bits(first["z"])
    changed_c = (second["fb"] != first["fb"]).any(-1)[::-1]
    assert changed_z.any() and not (changed_c & ~changed_z).any(), "a pixel changed colour and kept its z bits"
    assert (K.drawn(first) & ~changed_z).any(), "the second render wins every drawn pixel"
    for stage in K.ON_TOP_STAGES:
        staged = K.stage_host(stage, first["fb"])
        want, won = K.on_top(first, second, staged)
        assert np.array_equal(won, changed_z)
        assert not np.array_equal(want, second["fb"]) and not np.array_equal(want, staged)
    if (W, Hh) == K.MIDDLE:
        staged = K.stage_host("shift", first["fb"])
        a = K.tile_pixels(K.state_a_by_the_footprint(first, staged), Hh, W)
        assert (a & changed_z).any() and (a & ~changed_z).any(), "the second render misses the state-A tiles or fills them"


def test_posed_frames_and_the_callers_buffer(built, small_synthetic):
    """208 x 64: the warp and the blur that follows change the selected frame of the posed group, whose poses differ.
    256 x 48 on noise: the shift under another border, then the outline, each change the dense frame."""
    import tiny_renderer_amd as T
    from tests import dense_cases as DC
    from tests import test_dense_frames_host as TH
    W, Hh = K.POSED
    par = PC.TCC.frame_params(PC.POSED_N)
    frames = []
    for i in range(PC.POSED_N):
        m, at = PC.twin_mesh(K.POSED_KIND, small_synthetic[0], 0.5 * i)
        frames.append(PC._cpu(W, Hh, (m, small_synthetic[1]), at, q=par[i]))
    sel, other = frames[PC.POSED_N - 1 - K.POSED_BACK], frames[PC.POSED_N - 1]
    staged = K.stage_host(K.POSED_STAGE, sel["fb"])
    p = K.TD.params_for(sel, 3, bg=1)
    want = T.depth_of_field_host(sel["z"], staged, p)
    assert not np.array_equal(staged, sel["fb"]) and not np.array_equal(want, staged)
    assert not np.array_equal(T.depth_of_field_host(other["z"], staged, p), want), "another pose's depth would not show"
    assert not np.array_equal(T.depth_of_field_host(sel["z"], sel["fb"], p), want)
    W, Hh = K.DENSE
    f = TH.dense(small_synthetic, W, Hh, "noise")
    staged = K.stage_host("shift_paper", f["fb"])
    op = T.outline_params(**K.outline_kw(False))
    want = T.outline_host(f["z"], staged, op)
    assert not np.array_equal(staged, f["fb"]) and not np.array_equal(want, staged)
    assert not np.array_equal(want, T.outline_host(f["z"], f["fb"], op))
    assert (staged == np.array(K.WC.PAPER, np.uint8)).all(-1).any(), "no border colour comes in"
