"""The frame stages at the two ends of the frame sizes, on the host: every host rule against the suite's numpy restatement
over the dense frames of tests/extreme_cases.py -- frames below one 128 x 16 tile, down to one pixel, and frames with a
side of 32768 -- and the proof that those frames reach what each size is for.

The GPU cases of tests/test_frame_extremes.py compare the device with the host rule over the device's OWN snapshot, and
one of them shows that snapshot to be the frame built here (the oracle's drawn pixels pasted over the backdrop).  What is
asserted here about that frame therefore holds for the device's.  On the long frames one parameter set a stage runs, so
that the numpy rules stay affordable.

Every comparison is np.array_equal."""
import numpy as np
import pytest

from tests import aa_cases as AC
from tests import convolve_cases as CC
from tests import dense_cases as DC
from tests import extreme_cases as EC
from tests import helpers as H
from tests import outline_cases as OC
from tests import resize_cases as RC
from tests import warp_cases as WC
from tests import yuv_cases as YC

bits, F32_MIN_BITS = EC.bits, EC.F32_MIN_BITS
NO_WINNER = 0xFFFFFFFF
ALL_SIZES = EC.SIZES + (EC.RESOLVE_LONG,)
_frames = {}


def sizes(which=ALL_SIZES):
    return pytest.mark.parametrize("W,Hh", which, ids=["%dx%d" % s for s in which])


def rendered(ms, W, Hh):
    """The oracle's frame of the model on a cleared buffer, once per size: (colour, z, winner words)."""
    if (W, Hh) not in _frames:
        import tiny_renderer_amd as T
        from oracle import oracle as O
        mesh, texs = EC.model(ms, W, Hh)
        at = EC.table(W, Hh)
        s = O.Scene(W, Hh, mesh if at is None else T.apply_instances(mesh, at), texs, EC.PIPE)
        s.clear()
        s.set_light_direction(H.light(EC.LIGHT)), s.set_camera(*H.camera(EC.CAM))
        assert s.render() == 0, "the reference panics on this frame"
        _frames[W, Hh] = (s.get_frame_buffer(), s.z_f32(), s.winner_u32())
        s.close()
    return _frames[W, Hh]


def dense(ms, W, Hh):
    """{"fb", "z", "back", "drawn" (z's orientation)}: the frame the device produces from the backdrop."""
    fb, z, _ = rendered(ms, W, Hh)
    back = EC.backdrop(W, Hh)
    f = {"fb": DC.paste(back, fb, z), "z": z, "back": back, "drawn": bits(z) != F32_MIN_BITS}
    assert (f["fb"][~f["drawn"][::-1]] == back[~f["drawn"][::-1]]).all()
    return f


def differ(got, want, what):
    assert got.shape == want.shape and np.array_equal(got, want), "%r: %d bytes differ" % (what, int((got != want).sum()))


# ----------------------------------------------------------------------------------------------------------------------
# what the frames reach
# ----------------------------------------------------------------------------------------------------------------------

@sizes()
def test_the_model_draws_where_it_can(built, small_synthetic, W, Hh):
    """Drawn and undrawn pixels both exist wherever the model draws at all; at EC.DRAWS_NOTHING no sphere and no flat mesh
    over the whole view leaves a pixel, so the depth stages run on an all-undrawn depth there."""
    import tiny_renderer_amd as T
    from oracle import oracle as O
    f = dense(small_synthetic, W, Hh)
    assert EC.REASON.get((W, Hh)) or (W, Hh) == EC.RESOLVE_LONG
    if EC.draws(W, Hh):
        assert f["drawn"].any() and not f["drawn"].all(), "the model covers part of the backdrop"
        assert not np.array_equal(f["fb"], f["back"])
        if (W, Hh) in EC.DEPTH_CHANGES:
            assert f["drawn"].sum() > 50 and len(np.unique(f["z"][f["drawn"]])) > 24, "dozens of distinct depths"
        return
    assert not f["drawn"].any() and np.array_equal(f["fb"], f["back"])
    # ... and not for want of trying: the spheres of every table of the suite, and a square over the whole view
    whole = dict(EC.flat_mesh(), pos=np.array([[-4, -4, 0], [4, -4, 0], [4, 4, 0], [-4, 4, 0]], np.float32))
    for mesh in [T.apply_instances(small_synthetic[0], at) for at in (EC.TWO, OC.AT_SMALL, OC.AT_WIDE, np.array([[0, 0, 0, 3.0]], np.float32))] + [whole]:
        s = O.Scene(W, Hh, mesh, small_synthetic[1], EC.PIPE)
        s.clear()
        s.set_light_direction(H.light(EC.LIGHT)), s.set_camera(*H.camera(EC.CAM)), s.render()
        assert (bits(s.z_f32()) == F32_MIN_BITS).all(), "a model does draw at %d x %d: use it" % (W, Hh)
        s.close()
    # the square does draw where the frame has two pixels a side (3 x 2 is drawn with half of it)
    s = O.Scene(3, 2, whole, small_synthetic[1], EC.PIPE)
    s.clear()
    s.set_light_direction(H.light(EC.LIGHT)), s.set_camera(*H.camera(EC.CAM)), s.render()
    assert (bits(s.z_f32()) != F32_MIN_BITS).all()
    s.close()


def test_32768_columns_reach_the_upper_half_of_the_16_bit_fields(built, small_synthetic):
    """On 32768 x 17 a drawn pixel lies in a tile column at or past 128, the last column is drawn, and a polygon's box
    ends past 16383 (the polygon that wins a pixel there covers it, so its box holds it); on 20 x 32768 a drawn pixel
    lies in a tile row past 1024."""
    fb, z, win = rendered(small_synthetic, 32768, 17)
    ys, xs = np.nonzero(win != NO_WINNER)
    assert (xs // 128 >= 128).any() and xs.max() == 32767
    far = np.unique(win[:, 16384:][win[:, 16384:] != NO_WINNER])
    assert far.size > 10, "polygons whose box has bx1 > 16383"
    both = np.intersect1d(far, np.unique(win[:, :16384]))
    assert both.size > 0, "a polygon's box spans column 16384: bx0 <= 16383 < bx1"
    fb, z, win = rendered(small_synthetic, 20, 32768)
    ys, xs = np.nonzero(win != NO_WINNER)
    assert (ys // 16 >= 1024).any() and (ys // 16 < 1024).any() and len(np.unique(ys // 16)) > 512


@pytest.mark.parametrize("pipe", ["phong", "shadow"])
@sizes(EC.LONG)
def test_the_reference_renders_the_parity_cases(built, small_synthetic, W, Hh, pipe):
    """The oracle reports no panic of the reference for the frames tests/test_frame_extremes.py compares with it: the
    single render, and the six of the render_frames call.  (It does report one at 20 x 32768 under the suite's light in
    the shadow pipeline: EC.parity_light.)"""
    import tiny_renderer_amd as T
    from oracle import oracle as O
    from tests import test_resolve as TR
    s = O.Scene(W, Hh, T.apply_instances(small_synthetic[0], EC.table(W, Hh)), small_synthetic[1], pipe)
    s.clear()
    s.set_light_direction(H.light(EC.parity_light(W, Hh, pipe))), s.set_camera(*H.camera(EC.CAM))
    assert s.render() == 0
    for q in TR._params(6):
        s.clear(), s.set_light_direction(q[0:3]), s.set_camera(q[3:6], q[6:9], q[9:12])
        assert s.render() == 0
    if (W, Hh, pipe) == (20, 32768, "shadow"):
        s.clear()
        s.set_light_direction(H.light(EC.LIGHT)), s.set_camera(*H.camera(EC.CAM))
        assert s.render() == 16, "TRO_E_SHADOW_OOB"
    s.close()


# ----------------------------------------------------------------------------------------------------------------------
# the rules
# ----------------------------------------------------------------------------------------------------------------------

def changed(stage, W, Hh, wants, fb):
    if EC.must_change(stage, W, Hh):
        assert any(not np.array_equal(w, fb) for w in wants), "no parameter set of %s changes the frame" % stage


@sizes(EC.SIZES)
def test_aa(built, small_synthetic, W, Hh):
    import tiny_renderer_amd as T
    f = dense(small_synthetic, W, Hh)
    wants = []
    for kw in EC.aa_sets(W, Hh):
        wants.append(AC.rule_np(f["fb"], **kw)["out"])
        differ(T.aa_host(f["fb"], T.aa_params(**kw)), wants[-1], kw)
    changed("aa", W, Hh, wants, f["fb"])
    if (W, Hh) == (1, 1):
        assert np.array_equal(wants[0], f["fb"]), "one pixel has no edge"


@sizes(EC.SIZES)
def test_bloom(built, small_synthetic, W, Hh):
    import tiny_renderer_amd as T
    from tests import test_bloom as TB
    f = dense(small_synthetic, W, Hh)
    wants = []
    for q in EC.bloom_sets(W, Hh):
        wants.append(TB.rule(f["fb"], *q))
        differ(T.bloom_host(f["fb"], TB.P(*q)), wants[-1], q)
    changed("bloom", W, Hh, wants, f["fb"])


@sizes(EC.SIZES)
def test_grade(built, small_synthetic, W, Hh):
    import tiny_renderer_amd as T
    from tests import test_grade as TG
    f = dense(small_synthetic, W, Hh)
    wants = []
    for lut in EC.grade_luts(W, Hh):
        wants.append(TG.rule(f["fb"], lut))
        differ(T.grade_host(f["fb"], lut), wants[-1], lut.shape[0])
    changed("grade", W, Hh, wants, f["fb"])


@sizes(EC.SIZES)
def test_convolve(built, small_synthetic, W, Hh):
    import tiny_renderer_amd as T
    f = dense(small_synthetic, W, Hh)
    ALL = CC.everything()
    wants = []
    for name, edge, border in EC.convolve_sets(W, Hh):
        wants.append(CC.rule(f["fb"], ALL[name], edge, border))
        differ(T.convolve_host(f["fb"], CC.params(ALL[name], edge, border)), wants[-1], (name, edge, border))
    changed("convolve", W, Hh, wants, f["fb"])


@sizes(EC.SIZES)
def test_outline(built, small_synthetic, W, Hh):
    import tiny_renderer_amd as T
    f = dense(small_synthetic, W, Hh)
    wants = []
    for kw in EC.outline_sets(W, Hh):
        wants.append(OC.rule_np(f["z"], f["fb"], **kw))
        differ(T.outline_host(f["z"], f["fb"], T.outline_params(**kw)), wants[-1], kw)
    assert any(kw["radius"] == 3 for kw in EC.outline_sets(W, Hh))
    changed("outline", W, Hh, [w for w, kw in zip(wants, EC.outline_sets(W, Hh)) if not kw.get("only")], f["fb"])
    if not EC.draws(W, Hh):
        for w, kw in zip(wants, EC.outline_sets(W, Hh)):
            assert kw.get("only") or np.array_equal(w, f["fb"]), "nothing drawn: no ink"


@sizes(EC.SIZES)
def test_ambient_occlusion(built, small_synthetic, W, Hh):
    import tiny_renderer_amd as T
    from tests import test_ambient_occlusion as TA
    f = dense(small_synthetic, W, Hh)
    wants = []
    for kw in EC.ao_sets(W, Hh):
        assert kw["radius"] == 8
        wants.append(TA.rule(f["z"], f["fb"], **kw))
        differ(T.ambient_occlusion_host(f["z"], f["fb"], **kw), wants[-1], kw)
        assert np.array_equal(wants[-1][~f["drawn"][::-1]], f["back"][~f["drawn"][::-1]]), "the backdrop is kept"
    changed("ao", W, Hh, wants[:1], f["fb"])


@sizes(EC.SIZES)
def test_depth_of_field(built, small_synthetic, W, Hh):
    import tiny_renderer_amd as T
    from tests import test_depth_of_field as TD
    f = dense(small_synthetic, W, Hh)
    wants = []
    for p in EC.dof_sets(f, W, Hh):
        assert int(p.max_radius) == 8
        kw = dict(focus=p.focus, scale=p.scale, R=8, bg=int(p.background_radius), rng=p.range)
        wants.append(TD.rule(f["z"], f["fb"], **kw))
        differ(T.depth_of_field_host(f["z"], f["fb"], p), wants[-1], kw)
    changed("dof", W, Hh, wants, f["fb"])
    if (W, Hh) in EC.DEPTH_CHANGES:
        coc = T.dof_coc(EC.dof_sets(f, W, Hh)[0], f["z"])[f["drawn"]]
        assert (coc == 0).any() and (coc == 8).any(), "the model holds a sharp pixel and one at the largest circle"


@sizes(EC.SIZES)
def test_warp(built, small_synthetic, W, Hh):
    import tiny_renderer_amd as T
    f = dense(small_synthetic, W, Hh)
    wants = []
    for name, g, w, h, edge, border in EC.warp_sets(W, Hh):
        want = WC.rule_np(f["fb"], g, w, h, WC.CLAMP if edge == "clamp" else WC.BORDER, border)
        got = T.warp_host(f["fb"], g, w, h, T.warp_params(edge, border, per_channel=np.asarray(g).ndim == 4))
        differ(got, want, (name, w, h, edge, border))
        if (w, h) == (W, Hh):
            wants.append(want)
            if name == "identity":
                assert np.array_equal(want, f["fb"])
    if not EC.is_long(W, Hh):
        assert EC.warp_sets(W, Hh)[0][2:4] == (W, Hh), "the first set is the in-place case"
        changed("warp", W, Hh, wants[:1], f["fb"])
    elif max(W, Hh) == 32768:
        assert np.abs(EC.warp_sets(W, Hh)[0][1]).max() == WC.NODE_MAX, "no node at the coordinate limit"


def test_warp_footprints_at_and_past_the_flag_scan():
    """k_warp scans the flags of a footprint of at most 1024 source tiles and looks the flag up texel by texel beyond.
    On 20 x 32768 (1 x 2048 tiles) the first workgroup of "whole" covers 1025 tiles and that of "whole-3" exactly 1024;
    no other frame of the suite has a footprint past the bound with a side above 8192 (32768 x 17 has 512 tiles in all).
    The counts are the kernel's arithmetic restated (EC.warp_footprints)."""
    g = EC.whole_grids(20, 32768)
    n = EC.warp_footprints(g["whole"], 20, 32768, 17, 33)
    assert n.shape == (3, 1) and n[0, 0] == 1025 > EC.WARP_FLAG_TILES, n
    n = EC.warp_footprints(g["whole-3"], 20, 32768, 17, 33)
    assert n[0, 0] == 1024 == EC.WARP_FLAG_TILES, n
    names = [c[0] for c in EC.warp_sets(20, 32768)]
    assert "whole" in names and "whole-3" in names
    assert {c[4] for c in EC.warp_sets(20, 32768) if c[0] == "whole"} == {"border", "clamp"}
    for W, Hh in ((32768, 17), (8200, 16)):
        for name, grid in EC.whole_grids(W, Hh).items():
            assert EC.warp_footprints(grid, W, Hh, 17, 33).max() <= ((W + 127) // 128) * ((Hh + 15) // 16) <= EC.WARP_FLAG_TILES
    # the arithmetic itself, on a footprint that can be counted by hand: nodes (0, 0) .. (300, 40) of a 640 x 480 frame
    # cover columns 0 .. 301 (three tile columns) and buffer rows 0 .. 41 (tile rows 27 .. 29 from the bottom)
    hand = np.zeros((2, 2, 2), np.int64)
    hand[:, 1, 0], hand[1, :, 1] = 300 * 256, 40 * 256
    assert EC.warp_footprints(hand, 640, 480, 16, 16)[0, 0] == 9


def test_warp_reaches_16384_source_pixels_and_no_further(built, small_synthetic):
    """The known answer: nodes end at 2^22 / 256 = 16384, so of a 32768-wide frame the columns past 16384 cannot be
    named.  A grid that asks for x = 4 X is clipped there by the builders: every output column from 4096 on shows source
    column 16384 under TR_WARP_CLAMP and under a border alike (16384 lies inside the frame)."""
    import tiny_renderer_amd as T
    W, Hh = 32768, 17
    f = dense(small_synthetic, W, Hh)
    g = EC.stretch_grid(W, Hh, 8192, Hh)
    assert g.max() == WC.NODE_MAX and (g[..., 0] == WC.NODE_MAX).any() and g.shape == WC.grid_shape(8192, Hh) + (2,)
    for edge, border in (("clamp", (0, 0, 0)), ("border", WC.PAPER)):
        want = WC.rule_np(f["fb"], g, 8192, Hh, WC.CLAMP if edge == "clamp" else WC.BORDER, border)
        differ(T.warp_host(f["fb"], g, 8192, Hh, T.warp_params(edge, border)), want, edge)
        assert np.array_equal(want[:, 4096:], np.repeat(f["fb"][:, 16384:16385], 4096, 1)), "source column 16384, and no further"
        assert np.array_equal(want[:, :4096], f["fb"][:, 0:16384:4])
    assert f["drawn"][:, 16385:].any(), "the model is drawn where the grid cannot reach"


@sizes(EC.SIZES)
def test_resize(built, small_synthetic, W, Hh):
    import tiny_renderer_amd as T
    f = dense(small_synthetic, W, Hh)
    outs = EC.resize_outputs(W, Hh)
    assert outs[0] == (RC.up8(W), RC.up8(Hh)) and (min(W, 8192), min(Hh, 8192)) in outs
    for w, h, filt in EC.resize_sets(W, Hh):
        want = EC.resize_np(f["fb"], w, h, filt)
        differ(T.resize_host(f["fb"], w, h, filt), want, (w, h, filt))
        if not EC.is_long(W, Hh):
            differ(want, RC.resize_np(f["fb"], w, h, filt), ("tap by tap against the matrix products", w, h, filt))
        if filt == "area" and (w, h) == (W, Hh):
            assert np.array_equal(want, f["fb"]), "the same size is a copy"
    if (W, Hh) == (32768, 17):
        first, count, _ = RC.tables_np(RC.AREA, W, 4096)
        assert int(first.max()) + int(count.max()) == 32768 and first.max() > 32767 - 16, "`first` in the upper half of its 16 bits"


@sizes(tuple(s for s in EC.SIZES if EC.yuv_ok(*s)))
def test_yuv(built, small_synthetic, W, Hh):
    import tiny_renderer_amd as T
    f = dense(small_synthetic, W, Hh)
    for layout, m, r in EC.yuv_sets(W, Hh):
        got = T.yuv_host(f["fb"], layout, m, r, flat=True)
        assert np.array_equal(got, YC.flat_np(f["fb"], layout, m, r)), (layout, m, r)
    assert [s for s in EC.SIZES if not EC.yuv_ok(*s)] == list(EC.LONG), "every long frame is past the planes' 8192"


@sizes()
def test_statistics_and_the_box_of_resolve(built, small_synthetic, W, Hh):
    import tiny_renderer_amd as T
    from tests import test_frame_stats_host as TS
    from tests.test_outline import box
    f = dense(small_synthetic, W, Hh)
    zkw = EC.z_range(f)
    for window in (None, EC.window(W, Hh)):
        TS.same(T.frame_stats_host(f["fb"], f["z"], window=window, **zkw), TS.rule(f["fb"], f["z"], window, **zkw), "depth")
        TS.same(T.frame_stats_host(f["fb"], window=window), TS.rule(f["fb"], None, window), "colour")
    st = T.frame_stats_host(f["fb"], f["z"], **zkw)
    assert st.n_pixels == W * Hh and st.n_drawn == int(f["drawn"].sum())
    # resolve has no host entry point: its rule is `box`, pinned here to the rounded mean in exact float64 arithmetic
    for k in EC.resolve_factors(W, Hh):
        mean = f["fb"].reshape(Hh // k, k, W // k, k, 3).astype(np.float64).sum((1, 3)) / (k * k)
        differ(box(f["fb"], k), np.floor(mean + 0.5).astype(np.uint8), k)
    if (W, Hh) == EC.RESOLVE_LONG:
        assert EC.resolve_factors(W, Hh) == [2, 4, 8]


# ----------------------------------------------------------------------------------------------------------------------
# two scenes: the cases of the GPU file are not vacuous
# ----------------------------------------------------------------------------------------------------------------------

def oracle_pair(ms, other, W, Hh, pipe):
    """The oracle's frames of dst and src of the two-scene cases."""
    import tiny_renderer_amd as T
    from tests import test_shadow_merge as TM
    dst_at, src_at = EC.pair_tables(W, Hh)
    return (TM.oracle_frame(W, Hh, T.apply_instances(ms[0], dst_at), ms[1], pipe, EC.CAM, EC.LIGHT),
            TM.oracle_frame(W, Hh, T.apply_instances(other[0], src_at), other[1], pipe, EC.CAM, EC.LIGHT))


@sizes(EC.PAIR_SIZES)
def test_two_scenes_meet(built, small_synthetic, W, Hh):
    """composite: src wins pixels and loses pixels it covers; shadow_merge: the merged shadow buffer is not dst's."""
    import tiny_renderer_amd as T
    from tests import test_composite as TC
    from tests import test_shadow_merge as TM
    other = T.synthetic_scene(n_lat=9, n_lon=17, tex_size=128, radius=0.75)
    fd, fs = oracle_pair(small_synthetic, other, W, Hh, "phong")
    got, wins = TC.merge(fd, fs, 1000)
    assert wins.any() and ((bits(fs["z"]) != F32_MIN_BITS) & ~wins).any(), "src wins everything it covers, or nothing"
    z, c, w = T.composite_host(fd["z"], fd["fb"][::-1], fs["z"], fs["fb"][::-1], fd["win"], fs["win"], 1000)
    assert np.array_equal(bits(z), bits(got["z"])) and np.array_equal(c[::-1], got["fb"]) and np.array_equal(w, got["win"])
    fd, fs = oracle_pair(small_synthetic, other, W, Hh, "shadow")
    want = TM.rule(fd["shadow"], fs["shadow"])
    assert not np.array_equal(bits(want), bits(fd["shadow"]))
    assert np.array_equal(bits(want), bits(T.shadow_merge_host(fd["shadow"], fs["shadow"])))
