"""The frame stages and the render chain at the two ends of the frame sizes, on the device: frames below one 128 x 16
tile, down to one pixel, where every halo clamp, every store form and every list takes its edge form at once, and frames
with a side of 32768 (and 8200, the first past the stages' own 8192), where the 16-bit fields, the tile counts and the
footprint scans are at their ends.

The frames are tests/extreme_cases.py's: noise in a caller's guarded buffer, drawn into without a clear
(tests/test_dense_frames.py's dense_scene).  The expectation is the host rule over the scene's own snapshot;
tests/test_frame_extremes_host.py pins the host rules against numpy on the same frames and shows what each size reaches.
On the long frames one parameter set a stage runs.  Every comparison is np.array_equal."""
import ctypes as C

import numpy as np
import pytest

from tests import convolve_cases as CC
from tests import extreme_cases as EC
from tests import resize_cases as RC
from tests import test_composite as TC
from tests import test_dense_frames as TD
from tests import test_outline as TO
from tests import warp_cases as WC

bits, clean_flags, tiles_any = TC.bits, TC.clean_flags, TC.tiles_any
guarded, in_buffer, G = TD.guarded, TD.in_buffer, TD.G
other_synthetic = TC.other_synthetic
F32_MIN_BITS = EC.F32_MIN_BITS
ALL_SIZES = EC.SIZES + (EC.RESOLVE_LONG,)


def extreme_scene(ms, W, Hh):
    return TD.dense_scene(EC.model(ms, W, Hh), W, Hh, EC.KIND, table=EC.table, draws=EC.draws(W, Hh))


def refill(dev):
    """0x5A again, and the fill has finished before the scene's stream writes (torch fills on a stream of its own)."""
    import torch
    dev[:] = 0x5A
    torch.cuda.synchronize()


def flat(planes):
    return np.concatenate([p.reshape(-1) for p in planes])


def sets(stage, s, f):
    """TD.sets, and the same for the stages it does not know: [(label, want, call(out), get())]."""
    import tiny_renderer_amd as T
    W, Hh = s.width, s.height
    if stage in ("aa", "bloom", "dof", "outline", "grade", "ao", "resolve"):
        return TD.sets(stage, s, f, params=EC.td_params(stage, f, W, Hh), changes=EC.must_change(stage, W, Hh))
    out = []
    if stage == "convolve":
        ALL = CC.everything()
        for name, edge, border in EC.convolve_sets(W, Hh):
            p = CC.params(ALL[name], edge, border)
            out.append(((name, edge, border), T.convolve_host(f["fb"], p), lambda o, p=p: s.convolve(p, out=o), lambda p=p: s.get_convolved(p)))
    elif stage == "warp":
        for name, g, w, h, edge, border in EC.warp_sets(W, Hh):
            p = T.warp_params(edge, border, per_channel=np.asarray(g).ndim == 4)
            out.append(((name, w, h, edge, border), T.warp_host(f["fb"], g, w, h, p), lambda o, p=p, g=g, w=w, h=h: (s.set_warp(g, w, h), s.warp(p, out=o)),
                        lambda p=p, g=g, w=w, h=h: (s.set_warp(g, w, h), s.get_warped(p))[1]))
    elif stage == "resize":
        for w, h, filt in EC.resize_sets(W, Hh):
            out.append(((w, h, filt), T.resize_host(f["fb"], w, h, filt), lambda o, w=w, h=h, filt=filt: s.resize_into(o, w, h, filt),
                        lambda w=w, h=h, filt=filt: s.resize(w, h, filt)))
    elif stage == "yuv":
        for q in EC.yuv_sets(W, Hh):
            out.append((q, T.yuv_host(f["fb"], *q, flat=True), lambda o, q=q: s.to_yuv_into(o, *q), lambda q=q: flat(s.to_yuv(*q))))
    assert out
    own = [want for _, want, _, _ in out if want.shape == f["fb"].shape]      # (a long frame has no warp of its own size)
    if stage in ("convolve", "warp") and own and EC.must_change(stage, W, Hh):
        assert any(not np.array_equal(want, f["fb"]) for want in own), "every expectation is the input"
    return out


def sizes_of(stage):
    if stage == "resolve":
        return tuple(s for s in ALL_SIZES if EC.resolve_factors(*s))
    if stage == "yuv":
        return tuple(s for s in EC.SIZES if EC.yuv_ok(*s))
    return EC.SIZES


def cases(stages, sizes=sizes_of):
    rows = [(st, W, Hh) for st in stages for W, Hh in sizes(st)]
    return pytest.mark.parametrize("stage,W,Hh", rows, ids=["%s-%dx%d" % r for r in rows])


def test_every_size_has_every_stage():
    """Every listed size appears for every stage that accepts it; the others are the refusals of
    test_the_stages_own_limits: YUV past 8192 and the in-place warp past 8192."""
    assert set(sizes_of("yuv")) == set(EC.SMALL) and set(in_place_sizes("warp")) == set(EC.SMALL)
    assert {s for s in ALL_SIZES if s not in sizes_of("resolve")} == {s for s in EC.SIZES if s[0] % 2 or s[1] % 2}
    assert EC.RESOLVE_LONG in sizes_of("resolve") and EC.resolve_factors(*EC.RESOLVE_LONG) == [2, 4, 8]
    for st in ("aa", "outline", "dof", "bloom", "grade", "convolve", "warp", "resize", "ao"):
        assert sizes_of(st) == EC.SIZES


# ----------------------------------------------------------------------------------------------------------------------
# 1. the render chain at the long sizes
# ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("pipe", ["phong", "shadow"])
@pytest.mark.parametrize("W,Hh", EC.LONG, ids=["%dx%d" % s for s in EC.LONG])
def test_render_parity_at_the_long_sizes(small_synthetic, W, Hh, pipe):
    """Colour, z, winner words (and the shadow buffer) of `render` equal the oracle's, and so does every kept frame of a
    render_frames call whose last group is partial."""
    import tiny_renderer_amd as T
    from tests import test_gpu_parity as TP
    from tests import test_resolve as TR
    mesh, texs = T.apply_instances(small_synthetic[0], EC.table(W, Hh)), small_synthetic[1]
    gpu, cpu = TP.render_pair(W, Hh, mesh, texs, pipe, EC.CAM, EC.parity_light(W, Hh, pipe))
    TP.assert_parity(gpu, cpu, pipe)
    drawn = cpu.winner_u32() != 0xFFFFFFFF
    assert drawn.sum() > 10000
    gpu.close()
    grp = T.Scene(W, Hh, mesh, texs, pipe, frames_per_launch=4)
    p = TR._params(6)                                     # a group of four and a partial one of two
    grp.render_frames(p)
    kept = grp.frames_kept()
    assert kept >= 2
    for back in range(kept):
        q = p[len(p) - 1 - back]
        cpu.clear(), cpu.set_light_direction(q[0:3]), cpu.set_camera(q[3:6], q[6:9], q[9:12])
        assert cpu.render() == 0
        grp.select_frame(back)
        assert np.array_equal(bits(grp.read_z_f32()), bits(cpu.z_f32())), "frame -%d: z" % back
        assert np.array_equal(grp.get_frame_buffer(), cpu.get_frame_buffer()), "frame -%d: colour" % back
    grp.close(), cpu.close()


@pytest.mark.gpu
@pytest.mark.parametrize("W,Hh", ALL_SIZES, ids=["%dx%d" % s for s in ALL_SIZES])
def test_the_snapshot_is_the_frame_the_cpu_test_builds(small_synthetic, W, Hh):
    from tests import test_frame_extremes_host as TH
    s, buf, f = extreme_scene(small_synthetic, W, Hh)
    want = TH.dense(small_synthetic, W, Hh)
    assert np.array_equal(f["fb"], want["fb"]) and np.array_equal(bits(f["z"]), bits(want["z"]))
    s.close()


# ----------------------------------------------------------------------------------------------------------------------
# 2. every stage out of place and through its getter
# ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@cases(("aa", "outline", "dof", "bloom", "grade", "convolve", "warp", "resolve", "resize", "yuv"))
def test_out_of_place(small_synthetic, stage, W, Hh):
    """Every parameter set of the stage into device memory filled with 0x5A and through the getter: the host rule in
    every byte, nothing behind the result written, and the caller's frame, its guards and z as they were."""
    s, buf, f = extreme_scene(small_synthetic, W, Hh)
    zb = bits(f["z"])
    todo = sets(stage, s, f)
    dev = TO.device_buffer(max(want.size for _, want, _, _ in todo) + 64)
    for label, want, call, get in todo:
        refill(dev)
        call(dev.data_ptr())
        assert s.sync() == 0
        raw = dev.cpu().numpy()
        got = raw[:want.size].reshape(want.shape)
        assert np.array_equal(got, want), "%r: %d bytes differ" % (label, int((got != want).sum()))
        assert (raw[want.size:] == 0x5A).all(), "%r: bytes behind the result were written" % (label,)
        got = get()
        assert got.shape == want.shape and np.array_equal(got, want), "getter %r: %d bytes differ" % (label, int((got != want).sum()))
        in_buffer(buf, f["fb"])
        assert np.array_equal(bits(s.read_z_f32()), zb), "z changed"
    assert np.array_equal(s.get_frame_buffer(), f["fb"])
    s.close()


@pytest.mark.gpu
@cases(("ao",))
def test_ambient_occlusion_every_set(small_synthetic, stage, W, Hh):
    """Ambient occlusion has the in-place form alone: every parameter set on a fresh frame."""
    for k in range(len(EC.ao_sets(W, Hh))):
        s, buf, f = extreme_scene(small_synthetic, W, Hh)
        label, want, call, _ = sets("ao", s, f)[k]
        call(None)
        assert s.sync() == 0
        in_buffer(buf, want)
        assert np.array_equal(bits(s.read_z_f32()), bits(f["z"])), "z changed"
        s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("W,Hh", ALL_SIZES, ids=["%dx%d" % s for s in ALL_SIZES])
def test_statistics(small_synthetic, W, Hh):
    import tiny_renderer_amd as T
    s, buf, f = extreme_scene(small_synthetic, W, Hh)
    zkw = EC.z_range(f)
    for window in (None, EC.window(W, Hh)):
        want = T.frame_stats_host(f["fb"], f["z"], window=window, depth=True, **zkw)
        assert (want.n_drawn > 0) == EC.draws(W, Hh) or window is not None
        got = s.get_frame_stats(window=window, depth=True, **zkw)
        assert got == want, "%r != %r" % (got, want)
        assert s.get_frame_stats(window=window) == T.frame_stats_host(f["fb"], window=window)
    assert T.frame_stats_host(f["fb"]).n_pixels == W * Hh
    in_buffer(buf, f["fb"])
    assert np.array_equal(bits(s.read_z_f32()), bits(f["z"]))
    s.close()


# ----------------------------------------------------------------------------------------------------------------------
# 3. every stage in place
# ----------------------------------------------------------------------------------------------------------------------

def in_place_sizes(stage):
    """A grid is at most 8192 a side and the in-place warp wants the frame's size: the small frames alone."""
    return EC.SMALL if stage == "warp" else EC.SIZES


@pytest.mark.gpu
@cases(EC.IN_STAGES, in_place_sizes)
def test_in_place(small_synthetic, stage, W, Hh):
    """One parameter set of the stage in place in the caller's buffer: the host rule between guards that stay, the same
    through get_frame_buffer, no flag up over a tile that holds colour, z as it was."""
    s, buf, f = extreme_scene(small_synthetic, W, Hh)
    todo = sets(stage, s, f)
    label, want, call, _ = todo[EC.ONE[stage] if len(todo) > 1 else 0]
    assert want.shape == f["fb"].shape
    if EC.must_change(stage, W, Hh):
        assert not np.array_equal(want, f["fb"]), label
    call(None)
    assert s.sync() == 0
    in_buffer(buf, want)
    assert np.array_equal(s.get_frame_buffer(), want)
    assert not (clean_flags(s) & tiles_any(want[::-1].any(-1))).any(), "a tile with colour in it is flagged clean"
    assert np.array_equal(bits(s.read_z_f32()), bits(f["z"])), "z changed"
    in_buffer(buf, want)
    s.close()


# ----------------------------------------------------------------------------------------------------------------------
# 4. two scenes, and kept frames
# ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("W,Hh", EC.PAIR_SIZES, ids=["%dx%d" % s for s in EC.PAIR_SIZES])
def test_composite(small_synthetic, other_synthetic, W, Hh):
    import tiny_renderer_amd as T
    dst_at, src_at = EC.pair_tables(W, Hh)
    want = None
    for twin in (True, False):
        d = TC.scene(W, Hh, small_synthetic, "phong", dst_at, tap=True)
        s = TC.scene(W, Hh, other_synthetic, "phong", src_at, tap=True)
        TC.drive(d, EC.CAM, EC.LIGHT), TC.drive(s, EC.CAM, EC.LIGHT)
        if twin:
            fd, fs = TC.snap(d), TC.snap(s)
            want, wins = TC.merge(fd, fs, 1000)
            assert wins.any() and ((bits(fs["z"]) != F32_MIN_BITS) & ~wins).any(), "the case is vacuous"
            z, c, w = T.composite_host(fd["z"], fd["fb"][::-1], fs["z"], fs["fb"][::-1], fd["win"], fs["win"], 1000)
            assert np.array_equal(bits(z), bits(want["z"])) and np.array_equal(c[::-1], want["fb"]) and np.array_equal(w, want["win"])
        else:
            d.composite(s, winner_base=1000)
            assert d.sync() == 0
            TC.same(TC.snap(d), want)
            TC.same(TC.snap(s), fs)
        d.close(), s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("W,Hh", EC.PAIR_SIZES, ids=["%dx%d" % s for s in EC.PAIR_SIZES])
def test_shadow_merge(small_synthetic, other_synthetic, W, Hh):
    import tiny_renderer_amd as T
    from tests import test_shadow_merge as TM
    dst_at, src_at = EC.pair_tables(W, Hh)
    want = None
    for twin in (True, False):
        d = TM.scene(W, Hh, small_synthetic, "shadow", dst_at, tap=True)
        s = TM.scene(W, Hh, other_synthetic, "shadow", src_at, tap=True)
        TM.drive(d, EC.CAM, EC.LIGHT), TM.drive(s, EC.CAM, EC.LIGHT)
        if twin:
            fd, fs = TM.snap(d), TM.snap(s)
            want = dict(fd, shadow=T.shadow_merge_host(fd["shadow"], fs["shadow"]))
            assert not np.array_equal(bits(want["shadow"]), bits(fd["shadow"])), "the case is vacuous"
            assert np.array_equal(bits(want["shadow"]), bits(TM.rule(fd["shadow"], fs["shadow"])))
        else:
            d.shadow_merge(s)
            assert d.sync() == 0
            TM.same(TM.snap(d), want, what="dst:")
            TM.same(TM.snap(s), fs, what="src:")
        d.close(), s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("W,Hh", EC.ACCUMULATE_SIZES, ids=["%dx%d" % s for s in EC.ACCUMULATE_SIZES])
def test_accumulate_three_kept_frames(small_synthetic, W, Hh):
    import tiny_renderer_amd as T
    from tests import test_accumulate as TA
    from tests import test_resolve as TR
    mesh, texs = T.apply_instances(small_synthetic[0], EC.table(W, Hh)), small_synthetic[1]
    s = T.Scene(W, Hh, mesh, texs, "phong", frames_per_launch=3)
    s.render_frames(TR._params(3))
    assert s.frames_kept() == 3
    nb = W * Hh * 3
    for w in (None, [2, 0, 5]):
        dev = TO.device_buffer(nb + 32, 0xAB)
        s.accumulate_into(3, dev.data_ptr() + 16, w)
        assert s.sync() == 0
        host = s.accumulate(3, w)
        frames = TA.kept(s, 3)
        want = T.accumulate_host(frames, w)
        assert np.array_equal(want, TA.oracle(frames, w)) and want.any()
        assert not np.array_equal(frames[0], frames[1]) and not np.array_equal(frames[1], frames[2])
        raw = dev.cpu().numpy()
        assert (raw[:16] == 0xAB).all() and (raw[16 + nb:] == 0xAB).all()
        assert np.array_equal(raw[16:16 + nb].reshape(Hh, W, 3), want), w
        assert np.array_equal(host, want), w
    s.accumulate_in_place(3, [1, 2, 3])
    assert np.array_equal(s.get_frame_buffer(), T.accumulate_host(frames, [1, 2, 3]))
    s.close()


# ----------------------------------------------------------------------------------------------------------------------
# 5. the stages' own limits
# ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("W,Hh", EC.LONG, ids=["%dx%d" % s for s in EC.LONG])
def test_the_stages_own_limits(small_synthetic, W, Hh):
    """A warp grid or a resize output above 8192, an in-place warp, to_yuv and a resize below ceil(N / 8) are refused with
    their documented texts and leave the scene as it was; an out-of-place warp through a grid of at most 8192 a side whose
    nodes run to the coordinate limit equals the host rule, and source pixels past 16384 cannot be reached."""
    import tiny_renderer_amd as T
    from tiny_renderer_amd import _lib
    L = T.load_library()
    text = lambda: L.tr_last_error().decode()
    s, buf, f = extreme_scene(small_synthetic, W, Hh)
    flags = clean_flags(s)
    w, h = EC.cap(W), EC.cap(Hh)
    dev = TO.device_buffer(w * h * 3 + 64)
    host_out = np.full(64, 0xAA, np.uint8)
    wp, yp = T.warp_params(), T.yuv_params()
    assert L.tr_scene_warp(s._h, C.addressof(wp), None) == _lib.TR_E_INVALID and text() == "tr_scene_warp: the scene has no grid (tr_scene_set_warp)"
    g = np.ascontiguousarray(EC.stretch_grid(W, Hh, w, h))
    too_wide = (W, h) if W > EC.STAGE_MAX else (w, Hh)
    assert max(too_wide) > EC.STAGE_MAX
    for size in (too_wide, (EC.STAGE_MAX + 1, 1), (1, EC.STAGE_MAX + 1)):
        assert L.tr_scene_set_warp(s._h, size[0], size[1], 1, g.ctypes.data) == _lib.TR_E_INVALID
        assert text() == "tr_scene_set_warp: width and height must be 1..8192"
    with pytest.raises((ValueError, T.TinyRendererError)):
        s.set_warp(g, *too_wide)
    s.set_warp(g, w, h)
    assert L.tr_scene_warp(s._h, C.addressof(wp), None) == _lib.TR_E_INVALID
    assert text() == "tr_scene_warp: out == NULL warps in place, and the grid's size is not the frame's"
    for who, call in (("tr_scene_to_yuv", lambda: L.tr_scene_to_yuv(s._h, C.addressof(yp), dev.data_ptr())),
                      ("tr_scene_get_yuv", lambda: L.tr_scene_get_yuv(s._h, C.addressof(yp), host_out.ctypes.data))):
        assert call() == _lib.TR_E_INVALID and text() == who + ": width and height must be 1..8192"
    shrinks = ": a side shrinks by more than 8 (width and height must be at least an eighth of the source's, rounded up)"
    small = (RC.up8(W) - 1, h) if W >= Hh else (w, RC.up8(Hh) - 1)
    for fields, why in (((EC.STAGE_MAX + 1, h, 0, 0), ": width and height must be 1..8192"), ((w, EC.STAGE_MAX + 1, 1, 0), ": width and height must be 1..8192"),
                        (small + (0, 0), shrinks), (small + (1, 0), shrinks)):
        bad = T.ResizeParams(*fields)
        assert L.tr_scene_resize(s._h, C.addressof(bad), dev.data_ptr()) == _lib.TR_E_INVALID and text() == "tr_scene_resize" + why
        assert L.tr_scene_get_resized(s._h, C.addressof(bad), host_out.ctypes.data) == _lib.TR_E_INVALID and text() == "tr_scene_get_resized" + why
    with pytest.raises(ValueError):
        s.resize(*small)
    assert s.sync() == 0
    assert (host_out == 0xAA).all() and (dev.cpu().numpy() == 0x5A).all(), "a refused call wrote `out`"
    assert np.array_equal(clean_flags(s), flags)
    in_buffer(buf, f["fb"])
    assert np.array_equal(bits(s.read_z_f32()), bits(f["z"]))
    # the warp that is allowed: nodes to the limit, under the clamp and under a border that is not black
    assert g.max() == WC.NODE_MAX
    for edge, border in (("clamp", (0, 0, 0)), ("border", WC.PAPER)):
        p = T.warp_params(edge, border)
        want = T.warp_host(f["fb"], g, w, h, p)
        refill(dev)
        s.warp(p, out=dev.data_ptr())
        assert s.sync() == 0
        raw = dev.cpu().numpy()
        got = raw[:want.size].reshape(want.shape)
        assert np.array_equal(got, want), "%s: %d bytes differ" % (edge, int((got != want).sum()))
        assert (raw[want.size:] == 0x5A).all()
        assert np.array_equal(s.get_warped(p), want)
        if W == 32768:
            assert np.array_equal(got[:, 4096:], np.repeat(f["fb"][:, 16384:16385], 4096, 1)), "source column 16384, and no further"
        elif Hh == 32768:
            assert np.array_equal(got[4096:], np.repeat(f["fb"][16384:16385], 4096, 0)), "source row 16384, and no further"
        elif edge == "border":
            assert (got[:, 2051:] == np.array(WC.PAPER, np.uint8)).all(), "past the frame's last column: the border"
    in_buffer(buf, f["fb"])
    s.close()


@pytest.mark.gpu
def test_warp_footprint_past_the_flag_scan_over_flagged_tiles(small_synthetic):
    """20 x 32768 rendered on a CLEARED frame: tiles with their flag up lie under the footprints of 1025 tiles (looked up
    texel by texel, tile rows up to 2047) and of 1024 (scanned); tests/test_frame_extremes_host.py asserts the counts."""
    import tiny_renderer_amd as T
    W, Hh = 20, 32768
    s = TC.scene(W, Hh, small_synthetic, EC.PIPE, EC.table(W, Hh))
    TC.drive(s, EC.CAM, EC.LIGHT)
    fb = s.get_frame_buffer()
    TC.drive(s, EC.CAM, EC.LIGHT)                          # (a fresh frame: flags as a render leaves them)
    flags = clean_flags(s)
    assert flags.shape == (2048, 1) and flags[1023:].any() and not flags[1023:].all(), "flagged and unflagged tiles under the footprint (buffer rows 0 .. 16385: tile rows 1023 .. 2047 from the bottom)"
    assert fb.any()
    for name, g in EC.whole_grids(W, Hh).items():
        s.set_warp(g, 17, 33)
        for edge, border in (("clamp", (0, 0, 0)), ("border", WC.PAPER), ("border", (0, 0, 0))):
            p = T.warp_params(edge, border)
            want = T.warp_host(fb, g, 17, 33, p)
            got = s.get_warped(p)
            assert np.array_equal(got, want), "%s %s: %d bytes differ" % (name, edge, int((got != want).sum()))
    assert np.array_equal(clean_flags(s), flags) and np.array_equal(s.get_frame_buffer(), fb)
    s.close()


@pytest.mark.gpu
def test_the_device_reports_the_shadow_lookup_the_reference_panics_on(small_synthetic):
    """20 x 32768, shadow pipeline, the suite's light: the oracle reports TRO_E_SHADOW_OOB (asserted on the CPU), so the
    library must report TR_E_OOB_LOOKUP from sync; a defined frame rendered afterwards is the oracle's."""
    import tiny_renderer_amd as T
    from tiny_renderer_amd import _lib
    from tests import test_gpu_parity as TP
    W, Hh = 20, 32768
    assert EC.parity_light(W, Hh, "shadow") != EC.LIGHT
    mesh, texs = T.apply_instances(small_synthetic[0], EC.table(W, Hh)), small_synthetic[1]
    gpu = T.Scene(W, Hh, mesh, texs, "shadow")
    with pytest.raises(T.TinyRendererError) as e:
        TC.drive(gpu, EC.CAM, EC.LIGHT)
        gpu.sync()
        gpu.get_frame_buffer()
    assert e.value.code == _lib.TR_E_OOB_LOOKUP, e.value
    gpu.close()
    gpu, cpu = TP.render_pair(W, Hh, mesh, texs, "shadow", EC.CAM, EC.parity_light(W, Hh, "shadow"))
    TP.assert_parity(gpu, cpu, "shadow")
    gpu.close(), cpu.close()


# ----------------------------------------------------------------------------------------------------------------------
# 6. odd addresses on frames whose width is a multiple of 4
# ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("W,Hh", [(8, 8), (4, 16)], ids=["8x8", "4x16"])
@pytest.mark.parametrize("stage", TD.ODD)
def test_out_at_an_odd_address(small_synthetic, stage, W, Hh):
    """The wide store forms need an aligned `out`: one byte past a guard the stage takes the byte form and writes the
    same frame, and nothing around it."""
    n = W * Hh * 3
    s, buf, f = extreme_scene(small_synthetic, W, Hh)
    label, want, call, _ = sets(stage, s, f)[EC.ONE[stage]]
    assert not np.array_equal(want, f["fb"])
    tgt = guarded(np.full(n, 0xAA, np.uint8), extra=8)
    for off in (0, 1):
        call(tgt.data_ptr() + G + off)
        assert s.sync() == 0
        raw = tgt.cpu().numpy()
        got = raw[G + off:G + off + n].reshape(Hh, W, 3)
        assert np.array_equal(got, want), "offset %d: %d bytes differ" % (off, int((got != want).sum()))
        assert (raw[:G] == 0xAA).all() and (raw[G + off + n:] == 0xAA).all(), "offset %d: a guard byte changed" % off
        in_buffer(buf, f["fb"])
    s.close()
