"""The consumers of a frame that was warped or convolved IN PLACE, on the device.

tr_scene_warp and tr_scene_convolve with out == NULL replace a frame's colour and its per-tile colour flags through the
scratch frame and leave z and the z flags alone, so afterwards the two flag sets disagree (tests/warp_consumer_cases.py:
state A, colour flag up over drawn depth; state B, colour in a tile nothing was drawn in).  Every kernel that reads both
sets runs behind such a frame here: k_ao, k_dof, k_outline, k_stats with depth, k_composite on either side, k_tile in a
render without a clear, ensure_depth's depth-only repeat (the consumer is the first to ask the scene for depth: the
profile shows exactly one more launch of the tile kernel where depth was transient and none where it was stored), and
the colour stages, the kept frames, a caller's buffer and the library's one read-back buffer.

Every comparison is np.array_equal (or whole-record equality) against a chain of the library's host rules: the stage's
rule over the colour of a TWIN scene's snapshot, then the consumer's rule over that colour and the twin's z -- the z of
before the stage, which the stage leaves alone.  A case that exists to reach a state asserts on the device's own flags
that it did; tests/test_warp_consumers_host.py shows on the CPU that the cases can.

Combinations left out, because they reach nothing the kept ones do not: rotate7 and emboss at 200 x 40 (at a height
that is no multiple of 16 an in-place warp lowers every flag, which `shift` shows there, and emboss lowers every flag at
any size); shift_paper at 200 x 40 (no flag is up after it at either size); unsharp with the depth and colour consumers
(it changes drawn pixels only and leaves every flag where the render put it: it runs under the render without a clear);
the colour consumers with stored depth (they read none).

"Flags stay up far away" after gaussian31 cannot happen at these sizes: k_convolve keeps a tile's flag only where the
tile and all its neighbours are flagged, and a drawn tile neighbours every tile of 3 x 3 and of 2 x 3.  What the code
does instead is asserted from the device's flags: none is up, and the spill lies in undrawn tiles (state B)."""
import numpy as np
import pytest

from tests import convolve_cases as CC
from tests import test_accumulate as TA
from tests import test_composite as TC
from tests import test_dense_frames as TDF
from tests import test_depth_of_field as TD
from tests import test_postprocess_chain as PC
from tests import test_stage_entry_points as TS
from tests import warp_cases as WC
from tests import warp_consumer_cases as K
from tests.test_composite import other_synthetic  # noqa: F401

bits, scene, snap, clean_flags, tiles_any = TC.bits, TC.scene, TC.snap, TC.clean_flags, TC.tiles_any
BOTH = PC.BOTH
CASES = [("shift", K.MIDDLE), ("rotate7", K.MIDDLE), ("shift_paper", K.MIDDLE), ("shift", K.NARROW), ("gaussian31", K.MIDDLE),
         ("emboss", K.MIDDLE), ("gaussian31", K.NARROW)]
CASE_IDS = ["%s-%dx%d" % (st, sz[0], sz[1]) for st, sz in CASES]
_REF = {}


def drive(s, cam=K.CAM, light=K.LIGHT, clear=True):
    TC.drive(s, cam, light, clear)


def model(ms, size, store_depth=False, **kw):
    return scene(size[0], size[1], ms, K.PIPE, K.PLACE[size], store_depth=store_depth, **kw)


def frozen(f):
    for a in f.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return f


def twin(ms, size):
    """The snapshot of a twin scene that no stage touches, taken once and left alone."""
    key = ("model", size)
    if key not in _REF:
        t = model(ms, size)
        drive(t)
        _REF[key] = frozen(snap(t))
        t.close()
    return _REF[key]


def twin_pair(ms, size):
    """A twin's snapshots after its first render and after a second one, from another camera, without a clear."""
    key = ("pair", size)
    if key not in _REF:
        t = model(ms, size)
        drive(t)
        first = frozen(snap(t))
        drive(t, cam=K.TOP_CAM[size], clear=False)
        _REF[key] = (first, frozen(snap(t)))
        t.close()
    return _REF[key]


def other_twin(other, size):
    key = ("other", size)
    if key not in _REF:
        t = scene(size[0], size[1], other, K.PIPE, K.OTHER_AT[size])
        drive(t, light=K.OTHER_LIGHT)
        _REF[key] = frozen(snap(t))
        t.close()
    return _REF[key]


def same(got, want, what):
    assert got.shape == want.shape and np.array_equal(got, want), "%s: %d bytes differ" % (what, int((got != want).sum()))


def launches(s, kernel="k_tile"):
    """The pass launches so far.  ensure_depth's depth-only repeat of a colour pass is timed under k_tile, like the pass
    itself (k_tile_depth is the shadow pipelines' depth pass): the observable of tests/test_frame_stats.py."""
    assert s.sync() == 0
    return s.profile_read().get(kernel, {}).get("launches", 0)


def reaches(stage, size, f, staged, flags):
    """The device's own flags after the stage say that the case reached what it is for; always: no lit tile is flagged."""
    assert not (flags & K.lit(staged)).any(), "a tile that holds colour is flagged clean"
    undrawn = ~tiles_any(K.drawn(f))
    if size[1] % 16:
        if K.STAGES[stage][0] == "warp":
            assert not flags.any(), "the frame's tiles are not k_warp's at this height: every flag goes down"
    elif stage == "shift":
        assert K.state_a(f, staged, flags).any(), "state A: no flag is up over a tile with drawn z"
        assert K.state_a(f, staged, flags)[:, 0].all(), "the left tile column moved out of the image whole"
    if stage in ("shift", "shift_paper", "emboss", "rotate7", "gaussian31"):
        assert K.state_b(f, staged, flags).any(), "state B: no undrawn tile holds colour under a lowered flag"
    if K.STAGES[stage][0] == "convolve":
        # k_convolve keeps a flag only where the tile and all its neighbours are flagged: the drawn centre tile of
        # 3 x 3, or the drawn middle row of 2 x 3, neighbours every tile
        assert not flags.any(), "a flag stayed up next to a tile that held colour"
    if stage in ("shift_paper", "emboss"):
        assert not flags.any() and np.array_equal(K.state_b(f, staged, flags), undrawn), "state B in every undrawn tile, no flag up"
    if stage in ("rotate7", "gaussian31"):
        assert (~K.drawn(f) & staged[::-1].any(-1)).sum() > 50, "no colour over undrawn z"
    if stage == "rotate7":
        assert (K.drawn(f) & ~staged[::-1].any(-1)).sum() > 50, "no drawn z left without colour"


def staged_scene(ms, size, store_depth):
    s = model(ms, size, store_depth)
    s.profile_enable(True)
    return s


def consume(s, ms, stage, size, store_depth, names):
    """Each consumer behind a fresh render and the stage in place: the frame (or the record), the flags, z, the profile."""
    f = twin(ms, size)
    staged = K.stage_host(stage, f["fb"])
    after = dict(f, fb=staged)
    for name in names:
        host, run = K.consumer(name, f)
        want = host(after)
        drive(s)
        K.stage_run(s, stage)
        reaches(stage, size, f, staged, clean_flags(s))
        n0 = launches(s)
        got = run(s)
        flags = clean_flags(s)
        if K.is_getter(name):
            if name == "yuv":
                assert len(got) == len(want) and all(np.array_equal(a, b) for a, b in zip(got, want)), name
            else:
                assert got == want, "%s: %r != %r" % (name, got, want)
            frame = staged
        else:
            frame = want
        same(s.get_frame_buffer(), frame, "%s after %s" % (name, stage))
        assert not (flags & K.lit(frame)).any(), name + ": a tile with colour in it is flagged clean"
        if name in K.DEPTH_CONSUMERS:
            # the consumer was the first to ask for depth: one depth-only repeat behind the replaced colour, or none
            assert launches(s) - n0 == (0 if store_depth else 1), "%s: %d depth-only passes" % (name, launches(s) - n0)
        assert np.array_equal(bits(s.read_z_f32()), bits(f["z"])), name + ": z changed"
        same(s.get_frame_buffer(), frame, "%s after %s, after z was read" % (name, stage))
        if name in K.DEPTH_CONSUMERS:
            assert launches(s) - n0 == (0 if store_depth else 1), name + ": reading z repeated the pass again"


# ----------------------------------------------------------------------------------------------------------------------
# 1. depth consumers, 2. colour consumers
# ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@BOTH
@pytest.mark.parametrize("stage,size", CASES, ids=CASE_IDS)
def test_depth_consumers(small_synthetic, stage, size, store_depth):
    """k_ao plain and grey, k_dof with a background radius of 0 and 2, k_outline plain and ONLY over a paper that is not
    black, k_stats with depth."""
    s = staged_scene(small_synthetic, size, store_depth)
    consume(s, small_synthetic, stage, size, store_depth, K.DEPTH_CONSUMERS)
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("stage,size", CASES, ids=CASE_IDS)
def test_colour_consumers(small_synthetic, stage, size):
    """bloom, grade with a black and with a tinted entry 0, antialias, the colour statistics and to_yuv; z is read last,
    so ensure_depth repeats the pass behind two stages in place."""
    s = staged_scene(small_synthetic, size, False)
    consume(s, small_synthetic, stage, size, False, K.COLOUR_CONSUMERS)
    s.close()


# ----------------------------------------------------------------------------------------------------------------------
# 3. both orders
# ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@BOTH
@pytest.mark.parametrize("size", [K.MIDDLE, K.NARROW], ids=["384x48", "200x40"])
def test_warp_and_convolve_and_depth_of_field_in_either_order(small_synthetic, size, store_depth):
    import tiny_renderer_amd as T
    f = twin(small_synthetic, size)
    s = model(small_synthetic, size, store_depth)
    for warp, conv in K.ORDER_PAIRS:
        want = (K.stage_host(conv, K.stage_host(warp, f["fb"])), K.stage_host(warp, K.stage_host(conv, f["fb"])))
        assert not np.array_equal(want[0], want[1]), "the two orders give one frame"
        for order, names in enumerate(((warp, conv), (conv, warp))):
            drive(s)
            K.stage_run(s, names[0]), K.stage_run(s, names[1])
            flags = clean_flags(s)
            same(s.get_frame_buffer(), want[order], "%s then %s" % names)
            assert not (flags & K.lit(want[order])).any(), "a tile with colour in it is flagged clean"
            assert np.array_equal(bits(s.read_z_f32()), bits(f["z"]))
    p = TD.params_for(f, 3, bg=2)
    for warp in ("shift", "rotate7"):
        want = (T.depth_of_field_host(f["z"], K.stage_host(warp, f["fb"]), p), K.stage_host(warp, T.depth_of_field_host(f["z"], f["fb"], p)))
        assert not np.array_equal(want[0], want[1]), "the two orders give one frame"
        for order in (0, 1):
            drive(s)
            if order == 0:
                K.stage_run(s, warp), s.depth_of_field(p)
            else:
                s.depth_of_field(p), K.stage_run(s, warp)
            flags = clean_flags(s)
            same(s.get_frame_buffer(), want[order], "%s and depth of field, order %d" % (warp, order))
            assert not (flags & K.lit(want[order])).any(), "a tile with colour in it is flagged clean"
            assert np.array_equal(bits(s.read_z_f32()), bits(f["z"]))
    s.close()


# ----------------------------------------------------------------------------------------------------------------------
# 4. composite
# ----------------------------------------------------------------------------------------------------------------------

def after_a_merge(d, want):
    """resolve(2), the sparse read-back, the statistics with depth, then every byte of the merged frame."""
    import tiny_renderer_amd as T
    same(d.resolve(2), TD.box(want["fb"], 2), "resolve(2) of the merge")
    P = d.pinned_frame()
    P[...] = 0xAA
    d.get_frame_buffer_async(P)
    assert d.sync() == 0
    same(P, want["fb"], "the sparse read-back of the merge")
    zkw = K.zrange(want)
    got, rec = d.get_frame_stats(depth=True, **zkw), T.frame_stats_host(want["fb"], want["z"], depth=True, **zkw)
    assert got == rec, "%r != %r" % (got, rec)
    TC.same(snap(d), want)


@pytest.mark.gpu
@BOTH
@pytest.mark.parametrize("role", ["dst", "src"])
@pytest.mark.parametrize("size", [K.MIDDLE, K.NARROW], ids=["384x48", "200x40"])
def test_composite_with_a_warped_scene(small_synthetic, other_synthetic, size, role, store_depth):
    """dst: a state-A tile takes src's fragments where src wins and keeps zeros elsewhere.  src: a state-A tile gives its
    zero colour together with its depth, which is what the rule says."""
    W, Hh = size
    f, fo = twin(small_synthetic, size), other_twin(other_synthetic, size)
    staged = K.stage_host("shift", f["fb"])
    warped = dict(f, fb=staged, win=None)
    w = model(small_synthetic, size, store_depth)
    o = scene(W, Hh, other_synthetic, K.PIPE, K.OTHER_AT[size], store_depth=store_depth)
    drive(w), drive(o, light=K.OTHER_LIGHT)
    K.stage_run(w, "shift")
    flags = clean_flags(w)
    reaches("shift", size, f, staged, flags)
    a = K.tile_pixels(K.state_a(f, staged, flags), Hh, W)
    if role == "dst":
        want, wins = TC.merge(warped, fo)
        assert wins.any() and (K.drawn(fo) & ~wins).any()
        w.composite(o)
        after_flags = clean_flags(w)
        assert not (after_flags & (tiles_any(wins) | K.lit(want["fb"]))).any(), "a flag is up over a tile src won a pixel of"
        after_a_merge(w, want)
        if size == K.MIDDLE:
            got = w.get_frame_buffer()[::-1]
            assert (a & wins).any() and (a & ~wins).any()
            assert np.array_equal(got[a & wins], fo["fb"][::-1][a & wins]) and not got[a & ~wins].any()
        TC.same(snap(o), fo)
    else:
        want, wins = TC.merge(fo, warped)
        assert wins.any() and (K.drawn(f) & ~wins).any()
        o.composite(w)
        after_a_merge(o, want)
        if size == K.MIDDLE:
            assert (a & wins).any() and fo["fb"][::-1][a & wins].any()
            assert not o.get_frame_buffer()[::-1][a & wins].any(), "zero colour travels with the depth"
            assert np.array_equal(bits(o.read_z_f32())[a & wins], bits(f["z"])[a & wins])
        assert np.array_equal(clean_flags(w), flags), "src's flags changed"
        TC.same(snap(w), warped)
    w.close(), o.close()


# ----------------------------------------------------------------------------------------------------------------------
# 5. a render without a clear on top
# ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@BOTH
@pytest.mark.parametrize("size", [K.MIDDLE, K.NARROW], ids=["384x48", "200x40"])
@pytest.mark.parametrize("stage", K.ON_TOP_STAGES)
def test_a_render_without_a_clear_on_top(small_synthetic, stage, size, store_depth):
    """k_tile takes zfresh from the z flag and colour from memory: a pixel the second render wins has the twin's colour,
    every other pixel the staged colour; z is the twin's.  With transient depth the accumulating render is the first to
    ask for depth."""
    W, Hh = size
    first, second = twin_pair(small_synthetic, size)
    staged = K.stage_host(stage, first["fb"])
    want, won = K.on_top(first, second, staged)
    assert won.any() and not np.array_equal(want, second["fb"]) and not np.array_equal(want, staged)
    s = model(small_synthetic, size, store_depth)
    drive(s)
    K.stage_run(s, stage)
    flags = clean_flags(s)
    if stage != "unsharp":
        reaches(stage, size, first, staged, flags)
    drive(s, cam=K.TOP_CAM[size], clear=False)
    after = clean_flags(s)
    got = snap(s)
    assert not (after & K.lit(want)).any(), "a tile with colour in it is flagged clean"
    TC.same(got, {"fb": want, "z": second["z"], "win": None})
    if stage == "shift" and size == K.MIDDLE:
        touched = K.state_a(first, staged, flags) & tiles_any(won)
        assert touched.any(), "the second render touches no state-A tile"
        assert not (after & touched).any(), "a state-A tile the render drew into is still flagged clean"
        rest = K.tile_pixels(touched, Hh, W) & ~won
        assert rest.any() and not got["fb"][::-1][rest].any(), "a state-A tile holds something where nothing won"
    s.close()


# ----------------------------------------------------------------------------------------------------------------------
# 6. kept and posed frames
# ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_a_kept_posed_frame_warped_then_blurred_then_the_average(small_synthetic):
    """Four frames by one launch with a pose each, transient depth; frame 2 is selected, another frame's pose made
    current, the frame warped in place and blurred: depth is the selected frame's pose behind the replaced colour.  The
    other kept frames stay, the average takes the changed frame, and the frame's slot still remembers its own pose."""
    import tiny_renderer_amd as T
    ms, kind, n, back = small_synthetic, K.POSED_KIND, PC.POSED_N, K.POSED_BACK
    par = PC.TCC.frame_params(n)
    ks = [0.5 * i for i in range(n)]
    frames = [PC.twin_frame(kind, ms, ks[i], par[i]) for i in range(n)]     # render order
    sel = frames[n - 1 - back]
    staged = K.stage_host(K.POSED_STAGE, sel["fb"])
    p = TD.params_for(sel, 3, bg=1)
    want = T.depth_of_field_host(sel["z"], staged, p)
    assert not np.array_equal(want, staged) and not np.array_equal(staged, sel["fb"])
    assert not np.array_equal(T.depth_of_field_host(frames[n - 1]["z"], staged, p), want), "another pose's depth would not show"
    s = PC.posed_scene(kind, ms, 0, frames_per_launch=n)
    s.profile_enable(True)
    key = {"skin": "bone_palettes", "morph": "morph_weights"}[kind]
    s.render_frames(par, **{key: np.stack([PC.pose(kind, k) for k in ks])})
    assert s.frames_kept() == n
    s.select_frame(back)
    PC.set_pose(s, kind, ks[back])              # (frame n - 1 - back is selected: pose `back` is another frame's)
    n0 = launches(s)
    K.stage_run(s, K.POSED_STAGE)
    assert launches(s) == n0, "the warp asked for depth"
    s.depth_of_field(p)
    flags = clean_flags(s)
    assert launches(s) - n0 >= 1, "the blur drew no depth"
    same(s.get_frame_buffer(), want, "the kept frame")
    assert not (flags & K.lit(want)).any(), "a tile with colour in it is flagged clean"
    TD.same_state(TD.state(s), {"z": bits(sel["z"]), "win": None, "shadow": None})
    for other in (0, 1, 3):
        s.select_frame(other)
        TC.same(snap(s), frames[n - 1 - other])
    s.select_frame(0)
    kept = [want if k == back else frames[n - 1 - k]["fb"] for k in range(n)]
    avg = TA.oracle(kept)
    assert not np.array_equal(avg, TA.oracle([frames[n - 1 - k]["fb"] for k in range(n)]))
    same(s.accumulate(n), avg, "the average over the kept frames")
    s.select_frame(back)
    same(s.get_frame_buffer(), want, "the kept frame after the average")
    # select_frame makes a kept frame's pose current (include/tiny_renderer.h): the slot still remembers its own, and
    # that is what the next cleared render draws
    q = par[0]
    PC._frame_p(s, q)
    TC.same(snap(s), PC.twin_frame(kind, ms, ks[n - 1 - back], q))
    s.close()


# ----------------------------------------------------------------------------------------------------------------------
# 7. a caller's buffer
# ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_warp_then_outline_in_a_callers_buffer(small_synthetic):
    """Noise in a caller's guarded buffer, the model drawn over it without a clear; the shift under a border that is not
    black, then the outline, both in place: the scratch frame is copied over the CALLER's bytes and no others."""
    import tiny_renderer_amd as T
    W, Hh = K.DENSE
    s, buf, f = TDF.dense_scene(small_synthetic, W, Hh, "noise")
    staged = K.stage_host("shift_paper", f["fb"])
    op = T.outline_params(**K.outline_kw(False))
    want = T.outline_host(f["z"], staged, op)
    assert not np.array_equal(staged, f["fb"]) and not np.array_equal(want, staged)
    K.stage_run(s, "shift_paper")
    assert s.sync() == 0
    TDF.in_buffer(buf, staged)
    s.outline(op)
    assert s.sync() == 0
    flags = clean_flags(s)
    TDF.in_buffer(buf, want)
    same(s.get_frame_buffer(), want, "through the getter")
    assert not (flags & K.lit(want)).any(), "a tile with colour in it is flagged clean"
    assert np.array_equal(bits(s.read_z_f32()), bits(f["z"])), "z changed"
    TDF.in_buffer(buf, want)
    s.close()


# ----------------------------------------------------------------------------------------------------------------------
# 8. the library's one read-back buffer across the getters of the newer stages
# ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_one_library_buffer_serves_the_newer_getters(small_synthetic):
    """resize (larger than the frame: the buffer grows), get_warped, get_convolved, to_yuv, get_graded, resolve and a
    small resize, in this order and reversed, on a drawn frame and then on a cleared scene, whose short-circuits must
    return black -- or the image of the border colour, of the bias, of the table's entry 0 -- whatever a larger getter
    left in the buffer."""
    import tiny_renderer_amd as T
    W, Hh = 256, 48
    s = scene(W, Hh, small_synthetic, K.PIPE, TC.DST_AT)
    lut = TS.random_lut(17, 5, c0=(9, 0, 200))
    s.set_lut(lut)
    g = WC.grids(W, Hh, 161, 47)["rotate7"]
    s.set_warp(g, 161, 47)
    wp = T.warp_params("border", WC.PAPER)
    cp = CC.params(K.kernel("emboss"), "border", CC.PAPER)

    def getters(fb):
        return [("resize(700, 500)", lambda: s.resize(700, 500), T.resize_host(fb, 700, 500)),
                ("get_warped", lambda: s.get_warped(wp), T.warp_host(fb, g, 161, 47, wp)),
                ("get_convolved", lambda: s.get_convolved(cp), T.convolve_host(fb, cp)),
                ("to_yuv", lambda: np.concatenate([q.reshape(-1) for q in s.to_yuv("i444")]), T.yuv_host(fb, "i444", flat=True)),
                ("get_graded", s.get_graded, T.grade_host(fb, lut)),
                ("resolve(2)", lambda: s.resolve(2), TD.box(fb, 2)),
                ("resize(67, 9)", lambda: s.resize(67, 9), T.resize_host(fb, 67, 9))]

    drive(s)
    fb = s.get_frame_buffer()
    assert fb.any()
    table = getters(fb)
    assert all(want.any() and not np.array_equal(want, fb) for _, _, want in table)
    for order in (table, table[::-1]):
        for name, get, want in order:
            same(np.asarray(get()), want, name)
    same(s.get_frame_buffer(), fb, "a getter changed the frame")
    black = np.zeros_like(fb)
    table = getters(black)
    assert (table[1][2] == np.array(WC.PAPER, np.uint8)).all(-1).any() and (table[4][2] == np.array((9, 0, 200), np.uint8)).all()
    assert not table[0][2].any() and not table[5][2].any() and table[2][2].any()
    for order in (table, table[::-1]):
        for name, get, want in order:
            s.clear()
            same(np.asarray(get()), want, name + " of a cleared scene")
    s.clear()
    assert not s.get_frame_buffer().any()
    s.close()
