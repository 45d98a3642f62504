"""The frame stages on dense frames, on the device: k_ao, k_dof, k_bloom, k_grade, k_outline, k_aa, k_resolve and k_stats
equal their host rules in every byte over frames in which every pixel holds colour.

The pattern of tests/test_grade.py's test_random_colours_in_a_callers_buffer: a caller's buffer between guard bytes is
filled with a backdrop (tests/dense_cases.py: noise, white, or the planted picture of tests/test_aa_host.py), handed to
the scene and drawn into WITHOUT a clear.  The expectation is the host rule over the scene's own snapshot of that frame.
A frame is never rendered twice into one buffer (without a clear its z would be tested against itself), so every case
that changes the frame takes a fresh scene and a fresh buffer.  tests/test_dense_frames_host.py pins the host rules
against numpy on the same frames and shows what each backdrop reaches."""
import numpy as np
import pytest

from tests import dense_cases as DC
from tests import test_composite as TC
from tests import test_outline as TO

bits, scene, clean_flags, tiles_any, box = TC.bits, TC.scene, TC.clean_flags, TC.tiles_any, TO.box
F32_MIN_BITS, G = DC.F32_MIN_BITS, DC.GUARD
SIZES_OF = {"aa": DC.SIZES, "outline": DC.SIZES, "grade": DC.SIZES, "ao": DC.SIZES, "bloom": DC.SIZES_HALO, "dof": DC.SIZES_HALO,
            "resolve": ((256, 48), DC.MIDDLE)}
OUT_STAGES = ("aa", "bloom", "dof", "outline", "grade", "resolve")
IN_STAGES = ("ao", "dof", "bloom", "grade", "outline", "aa")
# the one parameter set of a stage that runs in place and at odd addresses (an index into sets()): the defaults of aa
# (on noise: the full list), radius 15 at threshold 0, the largest background over a blurred model, the larger table,
# radius 3 with creases at opacity 100
ONE = {"aa": 0, "bloom": 0, "dof": 3, "grade": 1, "outline": 3, "ao": 0}


def cases(stages):
    rows = [(st, W, Hh, kind) for st in stages for W, Hh in SIZES_OF[st] for kind in DC.BACKDROPS]
    return pytest.mark.parametrize("stage,W,Hh,kind", rows, ids=["%s-%dx%d-%s" % r for r in rows])


def guarded(frame_bytes, extra=0):
    """A device buffer of GUARD + the frame (+ extra) + GUARD bytes, the guards (and the extra) 0xAA."""
    import torch
    raw = np.concatenate([np.full(G, 0xAA, np.uint8), np.ascontiguousarray(frame_bytes).reshape(-1), np.full(extra + G, 0xAA, np.uint8)])
    buf = torch.from_numpy(raw).cuda()
    torch.cuda.synchronize()
    assert buf.data_ptr() % 16 == 0, "the scene's own kernels store 16-byte pieces"
    return buf


def dense_scene(ms, W, Hh, kind, table=DC.table, draws=True):
    """A scene that has drawn its model over the backdrop in a caller's guarded buffer, that buffer, and the snapshot
    {"fb", "z"} of the frame.  table(W, Hh): where the model stands; draws=False: a size at which no model leaves a pixel
    (tests/extreme_cases.py), where the frame is asserted to be the backdrop."""
    back = DC.backdrop(kind, W, Hh)
    buf = guarded(back)
    s = scene(W, Hh, ms, DC.PIPE, table(W, Hh))
    # A new scene's z is memory nobody has written, and a clear that is still pending when the frame is rendered would
    # make the pass start from cleared COLOUR too: the backdrop would read as zeros.  So the clear is made real on the
    # scene's own buffer first (a getter does that); from here on z reads as f32::MIN, and the caller's buffer, which is
    # handed over afterwards, is colour the scene knows nothing about.
    s.clear()
    assert not s.get_frame_buffer().any()
    s.set_frame_buffer_device(buf.data_ptr() + G)
    TC.drive(s, DC.CAM, DC.LIGHT, clear=False)
    f = {"fb": s.get_frame_buffer(), "z": s.read_z_f32()}
    drawn = (bits(f["z"]) != F32_MIN_BITS)[::-1]
    if not draws:
        assert not drawn.any() and np.array_equal(f["fb"], back), "something was drawn, or the backdrop did not stay"
        return s, buf, f
    assert drawn.any() and not drawn.all() and not np.array_equal(f["fb"], back), "nothing was drawn over the backdrop"
    assert np.array_equal(f["fb"][~drawn], back[~drawn]), "the backdrop did not stay where nothing was drawn"
    if kind == "noise":
        assert DC.distinct(f["fb"]) > W * Hh * 3 // 6, "the frame is not noise"
    return s, buf, f


def in_buffer(buf, want, off=0):
    """The frame at GUARD + off of a guarded buffer is `want`, and the guards on both sides are untouched."""
    raw = buf.cpu().numpy()
    n = want.size
    got = raw[G + off:G + off + n].reshape(want.shape)
    assert np.array_equal(got, want), "%d bytes differ" % int((got != want).sum())
    assert (raw[:G] == 0xAA).all() and (raw[G + off + n:] == 0xAA).all(), "a guard byte changed"
    return raw


def default_params(stage, s, f):
    """The stage's parameter sets of tests/dense_cases.py."""
    W, Hh = s.width, s.height
    if stage == "resolve":
        assert DC.resolve_factors(W, Hh) == [2, 4]
    return {"aa": DC.aa_sets, "bloom": lambda: DC.BLOOM_SETS, "dof": lambda: DC.dof_sets(f), "outline": DC.outline_sets,
            "grade": lambda: DC.grade_luts(W), "ao": lambda: DC.AO_SETS, "resolve": lambda: DC.resolve_factors(W, Hh)}[stage]()


def sets(stage, s, f, params=None, changes=True):
    """[(label, the host rule's frame, call(out): the stage into `out` or with None in place, get(): the getter)]
    params: the stage's parameter sets (None: those of tests/dense_cases.py); changes=False: a frame that no set of the
    stage changes is fine."""
    import tiny_renderer_amd as T
    from tests import test_bloom as TB
    if params is None:
        params = default_params(stage, s, f)
    out = []
    if stage == "aa":
        for kw in params:
            p = T.aa_params(**kw)
            out.append((kw, T.aa_host(f["fb"], p), lambda o, p=p: s.antialias(p, out=o), lambda p=p: s.get_antialiased(p)))
    elif stage == "bloom":
        for q in params:
            p = TB.P(*q)
            out.append((q, T.bloom_host(f["fb"], p), lambda o, p=p: s.bloom(p, out=o), lambda p=p: s.get_bloom(p)))
    elif stage == "dof":
        for p in params:
            label = (int(p.background_radius), float(p.scale))
            out.append((label, T.depth_of_field_host(f["z"], f["fb"], p), lambda o, p=p: s.depth_of_field(p, out=o),
                        lambda p=p: s.get_depth_of_field(p)))
    elif stage == "outline":
        for kw in params:
            p = T.outline_params(**kw)
            out.append((kw, T.outline_host(f["z"], f["fb"], p), lambda o, p=p: s.outline(p, out=o), lambda p=p: s.get_outlined(p)))
    elif stage == "grade":
        for lut in params:
            out.append((lut.shape[0], T.grade_host(f["fb"], lut), lambda o, lut=lut: (s.set_lut(lut), s.grade(out=o)),
                        lambda lut=lut: (s.set_lut(lut), s.get_graded())[1]))
    elif stage == "ao":
        for kw in params:
            out.append((kw, T.ambient_occlusion_host(f["z"], f["fb"], **kw), lambda o, kw=kw: s.ambient_occlusion(**kw), None))
    elif stage == "resolve":
        for k in params:
            out.append((k, box(f["fb"], k), lambda o, k=k: s.resolve_into(k, o), lambda k=k: s.resolve(k)))
    assert out and (not changes or any(not np.array_equal(want, f["fb"]) for _, want, _, _ in out)), "every expectation is the input"
    return out


def reaches(stage, kind, f):
    """What the CPU test shows for the frame built on the host, on the device's own snapshot where it is cheap: on noise
    every whole tile fills k_aa's list past seven rounds of 256, and at 256 x 48 one fills it to the last slot."""
    if stage == "aa" and kind == "noise":
        n = DC.aa_survivors(f["fb"])
        assert min(n) > 1792 and (f["fb"].shape[:2] != (48, 256) or max(n) == 2048), n


@pytest.mark.gpu
@cases(OUT_STAGES)
def test_out_of_place(small_synthetic, stage, W, Hh, kind):
    """Every parameter set of the stage into device memory filled with 0x5A and through the getter: the host rule in
    every byte, and the caller's frame, its guards and z as they were."""
    import torch
    s, buf, f = dense_scene(small_synthetic, W, Hh, kind)
    reaches(stage, kind, f)
    zb = bits(f["z"])
    dev = TO.device_buffer(W * Hh * 3)
    for label, want, call, get in sets(stage, s, f):
        dev[:] = 0x5A
        torch.cuda.synchronize()                          # (torch fills on its own stream: not behind the scene's kernel)
        call(dev.data_ptr())
        assert s.sync() == 0
        raw = dev.cpu().numpy()
        got = raw[:want.size].reshape(want.shape)
        assert np.array_equal(got, want), "%r: %d bytes differ" % (label, int((got != want).sum()))
        assert (raw[want.size:] == 0x5A).all(), "%r: bytes behind the result were written" % (label,)
        got = get()
        assert np.array_equal(got, want), "getter %r: %d bytes differ" % (label, int((got != want).sum()))
        in_buffer(buf, f["fb"])
        assert np.array_equal(bits(s.read_z_f32()), zb), "z changed"
    assert np.array_equal(s.get_frame_buffer(), f["fb"])
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", DC.BACKDROPS)
@pytest.mark.parametrize("W,Hh", DC.SIZES_HALO)
def test_the_snapshot_is_the_frame_the_cpu_test_builds(small_synthetic, W, Hh, kind):
    """What tests/test_dense_frames_host.py shows about the oracle's pixels pasted over the backdrop holds for the
    device's frame: the two are the same bytes, colour and z."""
    from tests import test_dense_frames_host as TH
    s, buf, f = dense_scene(small_synthetic, W, Hh, kind)
    want = TH.dense(small_synthetic, W, Hh, kind)
    assert np.array_equal(f["fb"], want["fb"]) and np.array_equal(bits(f["z"]), bits(want["z"]))
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", DC.BACKDROPS)
@pytest.mark.parametrize("W,Hh", DC.SIZES)
def test_statistics(small_synthetic, W, Hh, kind):
    import tiny_renderer_amd as T
    s, buf, f = dense_scene(small_synthetic, W, Hh, kind)
    z = f["z"][bits(f["z"]) != F32_MIN_BITS]
    zkw = dict(z_lo=float(z.min()), z_scale=float(np.float32(200.0) / (z.max() - z.min())))
    for window in (None, (W // 3, Hh // 4, W // 2, Hh // 2)):
        want = T.frame_stats_host(f["fb"], f["z"], window=window, depth=True, **zkw)
        assert 0 < want.n_drawn < want.n_pixels and (want.luma != 0).sum() >= (8 if kind != "white" else 2)
        got = s.get_frame_stats(window=window, depth=True, **zkw)
        assert got == want, "%r != %r" % (got, want)
        assert s.get_frame_stats(window=window) == T.frame_stats_host(f["fb"], window=window)
    if kind == "noise":
        assert (T.frame_stats_host(f["fb"]).hist[:3] != 0).mean() > 0.9, "noise fills the bins of the channels"
    in_buffer(buf, f["fb"])
    s.close()


@pytest.mark.gpu
@cases(IN_STAGES)
def test_in_place(small_synthetic, stage, W, Hh, kind):
    """One parameter set of the stage in place in the caller's buffer: the host rule between guards that stay, the same
    through get_frame_buffer, no flag up over a tile that holds colour, z as it was."""
    s, buf, f = dense_scene(small_synthetic, W, Hh, kind)
    reaches(stage, kind, f)
    label, want, call, _ = sets(stage, s, f)[ONE[stage]]
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
# chains on noise at 256 x 48: in place, then the snapshot
# ----------------------------------------------------------------------------------------------------------------------

CHAIN = (256, 48, "noise")


@pytest.mark.gpu
def test_chain_outline_aa_bloom_grade(small_synthetic):
    import tiny_renderer_amd as T
    from tests import test_bloom as TB
    s, buf, f = dense_scene(small_synthetic, *CHAIN)
    op = T.outline_params(**DC.outline_sets()[3])
    ap, bp, lut = T.aa_params(), TB.P(*DC.BLOOM_SETS[2]), DC.grade_luts(CHAIN[0])[1]
    steps = [T.outline_host(f["z"], f["fb"], op)]
    steps.append(T.aa_host(steps[-1], ap))
    steps.append(T.bloom_host(steps[-1], bp))
    steps.append(T.grade_host(steps[-1], lut))
    for a, b in zip([f["fb"]] + steps, steps):
        assert not np.array_equal(a, b), "a step of the chain changes nothing"
    s.set_lut(lut)
    s.outline(op), s.antialias(ap), s.bloom(bp), s.grade()
    got = s.get_frame_buffer()
    assert np.array_equal(got, steps[-1]), "%d bytes differ" % int((got != steps[-1]).sum())
    in_buffer(buf, steps[-1])
    assert np.array_equal(bits(s.read_z_f32()), bits(f["z"]))
    s.close()


@pytest.mark.gpu
def test_chain_bloom_resolve_and_aa_twice(small_synthetic):
    import tiny_renderer_amd as T
    from tests import test_bloom as TB
    s, buf, f = dense_scene(small_synthetic, *CHAIN)
    bp = TB.P(*DC.BLOOM_SETS[0])
    lit = T.bloom_host(f["fb"], bp)
    assert not np.array_equal(lit, f["fb"])
    s.bloom(bp)
    assert np.array_equal(s.resolve(2), box(lit, 2))
    in_buffer(buf, lit)
    s.close()
    s, buf, f = dense_scene(small_synthetic, *CHAIN)
    ap = T.aa_params()
    once = T.aa_host(f["fb"], ap)
    twice = T.aa_host(once, ap)
    assert not np.array_equal(once, f["fb"]) and not np.array_equal(twice, once)
    s.antialias(ap), s.antialias(ap)
    assert np.array_equal(s.get_frame_buffer(), twice), "filtering twice is the rule applied twice"
    in_buffer(buf, twice)
    s.close()


# ----------------------------------------------------------------------------------------------------------------------
# odd addresses: 256 x 48 takes the wide form of k_bloom, k_grade, k_outline and k_aa unless an address says otherwise
# (tests/test_depth_of_field.py's aligned-and-odd-offset case has k_dof)
# ----------------------------------------------------------------------------------------------------------------------

ODD = ("bloom", "grade", "outline", "aa")


def offsets(stage):
    """Ascending, so that the bytes behind a frame have not held an earlier one.  2 for k_grade: the rows of a 4-aligned
    width are then 2 mod 4."""
    return (0, 1, 2, 4) if stage == "grade" else (0, 1, 4)


@pytest.mark.gpu
@pytest.mark.parametrize("stage", ODD)
def test_out_at_odd_addresses(small_synthetic, stage):
    W, Hh, kind = CHAIN
    n = W * Hh * 3
    s, buf, f = dense_scene(small_synthetic, W, Hh, kind)
    label, want, call, _ = sets(stage, s, f)[ONE[stage]]
    assert not np.array_equal(want, f["fb"])
    tgt = guarded(np.full(n, 0xAA, np.uint8))
    before = None
    for off in offsets(stage):
        call(tgt.data_ptr() + G + off)
        assert s.sync() == 0
        raw = tgt.cpu().numpy()
        got = raw[G + off:G + off + n].reshape(Hh, W, 3)
        assert np.array_equal(got, want), "offset %d: %d bytes differ" % (off, int((got != want).sum()))
        assert (raw[:G] == 0xAA).all() and (raw[G + off + n:] == 0xAA).all(), "offset %d: a guard byte changed" % off
        assert before is None or np.array_equal(raw[G:G + off], before[G:G + off]), "offset %d: bytes ahead of `out` were written" % off
        before = raw
        in_buffer(buf, f["fb"])
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("stage", ODD)
def test_in_place_at_odd_addresses(small_synthetic, stage):
    """The scene's own kernels store 16-byte pieces, so the frame is rendered at an aligned address; its bytes are copied
    to the odd one, which is handed over: the launcher must see the alignment and take the guarded form."""
    import torch
    W, Hh, kind = CHAIN
    n = W * Hh * 3
    tgt = guarded(np.full(n, 0xAA, np.uint8), extra=8)
    for off in offsets(stage)[1:]:
        s, buf, f = dense_scene(small_synthetic, W, Hh, kind)
        label, want, call, _ = sets(stage, s, f)[ONE[stage]]
        assert s.sync() == 0
        tgt[G:G + off] = 0xAA
        tgt[G + off:G + off + n] = buf[G:G + n]
        torch.cuda.synchronize()
        s.set_frame_buffer_device(tgt.data_ptr() + G + off)
        assert np.array_equal(s.get_frame_buffer(), f["fb"])
        call(None)
        assert s.sync() == 0
        raw = tgt.cpu().numpy()
        got = raw[G + off:G + off + n].reshape(Hh, W, 3)
        assert np.array_equal(got, want), "offset %d: %d bytes differ" % (off, int((got != want).sum()))
        assert (raw[:G + off] == 0xAA).all() and (raw[G + off + n:] == 0xAA).all(), "offset %d: a guard byte changed" % off
        assert np.array_equal(s.get_frame_buffer(), want)
        in_buffer(buf, f["fb"])
        s.close()
