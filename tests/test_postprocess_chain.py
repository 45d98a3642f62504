"""The post-processing chain composed: resolve, composite, ambient occlusion, accumulation and depth of field share the
per-tile fast-clear flags of z and colour, ensure_depth (the depth-only repeat of a pass whose depth stayed on the chip),
the kept frames and the records of page-locked read-back buffers.  Each stage is pinned against its rule in its own file;
here they follow one another on one scene.

The expectation is always a chain of host rules (tr_ao_host, tr_dof_host, tr_accumulate_host's numpy restatement, the
numpy merge of tests/test_composite.py, the box filter) applied to a snapshot from a twin scene, or from the same scene
before it is rendered again; every comparison is np.array_equal.  Cases that exist to reach a path assert on the snapshot
that they reach it, and test_the_cases_hold_what_they_are_about decides with the CPU oracle alone what can be decided
without a GPU, for this file and for the additions to tests/test_depth_of_field.py."""
import numpy as np
import pytest

from tests import helpers as H
from tests import test_accumulate as TA
from tests import test_composite as TC
from tests import test_composite_consumers as TCC
from tests import test_depth_of_field as TD
from tests.test_composite import other_synthetic  # noqa: F401
from tests.test_morph import _frame_p, _targets

bits, drive, scene, snap, clean_flags, tiles_any, merge = TC.bits, TC.drive, TC.scene, TC.snap, TC.clean_flags, TC.tiles_any, TC.merge
F32_MIN_BITS = TC.F32_MIN_BITS
box = TD.box
BOTH = pytest.mark.parametrize("store_depth", [False, True], ids=["transient", "stored"])
AO = dict(radius=8, rings=2)
ORDER_SHAPES = {(384, 48): TC.DST_AT, (208, 40): TD.PLACE[(208, 40)]}


def drawn(f):
    return bits(f["z"]) != F32_MIN_BITS


def lit(fb):
    return tiles_any(fb[::-1].any(-1))


def ao(f, **kw):
    import tiny_renderer_amd as T
    return T.ambient_occlusion_host(f["z"], f["fb"], **dict(AO, **kw))


def dof(f, p):
    import tiny_renderer_amd as T
    return T.depth_of_field_host(f["z"], f["fb"], p)


def both_orders(f, p, grey):
    """(ambient occlusion then depth of field, depth of field then ambient occlusion) by the host rules."""
    first = dof(dict(f, fb=ao(f, grey=grey)), p)
    second = ao(dict(f, fb=dof(f, p)), grey=grey)
    return first, second


# ------------------------------------------------------------------------------------------------------------------
# Both orders of ambient occlusion and depth of field
# ------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@BOTH
@pytest.mark.parametrize("pipe", ["phong", "shadow"])
@pytest.mark.parametrize("W,Hh", sorted(ORDER_SHAPES))
def test_ambient_occlusion_and_depth_of_field_in_either_order(small_synthetic, W, Hh, pipe, store_depth):
    s = scene(W, Hh, small_synthetic, pipe, ORDER_SHAPES[(W, Hh)], tap=True, store_depth=store_depth)
    drive(s)
    f, before = snap(s), TD.state(s)
    p = TD.params_for(f, 3, bg=2)
    for grey in (False, True):
        want = both_orders(f, p, grey)
        assert not np.array_equal(want[0], want[1]), "the two orders give one frame"
        for order in (0, 1):
            drive(s)
            if order == 0:
                s.ambient_occlusion(grey=grey, **AO), s.depth_of_field(p)
            else:
                s.depth_of_field(p), s.ambient_occlusion(grey=grey, **AO)
            flags = clean_flags(s)
            got = s.get_frame_buffer()
            assert np.array_equal(got, want[order]), "grey %r, order %d: %d bytes differ" % (grey, order, int((got != want[order]).sum()))
            assert not (flags & lit(want[order])).any(), "a tile with colour in it is flagged clean"
            TD.same_state(TD.state(s), before)
    s.close()


# ------------------------------------------------------------------------------------------------------------------
# Posed scenes with transient depth: ensure_depth must draw the frame's pose, not the current one
# ------------------------------------------------------------------------------------------------------------------

POSED_W, POSED_H, POSED_N = 208, 64, 4
KINDS = ("skin", "morph", "xform", "inst")
STAGES = ("ao", "dof")


def pose(kind, k):
    if kind == "skin":
        return TCC.palette2(k)
    if kind == "morph":
        return np.array([0.5 * k, 1.0 - 0.4 * k], np.float32)
    if kind == "xform":
        return TCC.xtable("dst", k)
    return np.array([[-0.25 + 0.12 * k, 0.1 * k, 0.0, 0.7 - 0.05 * k]], np.float32)


def set_pose(s, kind, k):
    {"skin": s.set_bone_palette, "morph": s.set_morph_weights, "xform": s.set_instance_transforms, "inst": s.set_instances}[kind](pose(kind, k))


def posed_scene(kind, ms, k, **kw):
    """A scene of the mesh itself that draws pose k of `kind` on the device; depth stays transient."""
    mesh = ms[0]
    if kind == "xform":
        return scene(POSED_W, POSED_H, ms, "phong", None, instance_transforms=pose(kind, k), **kw)
    if kind == "inst":
        return scene(POSED_W, POSED_H, ms, "phong", pose(kind, k), **kw)
    s = scene(POSED_W, POSED_H, ms, "phong", TC.DST_AT, **kw)
    if kind == "skin":
        s.set_skin(*TCC.rig2(mesh), n_bones=2)
    else:
        dp, dn = _targets(mesh)
        s.set_morph_targets(dp[:2], dn[:2])
    set_pose(s, kind, k)
    return s


def twin_mesh(kind, mesh, k):
    """(mesh, instance table or None) of the plain scene that draws pose k: posed on the host."""
    import tiny_renderer_amd as T
    if kind == "skin":
        return T.skin_mesh(mesh, *TCC.rig2(mesh), pose(kind, k)), TC.DST_AT
    if kind == "morph":
        dp, dn = _targets(mesh)
        pos, nrm = T.morph_mesh(mesh, dp[:2], dn[:2], pose(kind, k))
        return dict(mesh, pos=pos, nrm=nrm), TC.DST_AT
    if kind == "xform":
        return TCC.host_posed("xform", "dst", mesh, k)
    return mesh, pose(kind, k)


def twin_frame(kind, ms, k, q=None):
    m, at = twin_mesh(kind, ms[0], k)
    t = scene(POSED_W, POSED_H, (m, ms[1]), "phong", at)
    _frame_p(t, TCC.frame_params(1)[0] if q is None else q)
    f = snap(t)
    t.close()
    return f


def stage_params(stage, f):
    return TD.params_for(f, 3, bg=1) if stage == "dof" else None


def run_stage(s, stage, p):
    s.depth_of_field(p) if stage == "dof" else s.ambient_occlusion(**AO)


def stage_host(stage, f, p):
    return dof(f, p) if stage == "dof" else ao(f)


def poses_show(stage, f, other, p):
    """The stage over the frame's colour with ANOTHER pose's z differs from the rule: a repeat under the wrong pose shows."""
    want = stage_host(stage, f, p)
    assert not np.array_equal(want, f["fb"]), "the stage changes nothing"
    assert not np.array_equal(stage_host(stage, dict(f, z=other["z"]), p), want), "another pose's depth would not show"
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("stage", STAGES)
@pytest.mark.parametrize("kind", KINDS)
def test_a_stage_over_a_posed_frame_draws_the_frames_pose(small_synthetic, kind, stage):
    """Pose 0 is set and rendered, pose 1 set without a render, then the stage: the depth it repeats the pass for is pose
    0's.  The next cleared render draws pose 1."""
    f0, f1 = twin_frame(kind, small_synthetic, 0), twin_frame(kind, small_synthetic, 1)
    p = stage_params(stage, f0)
    want = poses_show(stage, f0, f1, p)
    s = posed_scene(kind, small_synthetic, 0)
    q = TCC.frame_params(1)[0]
    _frame_p(s, q)
    set_pose(s, kind, 1)
    run_stage(s, stage, p)
    assert np.array_equal(s.get_frame_buffer(), want)
    assert np.array_equal(bits(s.read_z_f32()), bits(f0["z"]))
    _frame_p(s, q)
    TC.same(snap(s), f1)
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("stage", STAGES)
@pytest.mark.parametrize("kind", KINDS)
def test_a_stage_over_a_kept_frame_with_a_pose_per_frame(small_synthetic, kind, stage):
    """Four frames by one launch with a pose each; frame `back` = 2 is selected, ANOTHER frame's pose made current, and
    the stage runs: depth and colour are those of the selected frame's pose; the other kept frames stay."""
    n, back = POSED_N, 2
    par = TCC.frame_params(n)
    ks = [0.5 * i for i in range(n)]
    frames = [twin_frame(kind, small_synthetic, ks[i], par[i]) for i in range(n)]    # render order
    sel = frames[n - 1 - back]
    p = stage_params(stage, sel)
    want = poses_show(stage, sel, frames[n - 1], p)
    s = posed_scene(kind, small_synthetic, 0, frames_per_launch=n)
    key = {"skin": "bone_palettes", "morph": "morph_weights", "xform": "instance_transforms", "inst": "instances"}[kind]
    s.render_frames(par, **{key: np.stack([pose(kind, k) for k in ks])})
    assert s.frames_kept() == n
    s.select_frame(back)
    set_pose(s, kind, ks[back])                  # (frame n - 1 - back is selected: pose `back` is another frame's)
    run_stage(s, stage, p)
    assert np.array_equal(s.get_frame_buffer(), want)
    assert np.array_equal(bits(s.read_z_f32()), bits(sel["z"]))
    for other in (0, 1, 3):
        s.select_frame(other)
        TC.same(snap(s), frames[n - 1 - other])
    s.close()


# ------------------------------------------------------------------------------------------------------------------
# A stage on one kept frame, then the average
# ------------------------------------------------------------------------------------------------------------------

ACC_W, ACC_H, ACC_N = 384, 48, 4


def acc_views():
    """views() of tests/test_accumulate.py with every frame in the left tile column and well clear of the second, but
    the frame that becomes kept frame 1, whose rim stops two pixels short of it."""
    par = TA.views(ACC_N, 1.3, 1.27)
    par[ACC_N - 2] = TA.views(ACC_N, 1.3, 1.155)[ACC_N - 2]
    return par


def acc_params(f):
    return TD.params_for(f, 8, near=True)       # the rim is blurred: it spreads over the tile's border


def spill_tiles(flags, blurred):
    """Tiles flagged clean in EVERY kept frame (flags [n, ty, tx]) that the blurred frame puts colour into."""
    return flags.all(0) & lit(blurred)


@pytest.mark.gpu
@pytest.mark.parametrize("stage", ["dof", "grey_ao"])
def test_a_stage_on_a_kept_frame_then_the_average(small_synthetic, stage):
    """k_accumulate skips a frame's tile whose colour flag is up: the blur in place has to hand frame 1 a LOWERED flag
    for the tile it spread colour into, or the average loses that colour."""
    import torch
    W, Hh, n = ACC_W, ACC_H, ACC_N
    par = acc_views()
    mk = lambda: scene(W, Hh, small_synthetic, "phong", frames_per_launch=n)
    twin = mk()
    twin.render_frames(par)
    assert twin.frames_kept() == n
    flags = TA.kept_flags(twin, n)
    kept = []
    for k in range(3):
        twin.select_frame(k)
        kept.append(snap(twin))
    twin.close()
    if stage == "dof":
        p = acc_params(kept[1])
        staged = dof(kept[1], p)
        spill = spill_tiles(flags, staged)
        assert spill.any(), "the blur spreads into no tile that is clean in every kept frame"
    else:
        p = None
        staged = ao(kept[1], grey=True)
        assert not np.array_equal(staged, kept[1]["fb"])
        spill = np.zeros_like(flags[0])
    want = TA.oracle([kept[0]["fb"], staged, kept[2]["fb"]])
    assert not np.array_equal(want, TA.oracle([k["fb"] for k in kept]))
    assert stage != "dof" or (spill & lit(want)).any(), "the average is zero in every spill tile"
    s = mk()
    s.render_frames(par)
    s.select_frame(1)
    if stage == "dof":
        s.depth_of_field(p)
    else:
        s.ambient_occlusion(grey=True, **AO)
    assert np.array_equal(s.accumulate(3), want), "through the getter"
    dev = torch.full((W * Hh * 3,), 0xAB, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    s.accumulate_into(3, dev.data_ptr())
    assert s.sync() == 0
    torch.cuda.synchronize()
    assert np.array_equal(dev.cpu().numpy().reshape(Hh, W, 3), want), "into device memory"
    s.accumulate_in_place(3)
    assert np.array_equal(s.get_frame_buffer(), want), "in place"
    assert not (clean_flags(s) & lit(want)).any()
    for k in (0, 2):
        s.select_frame(k)
        TC.same(snap(s), kept[k])
    s.close()


# ------------------------------------------------------------------------------------------------------------------
# The whole chain
# ------------------------------------------------------------------------------------------------------------------

CHAIN_AT = np.array([[-0.55, 0.1, 0.2, 0.5]], np.float32)     # the second scene's object, over the left tile columns


@pytest.mark.gpu
@BOTH
@pytest.mark.parametrize("pipe", ["phong", "shadow"])
def test_the_whole_chain(small_synthetic, other_synthetic, pipe, store_depth):
    """accumulate in place, ambient occlusion, depth of field, composite as dst, resolve(2).  (Scenes with the winner tap
    keep one frame, so the merge is checked through colour and z.)"""
    W, Hh, n = ACC_W, ACC_H, ACC_N
    par = TA.views(n)
    mk = lambda: (scene(W, Hh, small_synthetic, pipe, frames_per_launch=n, store_depth=store_depth),
                  scene(W, Hh, other_synthetic, "phong", CHAIN_AT, store_depth=store_depth))
    a, b = mk()
    a.render_frames(par), drive(b, light=0.2)
    f = {"fb": TA.oracle(TA.kept(a, n)), "z": a.read_z_f32(), "win": None}
    fb_ = dict(snap(b), win=None)
    a.close(), b.close()
    assert f["fb"].any()
    p = TD.params_for(f, 3, bg=2)
    shaded = ao(f)
    blurred = dof(dict(f, fb=shaded), p)
    assert not np.array_equal(shaded, f["fb"]) and not np.array_equal(blurred, shaded)
    want, wins = merge(dict(f, fb=blurred), fb_)
    assert wins.any() and (drawn(fb_) & ~wins).any() and (drawn(f) & ~wins).any()
    a, b = mk()
    a.render_frames(par), drive(b, light=0.2)
    a.accumulate_in_place(n), a.ambient_occlusion(**AO), a.depth_of_field(p), a.composite(b)
    assert np.array_equal(a.resolve(2), box(want["fb"], 2))
    TC.same(snap(a), want)
    a.close(), b.close()


# ------------------------------------------------------------------------------------------------------------------
# The page-locked read-back around a frame changed in place
# ------------------------------------------------------------------------------------------------------------------

ORBIT_W, ORBIT_H = 512, 64
ORBIT_AT = TC._small(-0.4, 0.1)
SCRIBBLE = 55


def read_into(s, P):
    s.get_frame_buffer_async(P)
    assert s.sync() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("scribble", [False, True], ids=["untouched", "scribbled"])
@pytest.mark.parametrize("stage", ["dof", "accumulate"])
def test_read_back_orbit_around_a_frame_changed_in_place(small_synthetic, stage, scribble):
    """One page-locked buffer: frame A; A changed in place, with colour in a tile the render left flagged clean; a fresh
    frame B in which that tile is clean again (the buffer must hold zeros there); a clear (zeros everywhere).  scribbled:
    the caller overwrites the buffer before B and says so."""
    n = ACC_N
    par = TA.views(n)
    if stage == "dof":
        W, Hh = ORBIT_W, ORBIT_H
        mk = lambda: scene(W, Hh, small_synthetic, "phong", ORBIT_AT)
        first, fresh = (lambda q: drive(q)), (lambda q: drive(q, cam=-0.6))
    else:
        W, Hh = ACC_W, ACC_H
        mk = lambda: scene(W, Hh, small_synthetic, "phong", frames_per_launch=n)
        first, fresh = (lambda q: q.render_frames(par)), (lambda q: _frame_p(q, par[n - 2]))
    twin = mk()
    first(twin)
    flags_a = clean_flags(twin)
    A = snap(twin)
    if stage == "dof":
        p = TD.params_for(A, 8, near=True)
        changed = dof(A, p)
    else:
        changed = TA.oracle(TA.kept(twin, n))
    fresh(twin)
    flags_b = clean_flags(twin)
    B = snap(twin)
    twin.close()
    spill = flags_a & lit(changed) & flags_b
    assert spill.any(), "no tile is clean in A and in B and holds colour in between"
    s = mk()
    P = s.pinned_frame()
    P[...] = 99
    first(s)
    read_into(s, P)
    assert np.array_equal(P, A["fb"])
    if stage == "dof":
        s.depth_of_field(p)
    else:
        s.accumulate_in_place(n)
    read_into(s, P)
    assert np.array_equal(P, changed)
    fresh(s)
    if scribble:
        P[...] = SCRIBBLE
        s.host_buffer_written(P)
    read_into(s, P)
    assert np.array_equal(P, B["fb"]), "%d pixels differ" % int((P != B["fb"]).any(-1).sum())
    s.clear()
    read_into(s, P)
    assert not P.any()
    s.close()


# ------------------------------------------------------------------------------------------------------------------
# What can be decided without a GPU
# ------------------------------------------------------------------------------------------------------------------

def _cpu(W, Hh, ms, at, pipe="phong", cam=0.3, light=0.7, q=None):
    """The oracle's frame of the mesh under an instance table, as snap() returns a scene's."""
    import tiny_renderer_amd as T
    from oracle import oracle as O
    s = O.Scene(W, Hh, ms[0] if at is None else T.apply_instances(ms[0], at), ms[1], pipe)
    s.clear()
    if q is None:
        s.set_light_direction(H.light(light)), s.set_camera(*H.camera(cam))
    else:
        s.set_light_direction(q[0:3]), s.set_camera(q[3:6], q[6:9], q[9:12])
    s.render()
    out = {"fb": s.get_frame_buffer(), "z": s.z_f32(), "win": None}
    s.close()
    return out


def _clean(f, margin=3):
    """The tiles no drawn pixel comes within `margin` pixels of: clean by the polygons' boxes too."""
    d = drawn(f)
    wide = np.zeros_like(d)
    for dy in range(-margin, margin + 1):
        for dx in range(-margin, margin + 1):
            wide |= np.roll(np.roll(d, dy, 0), dx, 1)
    return ~tiles_any(wide)


def test_the_cases_hold_what_they_are_about(built, small_synthetic):
    """With the oracle's frames and the host functions alone: the three kinds of vote tile; drawn, blurred pixels in the
    partial tile column and row of 208 x 40 and 144 x 24; a tile that was drawn, is clean and lies next to a drawn one for
    the stale halo, with either stale field showing; the spill tile that no kept frame draws; the spill tile of the
    read-back orbit; and that the two orders of ambient occlusion and depth of field differ.  (A tile counts as clean
    here when the oracle draws no pixel in it; the scene's flags go by the polygons' boxes, which the GPU cases assert.)"""
    ms = small_synthetic
    f = _cpu(TD.VOTE_W, TD.VOTE_H, ms, TD.VOTE_AT)
    p = TD.vote_params(f)
    TD.assert_vote_tiles(f, p, TD.host(f, p))
    for (W, Hh), at in TD.PLACE.items():
        for pipe in ("phong", "shadow"):
            f = _cpu(W, Hh, ms, at, pipe)
            for R, bg in TD.RADII:
                p = TD.params_for(f, R, bg)
                TD.partial_tiles_are_blurred(f, p, TD.host(f, p))
    first = _cpu(TD.STALE_W, TD.STALE_H, ms, TD.STALE_FIRST)
    for x, y in TD.STALE_THEN:
        then = _cpu(TD.STALE_W, TD.STALE_H, ms, TC._small(x, y))
        p = TD.params_for(then, 8, near=True)
        TD.assert_stale_halo(first, then, _clean(then), p, TD.host(then, p))
    par = acc_views()
    kept = [_cpu(ACC_W, ACC_H, ms, None, q=par[ACC_N - 1 - k]) for k in range(ACC_N)]
    flags = np.array([~tiles_any(drawn(k)) for k in kept])
    blurred = dof(kept[1], acc_params(kept[1]))
    spill = spill_tiles(flags, blurred) & lit(TA.oracle([kept[0]["fb"], blurred, kept[2]["fb"]]))
    assert spill.any(), "the blur of kept frame 1 puts nothing the average keeps into a tile that every kept frame leaves empty"
    assert all(np.nonzero(drawn(k).any(0))[0].max() <= 125 for k in kept), "a kept frame comes within two pixels of the second tile column"
    A, B = _cpu(ORBIT_W, ORBIT_H, ms, ORBIT_AT), _cpu(ORBIT_W, ORBIT_H, ms, ORBIT_AT, cam=-0.6)
    changed = dof(A, TD.params_for(A, 8, near=True))
    assert (~tiles_any(drawn(A)) & ~tiles_any(drawn(B)) & lit(changed)).any(), "the orbit has no spill tile"
    par = TA.views(ACC_N)
    kept = [_cpu(ACC_W, ACC_H, ms, None, q=par[ACC_N - 1 - k]) for k in range(ACC_N)]
    assert (~tiles_any(drawn(kept[0])) & ~tiles_any(drawn(kept[1])) & lit(TA.oracle([k["fb"] for k in kept]))).any(), \
        "the orbit around an average has no spill tile"
    for (W, Hh), at in ORDER_SHAPES.items():
        for pipe in ("phong", "shadow"):
            f = _cpu(W, Hh, ms, at, pipe)
            p = TD.params_for(f, 3, bg=2)
            for grey in (False, True):
                a, b = both_orders(f, p, grey)
                assert not np.array_equal(a, b), (W, Hh, pipe, grey)
