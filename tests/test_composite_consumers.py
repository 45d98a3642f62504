"""What reads a scene's frame AFTER tr_scene_composite wrote it from outside the scene's own render chain, and what the
merge reads of a frame whose depth it has to draw again.

A. Consumers of dst's flags: k_composite lowers dst's colour-clean and z flags by one store of lane 0 where src opens a
   tile dst had left clean.  k_resolve, the sparse read-back into page-locked memory (with its own record of the host
   buffer), the depth views and band_tiles() skip work on those flags: each of them is run on a merged frame here.
B. Posed inputs: for a transient-depth frame the merge repeats the frame's colour pass for depth alone, with the slot's
   remembered instance table and pose -- not the scene's current one.  Skinned, morphed and transformed scenes on either
   side, kept frames of fused groups with a pose per frame, layers.
C. A CPU test that computes, with the oracle alone, that every case above has the tiles it is about.

Expected values never come from the merged scene: the merged frame is the numpy rule (`merge`, tests/test_composite.py)
over the frames of twin scenes that are never merged -- of the HOST-posed meshes (T.skin_mesh / T.morph_mesh /
T.transform_mesh) where a scene is posed --, the resolved frame is `box` (tests/test_resolve.py) of it, the depth view
the restated f32 -> u8 rule.  Every comparison is exact."""
import itertools

import numpy as np
import pytest

from tests import helpers as H
from tests.test_composite import (DST_AT, F32_MIN_BITS, SRC_AT, band_y, bits, clean_flags, concat, drive, merge,  # noqa: F401
                                  oracle_frame, other_synthetic, same, scene, snap, tiles_any)
from tests.test_instance_transforms import _rot
from tests.test_morph import _frame_p, _targets
from tests.test_resolve import box

FACTORS = (2, 4, 8)
HH = 128                      # eight tile rows: room for tiles of every kind (the CPU test below asserts them)
WIDTHS = (256, 208, 200)      # WIDE forms and whole tiles; WIDE and a partial last tile; the narrow forms, no tile read-back
BAND = (512, 128, (16, 96))   # rows that are multiples of 16 and of every resolve factor
AT3 = np.array([[0.0, -0.1, 0.3, 0.45]], np.float32)    # a third object, in front of the two
SMALL_AT = np.array([[0.0, -0.6, 0.0, 0.3]], np.float32)  # a small object at the bottom of a 128 x 64 frame
SRC_LIGHT = 0.2
BOTH = pytest.mark.parametrize("store_depth", [False, True], ids=["transient", "stored"])


def grey(z):
    """get_z_buffer of z [H, W] (row 0 = bottom): scene.rs:101-113, `as u8` of an f32 saturates and takes NaN to 0."""
    with np.errstate(invalid="ignore"):
        u8 = np.nan_to_num(np.clip(np.trunc(z), 0, 255)).astype(np.uint8)
    return np.repeat(u8[::-1, :, None], 3, axis=2)


def covered(f):
    return bits(f["z"]) != F32_MIN_BITS


def tile_sets(fd, fs, band=None):
    """The three kinds of tile of a merge, from two un-merged frames: [tiles_y, tiles_x] bool each, tiles outside the
    band (output rows, row 0 = top) masked out.  opened: src wins a pixel and dst drew nothing in the whole tile (the
    flag-lowering path); shared: both drew and each wins a pixel; clean: neither drew."""
    wins = merge(fd, fs)[1]
    cd, cs = covered(fd), covered(fs)
    inside = np.ones(cd.shape, bool)
    if band is not None:
        y0, y1 = band_y(cd.shape[0], band)
        inside[:y0], inside[y1:] = False, False
    opened = tiles_any(wins & inside) & ~tiles_any(cd)
    shared = tiles_any(wins & inside) & tiles_any(cd & cs & ~wins & inside)
    clean = ~tiles_any(cd) & ~tiles_any(cs) & tiles_any(inside)
    return opened, shared, clean


def lit_tiles(fb):
    """[tiles_y, tiles_x]: does the tile hold a non-zero colour byte (fb as the getter returns it, row 0 = top)?"""
    return tiles_any(fb[::-1].any(-1))


# ------------------------------------------------------------------------------------------------------------------
# Poses: one kind at a time, two of each (k = 0, 1), on either side
# ------------------------------------------------------------------------------------------------------------------

KINDS = ("skin", "morph", "xform")
MORPH_WEIGHTS = (np.array([0.0, 1.0], np.float32), np.array([1.25, 0.0], np.float32))   # two targets, one zero weight


def rig2(mesh):
    """A two-bone rig in the manner of tests/test_skin.py's: the cap has all-zero weights (it keeps the mesh's bits), the
    base one influence of weight 1.0f on bone 1, and in between bone 0 and bone 1 blend by height (two of the four
    influences are zero there)."""
    pos = np.asarray(mesh["pos"], np.float32).reshape(-1, 3)
    y = pos[:, 1].astype(np.float64)
    r = np.abs(y).max()
    t = np.clip((y / r + 1.0) / 2.0, 0.0, 1.0)
    bones = np.tile(np.array([0, 1, 1, 0], np.uint32), (pos.shape[0], 1))
    weights = np.stack([1.0 - t, t, np.zeros_like(t), np.zeros_like(t)], axis=1).astype(np.float32)
    cap, base = y > 0.9 * r, y < -0.9 * r
    weights[cap] = 0.0
    bones[base] = np.array([1, 0, 0, 0], np.uint32)
    weights[base] = np.array([1.0, 0.0, 0.0, 0.0], np.float32)
    assert cap.any() and base.any() and (~cap & ~base).any()
    return bones, weights


def palette2(k):
    import tiny_renderer_amd as T
    lin = [_rot(20 + 35 * k), _rot(35 - 25 * k, 10, -15)]
    off = [[0.0, 0.06 * k, 0.0], [0.1, -0.05 * k, 0.0]]
    return T.instance_transforms(np.array(lin), np.array(off))


def xtable(role, k):
    """Two entries: the object where DST_AT / SRC_AT puts it, turned (further with k), and a small MIRRORED copy."""
    import tiny_renderer_amd as T
    at = (DST_AT if role == "dst" else SRC_AT)[0].astype(np.float64)
    side = -1.0 if role == "dst" else 1.0
    lin = [_rot(30 + 40 * k, 10 * k) * at[3], _rot(15, -10, 5) @ np.diag([-0.22, 0.22, 0.22])]
    off = [at[:3] + np.array([0.0, 0.07 * k, 0.0]), [side * 0.72, -0.45 + 0.05 * k, 0.1]]
    t = T.instance_transforms(np.array(lin), np.array(off))
    assert np.linalg.det(t[1, 0:12].reshape(3, 4)[:, :3].astype(np.float64)) < 0
    return t


def host_posed(kind, role, mesh, k):
    """(mesh, instance table or None) of the plain scene that draws what the posed scene draws under pose k."""
    import tiny_renderer_amd as T
    at = DST_AT if role == "dst" else SRC_AT
    if kind == "skin":
        return T.skin_mesh(mesh, *rig2(mesh), palette2(k)), at
    if kind == "morph":
        dp, dn = _targets(mesh)
        pos, nrm = T.morph_mesh(mesh, dp[:2], dn[:2], MORPH_WEIGHTS[k])
        return dict(mesh, pos=pos, nrm=nrm), at
    table = xtable(role, k)
    pos, nrm = T.transform_mesh(mesh, table)
    idx = np.asarray(mesh["idx"], np.uint32).reshape(-1, 9)
    n_pos, n_nrm = np.asarray(mesh["pos"]).reshape(-1, 3).shape[0], np.asarray(mesh["nrm"]).reshape(-1, 3).shape[0]
    parts = []
    for e in range(table.shape[0]):
        q = idx.copy()
        q[:, 0::3] += np.uint32(e * n_pos)
        q[:, 2::3] += np.uint32(e * n_nrm)
        parts.append(q)
    return dict(mesh, pos=pos, nrm=nrm, idx=np.concatenate(parts)), None


def drawn_mesh(kind, role, mesh, k):
    """The mesh the oracle draws: the host-posed mesh with its instance table applied."""
    import tiny_renderer_amd as T
    if kind is None:
        return T.apply_instances(mesh, DST_AT if role == "dst" else SRC_AT)
    posed, at = host_posed(kind, role, mesh, k)
    return posed if at is None else T.apply_instances(posed, at)


def set_pose(s, kind, role, k):
    if kind == "skin":
        s.set_bone_palette(palette2(k))
    elif kind == "morph":
        s.set_morph_weights(MORPH_WEIGHTS[k])
    else:
        s.set_instance_transforms(xtable(role, k))


def posed_scene(W, Hh, kind, role, ms, pipe, k=0, tap=False, **kw):
    """A scene of the mesh itself that draws pose k of `kind` on the device."""
    mesh = ms[0]
    if kind == "xform":
        s = scene(W, Hh, ms, pipe, None, tap, instance_transforms=xtable(role, k), **kw)
    else:
        s = scene(W, Hh, ms, pipe, DST_AT if role == "dst" else SRC_AT, tap, **kw)
        if kind == "skin":
            s.set_skin(*rig2(mesh), n_bones=2)
        else:
            dp, dn = _targets(mesh)
            s.set_morph_targets(dp[:2], dn[:2])
        set_pose(s, kind, role, k)
    return s


def twin_scene(W, Hh, kind, role, ms, pipe, k=0, tap=False, **kw):
    """The plain scene of the host-posed mesh (kind None: of the mesh itself)."""
    if kind is None:
        return scene(W, Hh, ms, pipe, DST_AT if role == "dst" else SRC_AT, tap, **kw)
    posed, at = host_posed(kind, role, ms[0], k)
    return scene(W, Hh, (posed, ms[1]), pipe, at, tap, **kw)


def frame_params(n):
    p = np.zeros((n, 12), np.float32)
    for k in range(n):
        p[k, 0:3] = H.light(0.7 - 0.1 * k)
        p[k, 3:6], p[k, 6:9], p[k, 9:12] = H.camera(0.3 - 0.15 * k)
    return p


GROUP_W, GROUP_N = 208, 4
SELECT_ORDER = (2, 0, 3, 1)
MORPH_ROWS_BOUND = 32 + 4 * 4 + 1    # a set per frame slot, per frame of the groups in flight, the current state
# ... and what that comes to HERE: a set of rows is allocated when a chain first reads a pose, once per pose, and these
# cases draw GROUP_N poses and no more (the merge's repeat reads the rows the frame's own pass left; a pose that is set
# and never rendered gets none).  So: the frames kept, plus one for the current pose
GROUP_ROWS = GROUP_N + 1
assert GROUP_ROWS <= MORPH_ROWS_BOUND


def group_palettes():
    return np.stack([palette2(0.5 * i) for i in range(GROUP_N)])


def group_tables():
    return np.stack([xtable("dst", 0.5 * i) for i in range(GROUP_N)])


def group_meshes(small, other, i):
    """Frame i of the fused groups: (dst's drawn mesh and table, src's) -- dst through a transform table per frame, src
    skinned with a palette per frame under SRC_AT."""
    import tiny_renderer_amd as T
    pos, nrm = T.transform_mesh(small, group_tables()[i])
    base, _ = host_posed("xform", "dst", small, 0)     # (the indices: the same two entries)
    return (dict(base, pos=pos, nrm=nrm), None), (T.skin_mesh(other, *rig2(other), group_palettes()[i]), SRC_AT)


# ------------------------------------------------------------------------------------------------------------------
# References, computed once per session and left alone
# ------------------------------------------------------------------------------------------------------------------

_REF = {}


def reference(small, other, W, Hh=HH, band=None, pipe="phong", tap=False):
    """The plain pair's own frames and their merge, from twin scenes that are never merged.  flags: dst's colour-clean
    flags before the merge; shadow: dst's shadow view and bits."""
    key = (W, Hh, band, pipe, tap)
    if key not in _REF:
        kw = {} if band is None else {"band_rows": band}
        d, s = scene(W, Hh, small, pipe, DST_AT, tap, **kw), scene(W, Hh, other, "phong", SRC_AT, tap, **kw)
        drive(d), drive(s, light=SRC_LIGHT)
        flags = clean_flags(d)
        fd, fs = snap(d), snap(s)
        want, wins = merge(fd, fs, 1000)
        out = {"fd": fd, "fs": fs, "want": want, "wins": wins, "flags": flags, "shadow": d.get_shadow_buffer(),
               "shadow_bits": bits(d.read_shadow_f32())}
        opened, shared, clean = tile_sets(fd, fs, band)
        assert opened.any() and shared.any() and clean.any(), "the case is vacuous"
        d.close(), s.close()
        for v in out.values():
            for a in (v.values() if isinstance(v, dict) else [v]):
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
        _REF[key] = out
    return _REF[key]


def plain_pair(small, other, W, Hh=HH, store_depth=False, band=None, pipe="phong", tap=False, **kw):
    if band is not None:
        kw["band_rows"] = band
    d = scene(W, Hh, small, pipe, DST_AT, tap, store_depth=store_depth, **kw)
    kw.pop("frame_buffer_device", None)
    return d, scene(W, Hh, other, "phong", SRC_AT, tap, store_depth=store_depth, **kw)


def read_into(s, P):
    s.get_frame_buffer_async(P)
    assert s.sync() == 0


# ------------------------------------------------------------------------------------------------------------------
# C. The design of the cases, on the CPU
# ------------------------------------------------------------------------------------------------------------------

def _oracle(W, Hh, mesh, texs, cam=0.3, light=0.7, band=None, pipe="phong"):
    from oracle import oracle as O
    s = O.Scene(W, Hh, mesh, texs, pipe)
    if band is not None:
        s.set_output_band(*band)
    s.clear(), s.set_light_direction(H.light(light)), s.set_camera(*H.camera(cam)), s.render()
    out = {"fb": s.get_frame_buffer(), "z": s.z_f32(), "win": None}
    s.close()
    return out


def _oracle_p(W, Hh, mesh, texs, q):
    from oracle import oracle as O
    s = O.Scene(W, Hh, mesh, texs, "phong")
    s.clear(), s.set_light_direction(q[0:3]), s.set_camera(q[3:6], q[6:9], q[9:12]), s.render()
    out = {"fb": s.get_frame_buffer(), "z": s.z_f32(), "win": None}
    s.close()
    return out


def _assert_sets(name, fd, fs, band=None, shared=True):
    o, sh, c = tile_sets(fd, fs, band)
    assert o.any(), name + ": src opens no tile that dst left clean"
    assert sh.any() or not shared, name + ": no tile in which both win a pixel"
    assert c.any(), name + ": no tile stays clean on both sides"


def _differ(name, a, b, least=200):
    nz = int((bits(a["z"]) != bits(b["z"])).sum())
    nc = int((a["fb"] != b["fb"]).any(-1).sum())
    assert nz >= least and nc >= least, "%s: the poses differ in %d pixels of z, %d of rgb" % (name, nz, nc)


def test_every_case_has_the_tiles_it_is_about(built, small_synthetic):
    """With the oracle alone: every GPU case below has a tile src opens in dst, a tile both win pixels in and a tile
    clean on both sides, inside its band; the poses of cases 7 and 8 differ in at least 200 pixels of z and of rgb; the
    read-back orbit has tiles that fill and tiles that empty, and tiles that keep the caller's scribble unless
    host_buffer_written makes dst's record of the buffer lapse.  (0.2 s, after 0.5 s for its fixtures.)"""
    import tiny_renderer_amd as T
    small = small_synthetic
    other = T.synthetic_scene(n_lat=9, n_lon=17, tex_size=128, radius=0.75)
    plain_d, plain_s = drawn_mesh(None, "dst", small[0], 0), drawn_mesh(None, "src", other[0], 0)
    # cases 1, 2, 3, 5: the plain pair at every width; 1 and 4: the bands
    frames = {}
    for W in WIDTHS:
        fd, fs = _oracle(W, HH, plain_d, small[1]), _oracle(W, HH, plain_s, other[1], light=SRC_LIGHT)
        frames[W] = (fd, fs)
        _assert_sets("plain %d" % W, fd, fs)
        # case 2: dst alone -> merged fills a tile, merged -> dst alone empties it
        lit_d, lit_m = lit_tiles(fd["fb"]), lit_tiles(merge(fd, fs)[0]["fb"])
        assert (~lit_d & lit_m).any(), "no tile fills from frame one to frame two of the orbit"
        assert (lit_m & ~lit_d).any(), "no tile empties from frame two to frame three"
        # ... and the scribble before M*: some tile keeps it unless host_buffer_written makes the scene's record lapse
        clean = {"A": ~tiles_any(covered(fd)), "M": ~tiles_any(covered(fd) | covered(fs)), "S": ~tiles_any(covered(fs))}
        assert not (clean["M"] & lit_m).any() and not (clean["A"] & lit_d).any()
        n_starred = 0
        for orbit in sorted(ORBITS):
            for left in scribble_survivors(orbit, clean):
                n_starred += 1
                assert left.any(), "%s at %d: every scribbled tile is rewritten whatever the record says" % (orbit, W)
        assert n_starred == 2
        # case 5: merged into a pending clear, src's tiles against dst's earlier frame in the host buffer
        empty = {"fb": np.zeros_like(fd["fb"]), "z": np.full_like(fd["z"], F32_MIN_BITS.view(np.float32)), "win": None}
        _assert_sets("pending clear %d" % W, empty, fs, shared=False)
        assert (~lit_d & lit_tiles(fs["fb"])).any(), "src lights no tile that dst's earlier frame left as zeros in the host buffer"
    for band in ((0, 64), (64, 128)):
        _assert_sets("band pair %r" % (band,), *frames[208], band=band)
    W, Hh, band = BAND
    fd, fs = _oracle(W, Hh, plain_d, small[1], band=band), _oracle(W, Hh, plain_s, other[1], light=SRC_LIGHT, band=band)
    _assert_sets("band", fd, fs, band)
    fd = _oracle(208, HH, plain_d, small[1], pipe="shadow")
    _assert_sets("shadow dst", fd, frames[208][1])
    # case 1's shared host buffer: the small scene leaves tiles clean that the resolved merge lights
    fq = _oracle(128, HH // 2, T.apply_instances(small[0], SMALL_AT), small[1])
    half = box(merge(*frames[256])[0]["fb"], 2)
    assert (~lit_tiles(fq["fb"]) & lit_tiles(half)).any() and lit_tiles(fq["fb"]).any()
    # cases 6, 7: every kind on either side, both poses
    for kind, role in itertools.product(KINDS, ("src", "dst")):
        mesh, texs = (other if role == "src" else small)
        f = [_oracle(208, HH, drawn_mesh(kind, role, mesh, k), texs) for k in (0, 1)]
        _differ("%s %s" % (kind, role), f[0], f[1])
        for k in (0, 1):
            pair = (frames[208][0], f[k]) if role == "src" else (f[k], frames[208][1])
            _assert_sets("%s %s pose %d" % (kind, role, k), *pair)
    # case 8: four frames, each pair, and consecutive poses
    p = frame_params(GROUP_N)
    pairs = []
    for i in range(GROUP_N):
        (md, _), (ms, at) = group_meshes(small[0], other[0], i)
        pairs.append((_oracle_p(GROUP_W, HH, md, small[1], p[i]), _oracle_p(GROUP_W, HH, T.apply_instances(ms, at), other[1], p[i])))
        _assert_sets("group frame %d" % i, *pairs[-1])
    for i, j in itertools.combinations(range(GROUP_N), 2):
        _differ("group dst %d %d" % (i, j), pairs[i][0], pairs[j][0])
        _differ("group src %d %d" % (i, j), pairs[i][1], pairs[j][1])
    # ... and what a repeat under ANOTHER frame's pose but the frame's own camera would draw differs too
    for j in range(GROUP_N):
        (md, _), (ms, at) = group_meshes(small[0], other[0], j)
        for i in range(GROUP_N):
            if i != j:
                _differ("group dst %d, pose %d" % (i, j), pairs[i][0], _oracle_p(GROUP_W, HH, md, small[1], p[i]))
                _differ("group src %d, pose %d" % (i, j), pairs[i][1], _oracle_p(GROUP_W, HH, T.apply_instances(ms, at), other[1], p[i]))
    # case 9: the layers
    f1 = _oracle(208, HH, drawn_mesh("skin", "src", other[0], 0), other[1])
    f2 = _oracle(208, HH, T.apply_instances(other[0], AT3), other[1], cam=0.1)
    _assert_sets("layer one", frames[208][0], f1)
    m1, w1 = merge(frames[208][0], f1)
    m2, w2 = merge(m1, f2)
    on_top = _oracle(208, HH, plain_d, small[1], cam=-0.6)
    assert w1.any() and w2.any() and merge(m2, on_top)[1].any()


# ------------------------------------------------------------------------------------------------------------------
# A. Consumers of dst's flags after a merge
# ------------------------------------------------------------------------------------------------------------------

def _resolve_targets(d):
    import torch
    n = {f: (d.height // f) * (d.width // f) * 3 for f in FACTORS}
    dev = {f: torch.full((n[f] + 16,), 0xAA, dtype=torch.uint8, device="cuda") for f in FACTORS}
    pin = {f: d.pinned_resolved(f) for f in FACTORS}
    for f in FACTORS:
        pin[f][...] = 0xAA
    torch.cuda.synchronize()
    return n, dev, pin


def _check_resolved(d, fb, targets, word):
    import torch
    n, dev, pin = targets
    for f in FACTORS:
        assert np.array_equal(d.resolve(f), box(fb, f)), "%s: get_resolved, factor %d" % (word, f)
        d.resolve_into(f, dev[f].data_ptr())
        d.resolve_into(f, pin[f])
    assert d.sync() == 0
    torch.cuda.synchronize()
    for f in FACTORS:
        want = box(fb, f)
        host = dev[f].cpu().numpy()
        assert np.array_equal(host[:n[f]].reshape(want.shape), want), "%s: device target, factor %d" % (word, f)
        assert (host[n[f]:] == 0xAA).all()
        assert np.array_equal(pin[f], want), "%s: page-locked target, factor %d" % (word, f)


@pytest.mark.gpu
@BOTH
@pytest.mark.parametrize("W", WIDTHS)
@pytest.mark.parametrize("order", ["after", "before_and_after"])
def test_resolve_of_a_merged_frame(small_synthetic, other_synthetic, order, W, store_depth):
    """Case 1.  The tiles src opened must be READ by k_resolve; with a resolve of dst's own frame in the same targets
    first, nothing of it may survive the merge."""
    ref = reference(small_synthetic, other_synthetic, W)
    assert not np.array_equal(box(ref["fd"]["fb"], 8), box(ref["want"]["fb"], 8))
    d, s = plain_pair(small_synthetic, other_synthetic, W, store_depth=store_depth)
    targets = _resolve_targets(d)
    drive(d)
    if order == "before_and_after":
        _check_resolved(d, ref["fd"]["fb"], targets, "before the merge")
    drive(s, light=SRC_LIGHT)
    d.composite(s)
    _check_resolved(d, ref["want"]["fb"], targets, "after the merge")
    same(snap(d), ref["want"])
    d.close(), s.close()


@pytest.mark.gpu
@BOTH
def test_resolve_of_a_merged_frame_in_a_callers_buffer(small_synthetic, other_synthetic, store_depth):
    import torch
    W, guard = 208, 48
    ref = reference(small_synthetic, other_synthetic, W)
    buf = torch.full((guard + W * HH * 3 + guard,), 0xAA, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    d, s = plain_pair(small_synthetic, other_synthetic, W, store_depth=store_depth, frame_buffer_device=buf.data_ptr() + guard)
    targets = _resolve_targets(d)
    drive(d)
    _check_resolved(d, ref["fd"]["fb"], targets, "before the merge")
    drive(s, light=SRC_LIGHT)
    d.composite(s)
    _check_resolved(d, ref["want"]["fb"], targets, "after the merge")
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert np.array_equal(host[guard:guard + W * HH * 3].reshape(HH, W, 3), ref["want"]["fb"])
    assert (host[:guard] == 0xAA).all() and (host[guard + W * HH * 3:] == 0xAA).all()
    d.close(), s.close()


@pytest.mark.gpu
@BOTH
def test_band_pairs_merge_and_resolve_into_one_buffer(small_synthetic, other_synthetic, store_depth):
    import torch
    W = 208
    ref = reference(small_synthetic, other_synthetic, W)
    out = {f: torch.full((HH // f, W // f, 3), 0xAA, dtype=torch.uint8, device="cuda") for f in FACTORS}
    torch.cuda.synchronize()
    for band in ((0, 64), (64, 128)):
        d, s = plain_pair(small_synthetic, other_synthetic, W, store_depth=store_depth, band=band)
        drive(d)
        for f in FACTORS:
            d.resolve_into(f, out[f].data_ptr())     # dst's own band first: the merge must replace it
        drive(s, light=SRC_LIGHT)
        d.composite(s)
        for f in FACTORS:
            d.resolve_into(f, out[f].data_ptr())
        assert d.sync() == 0
        own = d.resolve(2)                           # the synchronous getter: the band's rows, zeros elsewhere
        r0, r1 = band[0] // 2, band[1] // 2
        want = box(ref["want"]["fb"], 2)
        assert np.array_equal(own[r0:r1], want[r0:r1]) and not own[:r0].any() and not own[r1:].any()
        d.close(), s.close()
    torch.cuda.synchronize()
    for f in FACTORS:
        assert np.array_equal(out[f].cpu().numpy(), box(ref["want"]["fb"], f)), "factor %d" % f


@pytest.mark.gpu
def test_resolve_into_a_page_locked_buffer_another_scene_reads_back_into(small_synthetic, other_synthetic):
    """Case 1, the host side: a small scene streams its frame into a page-locked buffer and remembers which tiles of it
    hold zeros; dst then resolves its merged frame into that buffer.  The small scene's record has lapsed: its next
    read-back must write every tile."""
    W = 256
    ref = reference(small_synthetic, other_synthetic, W)
    half = box(ref["want"]["fb"], 2)
    q = scene(W // 2, HH // 2, small_synthetic, "phong", SMALL_AT)
    drive(q)
    fq = q.get_frame_buffer()
    assert (~lit_tiles(fq) & lit_tiles(half)).any() and fq.any()
    d, s = plain_pair(small_synthetic, other_synthetic, W)
    R = d.pinned_resolved(2)
    R[...] = 0x99
    for rep in range(2):
        drive(q)
        read_into(q, R)
        assert np.array_equal(R, fq), "round %d: the small scene's frame" % rep
        read_into(q, R)
        assert np.array_equal(R, fq)
        drive(d), drive(s, light=SRC_LIGHT)
        d.composite(s)
        d.resolve_into(2, R)
        assert d.sync() == 0
        assert np.array_equal(R, half), "round %d: the resolved merge" % rep
        read_into(q, R)
        assert np.array_equal(R, fq), "round %d: the small scene's frame over the resolved merge" % rep
    q.close(), d.close(), s.close()


# (who reads back, what dst's frame is -- A: dst alone, M: the merge, M*: the merge again after the caller scribbled on the
# WHOLE buffer and said so, S: src's own frame --, into which buffer)
ORBITS = {
    "one_buffer": (("d", "A", 0), ("d", "M", 0), ("d", "A", 0), ("d", "M", 0), ("d", "M*", 0)),
    "two_buffers": (("d", "A", 0), ("d", "M", 1), ("d", "M", 0), ("d", "A", 1), ("d", "A", 0), ("d", "M", 1), ("d", "M*", 0),
                    ("d", "A", 1)),
    "src_in_between": (("d", "A", 0), ("s", "S", 0), ("d", "M", 0), ("d", "A", 0), ("s", "S", 0), ("s", "S", 0), ("d", "M", 0),
                       ("d", "M", 0), ("s", "S", 0), ("d", "A", 0)),
}
SCRIBBLE = 55


def scribble_survivors(orbit, clean):
    """Per M* step of the orbit: the tiles of the buffer that k_read_back would leave alone if the caller's word
    (host_buffer_written) were lost -- clean in the frame read back now AND in the frame dst put into that buffer before
    (nobody else having written it since), so dst's record of the buffer says "zeros" for them.  The scribble covers the
    whole buffer, so each of them holds it.  clean: {"A", "M", "S"} -> [tiles_y, tiles_x], no pixel of the tile drawn."""
    out, known = [], {}     # known: buffer -> tiles dst's record calls zeros (None: no record, every tile travels)
    for who, what, k in ORBITS[orbit]:
        if what == "M*":
            out.append(np.zeros_like(clean["M"]) if known.get(k) is None else known[k] & clean["M"])
        known[k] = None if who == "s" else clean[what[0]]
    return out


@pytest.mark.gpu
@BOTH
@pytest.mark.parametrize("W", WIDTHS)
@pytest.mark.parametrize("orbit", sorted(ORBITS))
def test_sparse_read_back_of_merged_frames(small_synthetic, other_synthetic, orbit, W, store_depth):
    """Case 2.  The page-locked buffer's record says "zeros" for the tiles dst left empty; the merge opens some of them
    behind the scene's back, a later frame of dst alone empties them again.  Every byte of every read-back."""
    ref = reference(small_synthetic, other_synthetic, W)
    frames = {"A": ref["fd"]["fb"], "M": ref["want"]["fb"], "M*": ref["want"]["fb"], "S": ref["fs"]["fb"]}
    assert (~lit_tiles(frames["A"]) & lit_tiles(frames["M"])).any()
    d, s = plain_pair(small_synthetic, other_synthetic, W, store_depth=store_depth)
    P = [d.pinned_frame() for _ in range(2)]
    for b in P:
        b[...] = 99               # unknown content to begin with
    drive(s, light=SRC_LIGHT)
    state = None
    for step, (who, what, k) in enumerate(ORBITS[orbit]):
        if what == "S":
            read_into(s, P[k])
        else:
            if what == "A" or (what == "M" and state != "A"):
                drive(d)
            if what == "M":
                d.composite(s)
            if what == "M*":
                P[k][...] = SCRIBBLE      # (every tile: also those the frame and the scene's record both call zeros)
                d.host_buffer_written(P[k])
            state = what[0]
            read_into(d, P[k])
        got, want = P[k], frames[what]
        assert np.array_equal(got, want), "step %d (%s %s): %d pixels differ" % (step, who, what, int((got != want).any(-1).sum()))
    same(snap(s), ref["fs"])
    d.close(), s.close()


GETTERS = ("z_view", "frame", "winner", "shadow_view", "resolve")
GETTER_ORDERS = ((0, 1, 2, 3, 4), (4, 3, 2, 1, 0), (2, 4, 0, 3, 1))


@pytest.mark.gpu
@BOTH
@pytest.mark.parametrize("order", GETTER_ORDERS, ids=["".join(map(str, o)) for o in GETTER_ORDERS])
def test_getters_of_every_kind_in_every_order(small_synthetic, other_synthetic, order, store_depth):
    """Case 3.  A shadow dst with taps on both: whichever getter comes first finds the flags the merge left."""
    W = 208
    ref = reference(small_synthetic, other_synthetic, W, pipe="shadow", tap=True)
    want = ref["want"]
    assert (want["win"] >= 1000).any() and (want["win"] < 1000).any()
    d, s = plain_pair(small_synthetic, other_synthetic, W, store_depth=store_depth, pipe="shadow", tap=True)
    drive(d), drive(s, light=SRC_LIGHT)
    d.composite(s, winner_base=1000)
    for g in order:
        name = GETTERS[g]
        if name == "z_view":
            assert np.array_equal(d.get_z_buffer(), grey(want["z"])), name
        elif name == "frame":
            assert np.array_equal(d.get_frame_buffer(), want["fb"]), name
        elif name == "winner":
            assert np.array_equal(d.read_winner_u32(), want["win"]), name
        elif name == "shadow_view":
            assert np.array_equal(d.get_shadow_buffer(), ref["shadow"]), name
        else:
            assert np.array_equal(d.resolve(2), box(want["fb"], 2)), name
    same(snap(d), want)
    assert np.array_equal(bits(d.read_shadow_f32()), ref["shadow_bits"])
    d.close(), s.close()


@pytest.mark.gpu
@BOTH
def test_band_tiles_after_a_merge(small_synthetic, other_synthetic, store_depth):
    """Case 4.  What the sparse tile push would send by: a tile whose flag is up is all zeros in dst's frame buffer, and
    the flags that came down are those of the clean tiles in which a pixel won."""
    W, Hh, band = BAND
    ref = reference(small_synthetic, other_synthetic, W, Hh, band)
    d, s = plain_pair(small_synthetic, other_synthetic, W, Hh, store_depth, band)
    drive(d), drive(s, light=SRC_LIGHT)
    d.composite(s)
    flags = clean_flags(d)
    t = d.band_tiles()
    rows = slice(t.first_tile_row, t.first_tile_row + t.tiles_y)
    assert (t.band_y0, t.band_y1) == band_y(Hh, band) and flags.shape == (t.tiles_y, t.tiles_x)
    won = tiles_any(ref["wins"])[rows]
    before = ~tiles_any(covered(ref["fd"]))[rows]    # clean before the merge: the tiles in which dst drew no pixel
    assert np.array_equal(ref["flags"], before), "the un-merged twin's own flags"
    assert (before & won).any() and (before & ~won).any() and (~before & won).any()
    assert int((before & ~flags).sum()) == int((before & won).sum()) and not (flags & ~before).any()
    assert np.array_equal(flags, before & ~won)
    fb = d.get_frame_buffer()
    assert not (lit_tiles(fb)[rows] & flags).any(), "a tile flagged clean holds colour"
    # the exchange's view: a flagged tile travels as zeros, the others as they are
    rebuilt = fb[::-1].copy()
    for ty, tx in zip(*np.nonzero(flags)):
        y0 = (t.first_tile_row + ty) * 16
        rebuilt[y0:y0 + 16, tx * 128:tx * 128 + 128] = 0
    y0, y1 = band_y(Hh, band)
    assert np.array_equal(rebuilt[y0:y1], ref["want"]["fb"][::-1][y0:y1])
    same(snap(d), ref["want"], band_y(Hh, band))
    d.close(), s.close()


@pytest.mark.gpu
@BOTH
@pytest.mark.parametrize("W", WIDTHS)
def test_merge_into_a_pending_clear_then_consumers(small_synthetic, other_synthetic, W, store_depth):
    """Case 5.  dst.clear() without a render, the merge, then resolve and a sparse read-back into a buffer that holds
    dst's earlier frame: src's frame where src drew, zeros elsewhere; z is src's or f32::MIN."""
    ref = reference(small_synthetic, other_synthetic, W)
    fs = ref["fs"]
    d, s = plain_pair(small_synthetic, other_synthetic, W, store_depth=store_depth)
    P = d.pinned_frame()
    P[...] = 99
    drive(d)
    read_into(d, P)
    assert np.array_equal(P, ref["fd"]["fb"])
    drive(s, light=SRC_LIGHT)
    d.clear()
    d.composite(s)
    assert np.array_equal(d.resolve(2), box(fs["fb"], 2))
    read_into(d, P)
    assert np.array_equal(P, fs["fb"]), "%d pixels differ" % int((P != fs["fb"]).any(-1).sum())
    assert np.array_equal(d.get_z_buffer(), grey(fs["z"]))
    same(snap(d), {"fb": fs["fb"], "z": fs["z"], "win": None})
    d.close(), s.close()


# ------------------------------------------------------------------------------------------------------------------
# B. Posed, instanced and kept sources and destinations
# ------------------------------------------------------------------------------------------------------------------

def _sides(small, other, kind, role, pipe, tap, W=208, k=0, texs=None):
    """(dst, src) with `role` posed on the device, and their twins of host meshes.  texs: one set of images for both
    (what the oracle of a concatenated mesh needs)."""
    small = small if texs is None else (small[0], texs)
    other = other if texs is None else (other[0], texs)
    out = []
    for make in (posed_scene, twin_scene):
        kd, ks = (kind, None) if role == "dst" else (None, kind)
        d = (make if kd else twin_scene)(W, HH, kd, "dst", small, pipe, k, tap)
        s = (make if ks else twin_scene)(W, HH, ks, "src", other, pipe, k, tap)
        out.append((d, s))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("role", ["src", "dst"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("pipe,tap", [("phong", False), ("darboux", False), ("specular", False), ("phong", True), ("darboux", True),
                                      ("specular", True)],
                         ids=["phong-transient", "darboux-transient", "specular-transient", "phong", "darboux", "specular"])
def test_posed_scene_merges_like_a_scene_of_the_posed_mesh(small_synthetic, other_synthetic, pipe, tap, kind, role):
    """Case 6.  Without the tap the depth of both sides is transient: the merge repeats each pipeline's last pass for
    depth alone, pose and all (under the tap a pass never defers its depth).  Frame and z against the twins' merge and the
    oracle of the concatenated host-posed mesh; with taps the winners too, winner_base = n_tri(dst)."""
    texs = small_synthetic[1]
    (d, s), (td, ts) = _sides(small_synthetic, other_synthetic, kind, role, pipe, tap, texs=texs)
    md = drawn_mesh(kind if role == "dst" else None, "dst", small_synthetic[0], 0)
    ms = drawn_mesh(kind if role == "src" else None, "src", other_synthetic[0], 0)
    n_d = np.asarray(md["idx"]).reshape(-1, 9).shape[0]
    for q in (d, s, td, ts):
        drive(q)
    want, wins = merge(snap(td), snap(ts), n_d)
    assert wins.any() and (covered(snap(ts)) & ~wins).any()
    d.composite(s, winner_base=n_d)
    got = snap(d)
    same(got, want)
    cpu = oracle_frame(208, HH, concat(md, ms), texs, pipe)
    if not tap:
        cpu["win"] = None
    else:
        assert (cpu["win"] >= n_d).any() and (cpu["win"] < n_d).any()
    same(got, cpu)
    same(snap(s), snap(ts))
    for q in (d, s, td, ts):
        q.close()


@pytest.mark.gpu
@pytest.mark.parametrize("role", ["src", "dst"])
@pytest.mark.parametrize("kind", KINDS)
def test_the_merge_draws_the_frames_pose_not_the_current_one(small_synthetic, other_synthetic, kind, role):
    """Case 7.  Pose 0 is rendered, pose 1 set without a render, then the merge: depth and colour are pose 0's.  The
    scene's current pose is still pose 1 afterwards."""
    (d, s), (td, ts) = _sides(small_synthetic, other_synthetic, kind, role, "phong", False)
    for q in (d, s, td, ts):
        drive(q)
    f_td, f_ts = snap(td), snap(ts)
    want, wins = merge(f_td, f_ts)
    assert wins.any()
    posed = d if role == "dst" else s
    set_pose(posed, kind, role, 1)
    d.composite(s)
    same(snap(d), want)
    same(snap(s), f_ts)
    # ... and pose 1 is what the next cleared render draws
    later = twin_scene(208, HH, kind, role, small_synthetic if role == "dst" else other_synthetic, "phong", 1)
    drive(posed), drive(later)
    f_later = snap(later)
    assert not np.array_equal(f_later["fb"], (f_td if role == "dst" else f_ts)["fb"])
    same(snap(posed), f_later)
    for q in (d, s, td, ts, later):
        q.close()


def _group_reference(small, other):
    key = "group"
    if key not in _REF:
        p = frame_params(GROUP_N)
        frames = []
        for i in range(GROUP_N):
            (md, at_d), (ms, at_s) = group_meshes(small[0], other[0], i)
            td, ts = scene(GROUP_W, HH, (md, small[1]), "phong", at_d), scene(GROUP_W, HH, (ms, other[1]), "phong", at_s)
            _frame_p(td, p[i]), _frame_p(ts, p[i])
            fd, fs = snap(td), snap(ts)
            want, wins = merge(fd, fs)
            assert wins.any() and (covered(fs) & ~wins).any()
            frames.append({"fd": fd, "fs": fs, "want": want})
            td.close(), ts.close()
        _REF[key] = frames
    return _REF[key]


def _group_scenes(small, other, **kw):
    d = scene(GROUP_W, HH, small, "phong", None, instance_transforms=group_tables()[0], **kw)
    s = scene(GROUP_W, HH, other, "phong", SRC_AT, **kw)
    s.set_skin(*rig2(other[0]), n_bones=2)
    return d, s


@pytest.mark.gpu
@pytest.mark.parametrize("another_pose", [False, True], ids=["selected_pose_current", "another_pose_current"])
def test_kept_frames_of_fused_groups_with_a_pose_per_frame(small_synthetic, other_synthetic, another_pose):
    """Case 8.  Four frames by one launch on either side, src with a palette per frame, dst with a transform table per
    frame; kept frames selected out of order and merged: the repeat for depth must draw the selected frame's pose, whose
    rows must still be alive.  another_pose: after the selection the scenes are given ANOTHER frame's pose as their current
    one (no render): the merge must still draw the selected frame's."""
    ref = _group_reference(small_synthetic, other_synthetic)
    p = frame_params(GROUP_N)
    d, s = _group_scenes(small_synthetic, other_synthetic, frames_per_launch=4)
    d.render_frames(p, instance_transforms=group_tables())
    s.render_frames(p, bone_palettes=group_palettes())
    assert d.frames_kept() == GROUP_N and s.frames_kept() == GROUP_N
    for back in SELECT_ORDER:
        d.select_frame(back), s.select_frame(back)
        if another_pose:    # (frame GROUP_N - 1 - back is selected: pose `back` is never its own)
            d.set_instance_transforms(group_tables()[back]), s.set_bone_palette(group_palettes()[back])
        d.composite(s)
        same(snap(d), ref[GROUP_N - 1 - back]["want"])
        assert GROUP_N <= s.debug_morph_rows() <= GROUP_ROWS    # (every kept frame's rows are alive: at least GROUP_N)
    for back in range(GROUP_N):     # src's frames are what they were, dst's are the merges
        d.select_frame(back), s.select_frame(back)
        same(snap(s), ref[GROUP_N - 1 - back]["fs"])
        same(snap(d), ref[GROUP_N - 1 - back]["want"])
    assert GROUP_N <= s.debug_morph_rows() <= GROUP_ROWS and d.debug_morph_rows() <= GROUP_ROWS
    d.close(), s.close()


@pytest.mark.gpu
def test_held_back_frames_with_a_pose_each_then_a_merge_without_a_sync(small_synthetic, other_synthetic):
    """Case 8 through the automatic groups: per-frame calls with a new palette / table before each render, then the
    merge at once; and the same with yet another pose set (not rendered) before the merge."""
    ref = _group_reference(small_synthetic, other_synthetic)
    p = frame_params(GROUP_N)
    for set_another in (False, True):
        d, s = _group_scenes(small_synthetic, other_synthetic)
        assert d.frames_per_launch > 1 and s.frames_per_launch > 1
        for i in range(GROUP_N):
            d.set_instance_transforms(group_tables()[i]), s.set_bone_palette(group_palettes()[i])
            _frame_p(d, p[i]), _frame_p(s, p[i])
        if set_another:
            d.set_instance_transforms(group_tables()[0]), s.set_bone_palette(group_palettes()[0])
        d.composite(s)
        same(snap(d), ref[GROUP_N - 1]["want"])
        same(snap(s), ref[GROUP_N - 1]["fs"])
        assert 0 < s.debug_morph_rows() <= GROUP_ROWS
        d.close(), s.close()


@pytest.mark.gpu
@BOTH
@pytest.mark.parametrize("first", ["skinned_first", "skinned_last"])
def test_layers_with_a_skinned_one_then_a_render_on_top_then_resolve(small_synthetic, other_synthetic, first, store_depth):
    """Case 9.  Three scenes, one skinned, merged in either order into a plain dst; dst renders without a clear on top
    (it depth-tests against the merged z); the result is resolved."""
    W = 208

    def make(twin):
        d = scene(W, HH, small_synthetic, "phong", DST_AT, store_depth=store_depth)
        s1 = (twin_scene if twin else posed_scene)(W, HH, "skin", "src", other_synthetic, "phong", 0, store_depth=store_depth)
        s2 = scene(W, HH, other_synthetic, "normal_map", AT3, store_depth=store_depth)
        return d, s1, s2

    def frames(d, s1, s2):
        drive(d), drive(s1), drive(s2, cam=0.1)

    d, s1, s2 = make(True)
    frames(d, s1, s2)
    f0, f1, f2 = snap(d), snap(s1), snap(s2)
    drive(d, cam=-0.6)
    on_top = snap(d)
    layers = (f1, f2) if first == "skinned_first" else (f2, f1)
    m1, w1 = merge(f0, layers[0])
    m2, w2 = merge(m1, layers[1])
    m3, w3 = merge(m2, on_top)
    assert w1.any() and w2.any() and w3.any()
    for q in (d, s1, s2):
        q.close()
    d, s1, s2 = make(False)
    frames(d, s1, s2)
    for q in ((s1, s2) if first == "skinned_first" else (s2, s1)):
        d.composite(q)
    drive(d, cam=-0.6, clear=False)
    assert np.array_equal(d.resolve(2), box(m3["fb"], 2))
    same(snap(d), m3)
    assert np.array_equal(d.resolve(4), box(m3["fb"], 4))
    for q in (d, s1, s2):
        q.close()
