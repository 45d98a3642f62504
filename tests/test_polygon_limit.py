"""Passes at and past 2^20 polygons.  The shared-bin tile kernels (k_tile, SHARED -- csrc/tr_kernels.hip) break depth ties
by a 32-bit word, (2^20 - 1 - polygon id) << 12 | bin slot + 1; a pass of more than 2^20 polygons -- mesh polygons x
instances -- must run the column kernels instead, decided alike in tile_layout (which also tells k_setup what to prepare),
launch_tile and tile_launch_is_interior.  A 512-polygon mesh under tables of 2047, 2048, 2049 and 2050 entries stands
2^20 - 512, 2^20, 2^20 + 512 and 2^20 + 1024 polygons; nearly every entry is off screen, so a frame is one k_setup sweep
over 10^6 rows and a handful of small spheres.  Two of the spheres on screen are bit-identical TWINS: every pixel they
cover is an exact z tie, which the lower polygon id must win -- below the limit (entries 5 and 6), straddling it (2046 and
2048) and above it (2048 and 2049).

The reference of every case is the CPU oracle on the host-concatenated mesh; rgb bytes, z bits, shadow bits and the
winner index are compared exactly.  No tolerance appears.  The design test (CPU) proves from the oracle alone that the
inputs are what they claim.

What the ABI does not offer, and what stands in its place here:
  * tr_scene_render_frames_instanced takes ONE table length for all its frames.  Frames whose tables differ in length meet
    in one fused group only as held-back frames (render after set_instances, nothing read in between): the mixed groups
    2047 / 2048 / 2049 / 2050 are formed that way, into the caller's buffers, and the profile proves the single launch.
  * tr_scene_select_frame reaches the frames of a render_frames call only, so held-back frames are compared through
    the buffers they were rendered into (rgb), the last one also through the scene's getters (z, shadow).
  * a pair of ids that both lie in [2^20, 2^21) keeps its order when the id field wraps (the shift drops bit 20 of both):
    only a tie ACROSS the limit can show a missing fallback in the winner; the pair above the limit guards the column
    kernels' own id compare and the 32-bit polygon arithmetic of the chain there.
  * twins of an offset/scale table are identical in colour too, so a fused frame (no winner tap) cannot show which of them
    won.  Two things stand in: the fused cases ask Scene.interior_tiles() for the form that ran wherever the layout makes
    it an observable (four pinned shared waves on these frames of whole tiles), and the TRANSFORM tables give the upper
    twin of the pair across the limit the same 3 x 4 but another normal matrix -- an exact z tie whose colour says who
    won, in every frame, tapped or not (xtab)."""
import numpy as np
import pytest

from tests import helpers as H
from tests.test_fused_parity import NO_WINNER, TWO_PASS, _tile_launches, assert_fused_parity, fused_pair, view
from tests.test_interior_tiles import TILE_H, TILE_W, VIEWS, render_kept
from tests.test_morph import POSE, _targets

LIMIT = 1 << 20                     # SHARED_MAX_POLYGONS, csrc/tr_kernels.hip
MAX_SLOTS = 4093                    # SHARED_MAX_SLOTS
ROWS = 512
ROLL = 268                          # rows of the 576-row sphere rotated by this: row 511 is the sphere's row 243, facing the camera
NS = (2047, 2048, 2049, 2050)
W, HH = 640, 480
CAM, LIGHT = 0.3, 0.7
Q = view(CAM, LIGHT)
SCALE = np.float32(0.3)
# places on screen (offset x, y): spheres of radius 0.24 that do not touch
PLACES = [(-0.7, -0.45), (-0.23, -0.45), (0.23, -0.45), (0.7, -0.45), (-0.7, 0.45), (-0.23, 0.45), (0.23, 0.45), (0.7, 0.45)]
TWINS = {"low": (5, 6), "straddle": (2046, 2048), "above": (2048, 2049)}
# the tables: (entries, twin pairs beside the low one)
TABLES = {"2047": (2047, ()), "2048": (2048, ()), "2049": (2049, ("straddle",)), "2050": (2050, ("straddle",)),
          "2050above": (2050, ("above",))}
LADDER_TABLES = tuple(TABLES)
LAYOUTS = {"auto": {}, "shared4": dict(tile_mode=2, tile_waves=4), "shared8": dict(tile_mode=2, tile_waves=8),
           "shared16": dict(tile_mode=2, tile_waves=16), "columns4": dict(tile_mode=1, tile_waves=4)}

_cache = {}


@pytest.fixture(scope="module", autouse=True)
def _release_cache():
    """The concatenated meshes (10^6 rows each) and the oracle's frames live as long as this module's tests, no longer."""
    yield
    _cache.clear()


def _memo(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def m512(mesh):
    """512 of the sphere's 576 rows, rotated so that the last one faces the test camera (asserted by the design test)."""
    return _memo("m512", lambda: dict(mesh, idx=np.ascontiguousarray(np.roll(np.asarray(mesh["idx"], np.uint32), ROLL, axis=0)[:ROWS])))


def placement(name):
    """entry -> place on screen: entry 0, the low twins, two in the middle, entry 2047 and the last entry where they exist
    and are no twin, the table's other twin pair."""
    n, pairs = TABLES[name]
    on = {0: 0, 5: 1, 6: 1, 700: 2, 1400: 3}
    for p in pairs:
        on[TWINS[p][0]] = on[TWINS[p][1]] = 6
    if n > 2047 and 2047 not in on:
        on[2047] = 4
    if n - 1 not in on:
        on[n - 1] = 5
    return n, pairs, on


def tab(name, without=None):
    """The offset/scale table: every entry off screen (x = 50 + 0.01 k, scale 0.3) but those of placement();
    without: that entry moved off screen too."""
    n, _, on = placement(name)
    t = np.zeros((n, 4), np.float32)
    t[:, 0] = np.float32(50.0) + np.float32(0.01) * np.arange(n, dtype=np.float32)
    t[:, 3] = SCALE
    for e, p in on.items():
        if e != without:
            t[e, 0:2] = PLACES[p]
    return t


TINT = 2.0   # the upper twin across the limit: its normals are those of an instance yawed by this much more (radians)


def xtab(name="2049", without=None):
    """The same shape as a transform table: scaled rotations.  Twins share a place and their angles, so their 3 x 4 --
    every position, every depth -- is bit-identical; the upper twin of the pair ACROSS the limit gets the normal matrix
    of another rotation: where it wins a tie it should lose, the colour shows it.  without: that entry off screen."""
    return _memo(("xtab", name, without), lambda: _xtab(name, without))


def _xtab(name, without):
    import tiny_renderer_amd as T
    n, pairs, on = placement(name)
    off = np.zeros((n, 3), np.float64)
    off[:, 0] = 50.0 + 0.01 * np.arange(n)
    k = np.arange(n)
    for e, p in on.items():
        if e != without:
            off[e, 0:2] = PLACES[p]
        k[e] = p       # (twins share a place, so they share their angles)
    t = T.rotation_instances(0.37 * k, 0.11 * k, 0.05 * k, off, np.full(n, 0.3))
    if "straddle" in pairs:
        lo, up = TWINS["straddle"]
        if without != lo:
            assert t[lo, 0:12].tobytes() == t[up, 0:12].tobytes()
        t[up, 12:21] = T.rotation_instances(0.37 * k[up] + TINT, 0.11 * k[up], 0.05 * k[up], off[up:up + 1], [0.3])[0, 12:21]
    return t


def _key(key):
    """(kind, table name, entry left out) of a cat() / oracle() key: a TABLES name, (name, without), "xform", "posed",
    or (kind, name, without)."""
    if isinstance(key, str):
        return ("tab", key, None) if key in TABLES else (key, "2049", None)
    return ("tab",) + tuple(key) if len(key) == 2 else tuple(key)


def cat(mesh, key):
    """The host-concatenated mesh of a table (key: see _key)."""
    import tiny_renderer_amd as T
    kind, name, without = _key(key)

    def make():
        m = m512(mesh)
        if kind == "xform":
            return T.apply_instance_transforms(m, xtab(name, without))
        if kind == "posed":
            pos, nrm = T.morph_mesh(m, *_targets(m), POSE)
            m = dict(m, pos=pos, nrm=nrm)
        return T.apply_instances(m, tab(name, without))
    return _memo(("cat", kind, name, without), make)


def oracle(small, key, pipe, q=Q, renders=1, size=(W, HH)):
    """The oracle's frame of cat(key): `renders` renders after one clear."""
    from oracle import oracle as O
    mesh, texs = small

    def make():
        cpu = O.Scene(size[0], size[1], cat(mesh, key), texs, pipe)
        cpu.clear()
        cpu.set_light_direction(q[0:3])
        cpu.set_camera(q[3:6], q[6:9], q[9:12])
        err = 0
        for _ in range(renders):
            err |= cpu.render()
        out = dict(err=err, rgb=cpu.get_frame_buffer(), z=cpu.z_f32().view(np.uint32), winner=cpu.winner_u32(),
                   shadow=cpu.shadow_f32().view(np.uint32) if pipe in TWO_PASS else None, tri_kept=cpu.stats()[0]["tri_kept"])
        cpu.close()
        return out
    return _memo(("oracle", _key(key), pipe, q.tobytes(), renders, size), make)


def grab(gpu, pipe, winner=False):
    out = dict(rgb=gpu.get_frame_buffer(), z=gpu.read_z_f32().view(np.uint32),
               shadow=gpu.read_shadow_f32().view(np.uint32) if pipe in TWO_PASS else None)
    if winner:
        out["winner"] = gpu.read_winner_u32()
    return out


def assert_frame(got, want, pipe, what=""):
    assert want["err"] == 0 and want["rgb"].any()
    assert np.array_equal(got["z"], want["z"]), "%s: z bits differ at %d pixels" % (what, int((got["z"] != want["z"]).sum()))
    if pipe in TWO_PASS:
        assert np.array_equal(got["shadow"], want["shadow"]), \
            "%s: shadow bits differ at %d pixels" % (what, int((got["shadow"] != want["shadow"]).sum()))
    if "winner" in got:
        bad = got["winner"] != want["winner"]
        assert not bad.any(), "%s: winner differs at %d pixels, first: polygon %d for %d" % (
            what, int(bad.sum()), int(got["winner"][bad][0]), int(want["winner"][bad][0]))
    assert np.array_equal(got["rgb"], want["rgb"]), "%s: rgb differs at %d pixels" % (what, int((got["rgb"] != want["rgb"]).any(-1).sum()))


def frame(s, q=Q, clear=True):
    if clear:
        s.clear()
    s.set_light_direction(q[0:3])
    s.set_camera(q[3:6], q[6:9], q[9:12])
    s.render()


# ---- CPU: the inputs are what they claim ----------------------------------------------------------------------------------

def test_expect_interior_counts_a_shared_mode_past_the_limit_as_columns():
    """The helper's new argument: without it, and up to 2^20 polygons, nothing changes for any caller; past them a shared
    mode counts as columns -- and only that: waves, frame and band still decide."""
    for n_poly in (None, 1, LIMIT - ROWS, LIMIT):
        for args in ((256, 32, "phong", 4, 1), (256, 32, "phong", 4, 2), (256, 32, "shadow", 8, 1), (255, 32, "phong", 4, 1),
                     (640, 480, "occlusion", 4, 1), (640, 480, "phong", 0, 0)):
            assert H.expect_interior(*args, n_poly=n_poly) == H.expect_interior(*args), (args, n_poly)
    assert not H.expect_interior(256, 32, "phong", 4, 2) and not H.expect_interior(256, 32, "phong", 4, 2, n_poly=LIMIT)
    assert H.expect_interior(256, 32, "phong", 4, 2, n_poly=LIMIT + 1) and H.expect_interior(256, 32, "shadow", 4, 2, n_poly=LIMIT + ROWS)
    assert H.expect_interior(256, 32, "phong", 4, 1, n_poly=LIMIT + ROWS)
    assert not H.expect_interior(256, 32, "phong", 0, 0, n_poly=LIMIT + ROWS)
    assert not H.expect_interior(256, 32, "phong", 8, 2, n_poly=LIMIT + ROWS)
    assert not H.expect_interior(255, 32, "phong", 4, 2, n_poly=LIMIT + ROWS)


def _largest_bin(win, hidden):
    """An upper bound of the records a 128 x 16 tile holds: 512 for every entry whose box on screen -- the box of its
    winners, two pixels wider (every polygon of a sphere projects inside its outline) -- meets the tile; a hidden upper
    twin has the box of its lower twin."""
    ys, xs = np.nonzero(win != NO_WINNER)
    entry = win[ys, xs] // ROWS
    tiles = np.zeros(((win.shape[0] + TILE_H - 1) // TILE_H, (win.shape[1] + TILE_W - 1) // TILE_W), np.int64)
    for e in np.unique(entry):
        x0, x1 = xs[entry == e].min() - 2, xs[entry == e].max() + 2
        y0, y1 = ys[entry == e].min() - 2, ys[entry == e].max() + 2
        tiles[max(y0, 0) // TILE_H:y1 // TILE_H + 1, max(x0, 0) // TILE_W:x1 // TILE_W + 1] += ROWS * (1 + hidden.get(int(e), 0))
    return int(tiles.max())


def test_design_holds(small_synthetic):
    """From the oracle alone: the frames are not empty, entry 0 and the last entry win pixels (a last entry that is an upper
    twin wins none, like every upper twin), polygon 2^20 - 1 wins pixels where it exists, every lower twin wins at least a
    thousand pixels and its upper twin none, the ties are real -- with the lower twin moved away the upper one wins exactly
    those pixels at bit-equal z -- and no tile comes near 4 093 records, in the camera's view and the light's."""
    mesh, _ = small_synthetic
    assert mesh["idx"].shape[0] == 576 and m512(mesh)["idx"].shape == (ROWS, 9)
    for name in TABLES:
        n, pairs, on = placement(name)
        assert cat(mesh, name)["idx"].shape[0] == n * ROWS
        o = oracle(small_synthetic, name, "phong")
        assert o["err"] == 0 and o["rgb"].any()
        win = o["winner"]
        won = np.bincount(win[win != NO_WINNER] // ROWS, minlength=n)
        assert set(np.nonzero(won)[0]) <= set(on), "an entry meant to be off screen is on it"
        uppers = {TWINS[p][1] for p in ("low",) + pairs}
        assert won[0] > 0 and (won[n - 1] > 0) == (n - 1 not in uppers)
        assert (win == n * ROWS - 1).any() == (n - 1 not in uppers), "the mesh's last row must face the camera"
        if n > 2047:
            assert (win == LIMIT - 1).sum() > 0, "polygon 2^20 - 1 wins no pixel"
        for p in ("low",) + pairs:
            lo, up = TWINS[p]
            assert won[lo] >= 1000 and won[up] == 0, (name, p, int(won[lo]), int(won[up]))
            alone = oracle(small_synthetic, (name, lo), "phong")
            at = (win // ROWS == lo) & (win != NO_WINNER)
            assert np.array_equal(alone["winner"][at], win[at] + np.uint32((up - lo) * ROWS)), "the twins are not identical"
            assert np.array_equal(alone["z"][at], o["z"][at]), "the twins' depths differ: no tie"
        hidden = {TWINS[p][0]: 1 for p in ("low",) + pairs}
        assert _largest_bin(win, hidden) <= MAX_SLOTS
        assert _largest_bin(oracle(small_synthetic, name, "phong", q=view(LIGHT, LIGHT))["winner"], hidden) <= MAX_SLOTS
    lo, up = TWINS["straddle"]
    for kind, name in [("posed", "2049")] + [("xform", x) for x in XNAMES]:
        n, pairs, _ = placement(name)
        o = oracle(small_synthetic, (kind, name, None), "phong")
        win = o["winner"]
        won = np.bincount(win[win != NO_WINNER] // ROWS, minlength=n)
        assert o["err"] == 0 and won[0] > 0, (kind, name)
        # (polygon 2^20 - 1: entry 2047 is turned like its place, and under the 2050 table its last row is behind its neighbour)
        assert (win == LIMIT - 1).any() or n in (2047, 2050), (kind, name)
        assert won[5] >= 1000 and won[6] == 0, (kind, name)
        assert _largest_bin(win, {5: 1, lo: 1}) <= MAX_SLOTS
        if "straddle" not in pairs:
            continue
        # the tie across the limit is a real one: without the lower twin the upper one wins exactly its pixels at bit-equal z ...
        assert won[lo] >= 1000 and won[up] == 0, (kind, name, int(won[lo]), int(won[up]))
        alone = oracle(small_synthetic, (kind, name, lo), "phong")
        at = (win // ROWS == lo) & (win != NO_WINNER)
        assert np.array_equal(alone["winner"][at], win[at] + np.uint32((up - lo) * ROWS)), "the twins are not identical"
        assert np.array_equal(alone["z"][at], o["z"][at]), "the twins' depths differ: no tie"
        # ... and under a transform table its colour says who won (identical under an offset/scale table)
        differ = int((alone["rgb"][::-1][at] != o["rgb"][::-1][at]).any(-1).sum())   # (frame rows from the top, buffer rows from the bottom)
        assert differ >= 1000 if kind == "xform" else differ == 0, (kind, name, differ)


# ---- GPU ------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("pipe", ["phong", "shadow"])
@pytest.mark.parametrize("name", LADDER_TABLES)
def test_ladder_across_the_limit(small_synthetic, name, pipe, layout):
    """Case 1: the per-frame kernels with the winner tap (MODE 0) under every layout, one table per step of the ladder."""
    import tiny_renderer_amd as T
    mesh, texs = small_synthetic
    gpu = T.Scene(W, HH, m512(mesh), texs, pipe, winner_tap=True, instances=tab(name), **LAYOUTS[layout])
    frame(gpu)
    assert_frame(grab(gpu, pipe, winner=True), oracle(small_synthetic, name, pipe), pipe, "%s %s %s" % (name, pipe, layout))
    gpu.close()


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["auto", "shared4", "columns4"])
@pytest.mark.parametrize("pipe", ["phong", "shadow"])
@pytest.mark.parametrize("name", ["2048", "2049"])
def test_plain_mesh_of_2_20_rows(small_synthetic, name, pipe, layout):
    """Case 1, second half: the concatenated mesh as a plain mesh -- no table, 2^20 and 2^20 + 512 rows."""
    import tiny_renderer_amd as T
    mesh, texs = small_synthetic
    gpu = T.Scene(W, HH, cat(mesh, name), texs, pipe, winner_tap=True, **LAYOUTS[layout])
    frame(gpu)
    assert_frame(grab(gpu, pipe, winner=True), oracle(small_synthetic, name, pipe), pipe, "plain %s %s %s" % (name, pipe, layout))
    gpu.close()


@pytest.mark.gpu
@pytest.mark.parametrize("pipe", ["phong", "shadow"])
@pytest.mark.parametrize("name", ["2047", "2048", "2049", "2050"])
def test_which_form_ran(small_synthetic, name, pipe):
    """Case 2: a frame of 2 x 2 whole tiles with the shared mode pinned.  The shared kernels have no interior form, so the
    scene reports the interior form exactly when every pass fell back to the column kernels: past 2^20 polygons."""
    mesh, texs = small_synthetic
    n = TABLES[name][0]
    Wf, Hf = 2 * TILE_W, 2 * TILE_H
    want_interior = H.expect_interior(Wf, Hf, pipe, 4, 2, n_poly=n * ROWS)
    assert want_interior == (n * ROWS > LIMIT)
    interior, kept = render_kept(Wf, Hf, m512(mesh), texs, pipe, tile_mode=2, instances=tab(name))
    assert interior == want_interior, "%d polygons: the %s kernels ran" % (n * ROWS, "interior column" if interior else "general")
    want = [oracle(small_synthetic, name, pipe, q=q, size=(Wf, Hf)) for q in VIEWS][::-1]
    assert_fused_parity(kept, want, pipe)


FUSED_LAYOUTS = ("auto", "shared4")


def _interior(pipe, layout, n_poly):
    """Must a fused launch of these 640 x 480 frames (whole tiles) have run the interior form?  Only four pinned waves
    can: shared4 past the limit, where the pass falls back to its columns."""
    opts = LAYOUTS[layout]
    return H.expect_interior(W, HH, pipe, opts.get("tile_waves", 0), opts.get("tile_mode", 0), n_poly=n_poly)


XNAMES = ("2047", "2048", "2049", "2050")      # the transform tables: xtab(name)
VIEWS4 = np.stack([view(CAM, LIGHT), view(0.0, 0.0), view(0.4, -0.3), view(-0.7, 0.5)])


@pytest.mark.gpu
@pytest.mark.parametrize("layout", FUSED_LAYOUTS)
@pytest.mark.parametrize("pipe,path", [("phong", "group2"), ("shadow", "group2"), ("shadow", "group1"), ("phong", "single2")])
@pytest.mark.parametrize("name", ["2048", "2049", "x2049"])
def test_fused_launches_on_the_limit(small_synthetic, name, pipe, path, layout):
    """Case 3: one group of four views by render_frames (transient depth, and stored depth for shadow) and, single2, a lone
    clear / render without the tap -- the kernels compiled for fused launches, asserted from the profile by fused_pair.
    x2049: the transform table, whose twins across the limit differ in colour -- no tap, and rgb still says who won."""
    mesh, texs = small_synthetic
    views = VIEWS4[:2] if path == "single2" else VIEWS4
    key, table = (("xform", "2049", None), dict(instance_transforms=xtab("2049"))) if name == "x2049" else (name, dict(instances=tab(name)))
    n = TABLES[name.lstrip("x")][0]
    expect = [oracle(small_synthetic, key, pipe, q=q) for q in views]
    # (640 x 480 is 5 x 30 whole tiles: four pinned waves that fall back to their columns run the interior form)
    interior = _interior(pipe, layout, n * ROWS)
    assert interior == (layout == "shared4" and n == 2049)
    kept, want = fused_pair(W, HH, m512(mesh), texs, pipe, views, path=path, expect=expect, interior=interior,
                            frames_per_launch=4, **table, **LAYOUTS[layout])
    assert_fused_parity(kept, want, pipe)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", FUSED_LAYOUTS)
@pytest.mark.parametrize("pipe", ["phong", "shadow"])
@pytest.mark.parametrize("name", ["2049", "2050"])
def test_render_frames_with_a_table_per_frame(small_synthetic, name, pipe, layout):
    """Case 3: render_frames(instances=...), four frames whose tables differ: with and without the lower twin of the pair
    across the limit (so the upper twin, past the limit, wins in every other frame).  Every pass must have fallen back:
    under four pinned shared waves the scene reports the interior column kernels."""
    import tiny_renderer_amd as T
    mesh, texs = small_synthetic
    keys = [name, (name, 2046), name, (name, 2046)]
    gpu = T.Scene(W, HH, m512(mesh), texs, pipe, frames_per_launch=4, **LAYOUTS[layout])
    gpu.render_frames(VIEWS4, instances=np.stack([tab(*k) if isinstance(k, tuple) else tab(k) for k in keys]))
    assert gpu.sync() == 0 and gpu.frames_kept() == 4
    want_interior = _interior(pipe, layout, TABLES[name][0] * ROWS)
    assert want_interior == (layout == "shared4")
    assert gpu.interior_tiles() == want_interior, "the %s form ran" % ("INTERIOR" if gpu.interior_tiles() else "general")
    for back in range(4):
        gpu.select_frame(back)
        assert_frame(grab(gpu, pipe), oracle(small_synthetic, keys[3 - back], pipe, q=VIEWS4[3 - back]), pipe, "frame %d" % (3 - back))
    gpu.close()


def _held_back(small, names, pipe, layout, store_depth=False, kind="tab"):
    """Renders one frame per table by the reference's four calls with set_instances (kind "xform": set_instance_transforms)
    in between and nothing read: the library holds the frames back and renders them as ONE group (asserted from the
    profile), whose layout goes by its largest frame -- asserted through interior_tiles(): under four pinned shared waves
    a group with one frame past the limit ran the interior column kernels, whichever frame that is; a group laid out by
    its smallest or its last frame would not have.
    What is compared: the rgb of EVERY frame, through the caller's buffer it was rendered into; z and shadow bits of the
    LAST frame only, which is the scene's current one -- select_frame does not reach held-back frames, so the earlier
    frames' depths are not read.  Under the transform tables the rgb alone says which twin won the ties across the limit."""
    import torch
    import tiny_renderer_amd as T
    mesh, texs = small
    g = len(names)
    # (created under the largest table: nothing grows later -- growing renders what is held back)
    first = dict(instances=tab("2050")) if kind == "tab" else dict(instance_transforms=xtab("2050"))
    gpu = T.Scene(W, HH, m512(mesh), texs, pipe, frames_per_launch=g, store_depth=store_depth, **first, **LAYOUTS[layout])
    assert gpu.frames_per_launch == g
    bufs = [torch.zeros(HH * W * 3, dtype=torch.uint8, device="cuda") for _ in names]
    gpu.profile_enable(True)
    for i, name in enumerate(names):
        if kind == "tab":
            gpu.set_instances(tab(name))
        else:
            gpu.set_instance_transforms(xtab(name))
        gpu.set_frame_buffer_device(bufs[i].data_ptr())
        frame(gpu, VIEWS4[i % 4])
    assert gpu.sync() == 0
    torch.cuda.synchronize()
    ran = _tile_launches(gpu.profile_read())
    assert ran["k_tile"] == (1, g), "the frames were not fused into one group: %r" % (ran,)
    want_interior = _interior(pipe, layout, max(TABLES[name][0] for name in names) * ROWS)
    assert gpu.interior_tiles() == want_interior, \
        "the group ran the %s form: its layout did not go by its largest frame" % ("INTERIOR" if gpu.interior_tiles() else "general")
    for i, name in enumerate(names):
        want = oracle(small, (kind, name, None), pipe, q=VIEWS4[i % 4])
        got = bufs[i].cpu().numpy().reshape(HH, W, 3)
        assert want["err"] == 0 and want["rgb"].any()
        assert np.array_equal(got, want["rgb"]), "frame %d (%s): rgb differs at %d pixels" % (i, name, int((got != want["rgb"]).any(-1).sum()))
    last = len(names) - 1
    assert_frame(grab(gpu, pipe), oracle(small, (kind, names[last], None), pipe, q=VIEWS4[last % 4]), pipe, "the last frame")
    gpu.profile_enable(False)
    gpu.close()


@pytest.mark.gpu
@pytest.mark.parametrize("layout", FUSED_LAYOUTS)
@pytest.mark.parametrize("pipe,store_depth", [("phong", False), ("shadow", False), ("shadow", True)])
@pytest.mark.parametrize("order", ["up", "down"])
def test_mixed_group_goes_by_its_largest_frame(small_synthetic, order, pipe, store_depth, layout):
    """Case 3: tables of 2047, 2048, 2049 and 2050 entries in ONE fused group, in that order and reversed (rgb of every
    frame, z and shadow of the last, the form that ran: _held_back)."""
    names = ["2047", "2048", "2049", "2050"]
    _held_back(small_synthetic, names if order == "up" else names[::-1], pipe, layout, store_depth)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", FUSED_LAYOUTS)
@pytest.mark.parametrize("pipe", ["phong", "shadow"])
@pytest.mark.parametrize("order", ["up", "down"])
def test_mixed_group_of_transform_tables(small_synthetic, order, pipe, layout):
    """Case 3 with transform tables of 2047 .. 2050 entries: the twins across the limit (frames 2049 and 2050) differ in
    colour, so a frame of the group that ran the shared kernels -- the group laid out by another frame than its largest,
    or no fallback at all -- gives the tie to the upper twin and its rgb differs."""
    _held_back(small_synthetic, list(XNAMES) if order == "up" else list(XNAMES)[::-1], pipe, layout, kind="xform")


@pytest.mark.gpu
@pytest.mark.parametrize("layout", FUSED_LAYOUTS)
@pytest.mark.parametrize("pipe", ["phong", "shadow"])
def test_held_back_frames_across_the_limit(small_synthetic, pipe, layout):
    """Case 4: 2048 -> 2049 -> 2048 entries between held-back frames (the pattern of test_held_back_frames_keep_their_table):
    rgb of every frame, z and shadow of the last -- see _held_back for why not more."""
    _held_back(small_synthetic, ["2048", "2049", "2048"], pipe, layout)


@pytest.mark.gpu
@pytest.mark.parametrize("pipe", ["phong", "shadow"])
@pytest.mark.parametrize("name", ["2048", "2049"])
def test_accumulating_render_on_the_limit(small_synthetic, name, pipe):
    """Case 5: a second render without a clear and with the same camera: every fragment ties with what the buffers hold --
    the colour pass rejects it, the depth pass accepts it.  The oracle does the same two renders."""
    import tiny_renderer_amd as T
    mesh, texs = small_synthetic
    gpu = T.Scene(W, HH, m512(mesh), texs, pipe, winner_tap=True, instances=tab(name))
    frame(gpu)
    frame(gpu, clear=False)
    assert_frame(grab(gpu, pipe, winner=True), oracle(small_synthetic, name, pipe, renders=2), pipe, "second render")
    gpu.close()


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["auto", "shared8"])
@pytest.mark.parametrize("pipe", ["phong", "shadow"])
@pytest.mark.parametrize("kind", ["xform", "posed"])
def test_other_table_kinds_across_the_limit(small_synthetic, kind, pipe, layout):
    """Case 6: a transform table (scaled rotations) with twins across the limit, and a morph pose under TAB(2049): against
    the oracle with the winner, and against a GPU scene of the host-built mesh."""
    import tiny_renderer_amd as T
    mesh, texs = small_synthetic
    m = m512(mesh)
    if kind == "xform":
        gpu = T.Scene(W, HH, m, texs, pipe, winner_tap=True, instance_transforms=xtab("2049"), **LAYOUTS[layout])
    else:
        gpu = T.Scene(W, HH, m, texs, pipe, winner_tap=True, instances=tab("2049"), **LAYOUTS[layout])
        gpu.set_morph_targets(*_targets(m))
        gpu.set_morph_weights(POSE)
    ref = T.Scene(W, HH, cat(mesh, kind), texs, pipe, winner_tap=True, **LAYOUTS[layout])
    frame(gpu)
    frame(ref)
    got, host = grab(gpu, pipe, winner=True), grab(ref, pipe, winner=True)
    want = oracle(small_synthetic, kind, pipe)
    assert_frame(got, want, pipe, "%s %s %s" % (kind, pipe, layout))
    assert_frame(host, want, pipe, "%s %s %s, host-built mesh" % (kind, pipe, layout))
    gpu.close()
    ref.close()
