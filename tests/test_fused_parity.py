"""Oracle parity of the FUSED tile kernels -- the instantiations every user gets by default -- at full size and at the
bin-length edges.

k_tile<FS, WAVES, SHARED, MODE> is compiled three times (launch_tile_waves, csrc/tr_kernels.hip): MODE 0 for per-frame
passes with a winner tap, tile stamps or uncleared targets; MODE 1 for fused launches that store their depth; MODE 2 for
fused launches whose depth stays on the chip (every cleared frame without a tap: what bench.py times).  The winner tap of
render_pair() (test_gpu_parity.py) pins a scene to MODE 0, so the hard inputs of that module never reach the fused modes;
here the same inputs -- and a ladder of bins of every length across every per-tile threshold -- go through scenes WITHOUT
a tap, in three paths:

    group2   render_frames, default depth handling          -> MODE 2, arguments from the group's table
    group1   render_frames, store_depth=True                -> MODE 1
    single2  clear(); set_*; render() with auto_group=False -> fused_single: MODE 2, arguments by value

Every compare is bit equality with the CPU oracle (z bits through read_z_f32 -- for MODE 2 the on-demand depth repeat --,
shadow bits, rgb; specular falls back to 1 LSB only where the build has no exact powf, as in test_gpu_parity.py).  Every
case also proves from the kernel profile that it ran what it claims: one k_tile launch per group (or per frame) covering
the expected frames, depth repeats exactly where the depth was transient, and no empty frame.
PARITY UNPINNED upstream: the oracle is the normative restatement (oracle/tr_oracle.h)."""
import numpy as np
import pytest

from tests import helpers as H
from tests.test_random_meshes import FAR_SEEDS, far_case

EXACT = ("default", "phong", "normal_map", "darboux", "shadow", "occlusion")
ALL = EXACT + ("specular",)
TWO_PASS = ("shadow", "occlusion")
FUSED_PATHS = ("group2", "group1", "single2")
NO_WINNER = 0xFFFFFFFF


def specular_exact():
    import tiny_renderer_amd as T
    return bool(T.load_library().tr_specular_exact())


def view(cam_angle, light_angle):
    """One row of render_frames' table: light, look_from, look_at, up."""
    f, a, u = H.camera(cam_angle)
    return np.array(list(H.light(light_angle)) + list(f) + list(a) + list(u), np.float32)


def oracle_views(W, Hh, mesh, texs, pipe, views):
    """The oracle's frame for every DISTINCT row of `views` (one render each), as a list parallel to `views`:
    dicts of rgb (as get_frame_buffer returns it), z bits, shadow bits (two-pass pipelines), winner and err."""
    from oracle import oracle as O
    cpu = O.Scene(W, Hh, mesh, texs, pipe)
    seen, out = {}, []
    for q in np.asarray(views, np.float32).reshape(-1, 12):
        key = q.tobytes()
        if key not in seen:
            cpu.clear()
            cpu.set_light_direction(q[0:3])
            cpu.set_camera(q[3:6], q[6:9], q[9:12])
            err = cpu.render()
            seen[key] = dict(err=err, rgb=cpu.get_frame_buffer(), z=cpu.z_f32().view(np.uint32),
                             shadow=cpu.shadow_f32().view(np.uint32) if pipe in TWO_PASS else None,
                             winner=cpu.winner_u32(), tri_kept=cpu.stats()[0]["tri_kept"])
        out.append(seen[key])
    cpu.close()
    return out


def _grab(gpu, pipe):
    """What a scene holds for its current frame.  The colour first: the z read of a transient frame repeats the pass."""
    rgb = gpu.get_frame_buffer()
    return dict(rgb=rgb, z=gpu.read_z_f32().view(np.uint32),
                shadow=gpu.read_shadow_f32().view(np.uint32) if pipe in TWO_PASS else None)


def _tile_launches(prof):
    return {k: (prof.get(k, {"launches": 0, "frames": 0})["launches"], prof.get(k, {"launches": 0, "frames": 0})["frames"])
            for k in ("k_tile", "k_tile_depth", "k_bin", "k_lit")}


def _assert_form(gpu, interior, what):
    if interior is not None:
        assert gpu.interior_tiles() == interior, \
            "%s: the %s form of the tile kernels ran" % (what, "INTERIOR" if gpu.interior_tiles() else "general")


def fused_pair(W, Hh, mesh, texs, pipe, views, path="group2", expect=None, oracle_mesh=None, interior=None, lit=None, **opts):
    """Renders `views` ([n, 12]: light and camera per frame) through a scene WITHOUT a winner tap by one of FUSED_PATHS and
    returns (kept, want): the frames the GPU kept (newest first for the group paths; every frame in turn for single2)
    beside the oracle's frames for the same views.  Asserts from the profile that the colour pass ran as ONE k_tile launch
    per group (group paths: the groups of `frames_per_launch` frames; single2: one launch of one frame per render), the
    depth pass of a two-pass pipeline likewise, and that reading the z buffer repeats the pass exactly when the depth was
    transient (MODE 2) -- which a MODE 0 or MODE 1 launch in its place would not do.
    expect: oracle frames computed before (oracle_views(...) of the same views); oracle_mesh: what the oracle renders when
    the scene draws something else than `mesh` itself (an instance table).
    interior: which FORM of the kernels must have run (Scene.interior_tiles(): every pass of the newest fused launches in
    the form compiled for frames of whole tiles) -- H.expect_interior(...) where the caller pins the layout, a literal with
    its reason where the scene chooses; asked after the launches (single2: after every render) and before any getter.
    lit: must k_lit have run (once per group or render) or not at all; None: not looked at."""
    import tiny_renderer_amd as T
    assert path in FUSED_PATHS
    views = np.ascontiguousarray(views, np.float32).reshape(-1, 12)
    n = len(views)
    if expect is None:
        expect = oracle_views(W, Hh, oracle_mesh if oracle_mesh is not None else mesh, texs, pipe, views)
    n_pass = 2 if pipe in TWO_PASS else 1
    kept, want = [], []
    if path == "single2":
        gpu = T.Scene(W, Hh, mesh, texs, pipe, auto_group=False, **opts)
        for i, q in enumerate(views):
            if any(q.tobytes() == p.tobytes() for p in views[:i]):
                continue   # (a view rendered before: nothing new)
            gpu.profile_enable(True)
            gpu.clear()
            gpu.set_light_direction(q[0:3])
            gpu.set_camera(q[3:6], q[6:9], q[9:12])
            gpu.render()
            assert gpu.sync() == 0
            ran = _tile_launches(gpu.profile_read())
            assert ran["k_tile"] == (1, 1), ran
            assert ran["k_tile_depth"] == ((1, 1) if n_pass == 2 else (0, 0)), ran
            assert ran["k_bin"] == (n_pass, n_pass), ran
            assert lit is None or ran["k_lit"] == ((1, 1) if lit else (0, 0)), ran
            _assert_form(gpu, interior, "%s, %dx%d, render %d" % (pipe, W, Hh, i))
            kept.append(_grab(gpu, pipe))
            again = _tile_launches(gpu.profile_read())
            assert again["k_tile"][0] == 2, "the depth was not transient: not the MODE 2 kernel (%r)" % (again,)
            gpu.profile_enable(False)
            want.append(expect[i])
    else:
        gpu = T.Scene(W, Hh, mesh, texs, pipe, store_depth=(path == "group1"), **opts)
        g = gpu.frames_per_launch
        assert opts.get("frames_per_launch", g) == g
        groups = (n + g - 1) // g
        gpu.profile_enable(True)
        gpu.render_frames(views)
        assert gpu.sync() == 0
        ran = _tile_launches(gpu.profile_read())
        assert ran["k_tile"] == (groups, n), ran
        assert ran["k_tile_depth"] == ((groups, n) if n_pass == 2 else (0, 0)), ran
        assert ran["k_bin"] == (groups * n_pass, n * n_pass), ran
        assert lit is None or ran["k_lit"] == ((groups, n) if lit else (0, 0)), ran
        _assert_form(gpu, interior, "%s, %dx%d, path %s" % (pipe, W, Hh, path))
        n_kept = gpu.frames_kept()
        assert n_kept == min(n, g)
        for back in range(n_kept):
            gpu.select_frame(back)
            kept.append(_grab(gpu, pipe))
            want.append(expect[n - 1 - back])
        again = _tile_launches(gpu.profile_read())
        repeats = n_kept if path == "group2" else 0   # one depth-only repeat per transient frame, none for stored depth
        assert again["k_tile"][0] == groups + repeats, "path %s: %r after %r" % (path, again, ran)
        gpu.profile_enable(False)
    gpu.close()
    return kept, want


def _where(diff, note):
    ys, xs = np.nonzero(diff)
    return "%d pixels, first at row %d column %d%s" % (len(ys), int(ys[0]), int(xs[0]), note(int(ys[0])) if note else "")


def assert_fused_parity(kept, want, pipe, note_z=None, note_rgb=None, allow_empty=False):
    """Every kept frame against the oracle's: z bits, shadow bits, rgb.  note_z / note_rgb: row -> text appended to a
    failure's message (rows of the z and shadow buffers count from the bottom, rows of the frame from the top)."""
    assert kept and len(kept) == len(want)
    for k, (g, o) in enumerate(zip(kept, want)):
        assert o["err"] == 0, "the reference would panic on this frame (oracle err %#x)" % o["err"]
        assert allow_empty or o["rgb"].any(), "an empty frame proves nothing"
        assert np.array_equal(g["z"], o["z"]), "frame %d: z bits differ at %s" % (k, _where(g["z"] != o["z"], note_z))
        if pipe in TWO_PASS:
            assert np.array_equal(g["shadow"], o["shadow"]), \
                "frame %d: shadow bits differ at %s" % (k, _where(g["shadow"] != o["shadow"], note_z))
        if pipe in EXACT or specular_exact():
            assert np.array_equal(g["rgb"], o["rgb"]), \
                "frame %d: rgb differs at %s" % (k, _where((g["rgb"] != o["rgb"]).any(-1), note_rgb))
        else:
            d = np.abs(g["rgb"].astype(np.int32) - o["rgb"].astype(np.int32))
            assert d.max() <= 1, "frame %d: specular rgb differs by %d" % (k, int(d.max()))  # tolerance: 1 LSB (device powf)


def five_frames(a, b):
    """Five frames of two distinct views: with four frames per launch, groups of 4 + 1; the frames kept are b, b, a (places
    1, 2, 3 of the first group) and b (a group of its own)."""
    return np.stack([a, b, b, a, b])


# ---- 1. full-size real models through the fused paths ---------------------------------------------------------------

def _full_size(mesh, texs, pipe, size, path, a, b, interior, expect=None, **opts):
    """size: the side of a square frame, or (width, height).  interior: the form that must have run (fused_pair)."""
    # (frames_per_launch=4 is what a 4096^2 scene chooses by itself; pinned so that every size gets groups of 4 + 1)
    W, Hh = size if isinstance(size, tuple) else (size, size)
    kept, want = fused_pair(W, Hh, mesh, texs, pipe, five_frames(a, b), path=path, expect=expect, interior=interior,
                            frames_per_launch=4, **opts)
    assert len(kept) == (2 if path == "single2" else 4)
    assert_fused_parity(kept, want, pipe)


# Which form the scenes that choose their own layout must run (tile_layout, csrc/tr_scene.cpp: 16 waves up to 1024 tiles in
# a launch, 8 up to 4608, else 4; the waves share a tile's bin -- no interior form -- up to 2048 tiles per frame or from three
# polygons per tile).  diablo has 5022 polygons.
#   4096^2        32 x 256 = 8192 tiles per frame (32768 in a launch of four), 0.6 polygons per tile: 4 waves, columns --
#                 phong and shadow (depth pass: the same grid) have the form in every pass, darboux's closure has none
#   8192^2 x64    64 x 512 = 32768 tiles, 321 408 polygons = 9.8 per tile: dense, the shared resolve
#   2048^2        16 x 128 = 2048 tiles per frame: the shared resolve
#   800^2         7 x 50 = 350 tiles per frame, 1400 in a launch of four: 16 or 8 waves (and partial tiles)
AUTO_INTERIOR = {("phong", 4096): True, ("shadow", 4096): True, ("darboux", 4096): False, ("specular", 8192): False}


@pytest.mark.gpu
@pytest.mark.parametrize("path", FUSED_PATHS)
@pytest.mark.parametrize("cfg", [("phong", 4096, 1), ("darboux", 4096, 1), ("shadow", 4096, 1), ("specular", 8192, 8)])
def test_baseline_configs_at_full_size_fused(diablo, cfg, path):
    """test_baseline_configs_at_full_size's four configs (BASELINE.json configs[2..4] and the metric's own workload) through
    the fused kernels; the x64 grid at 8192^2 is the one that takes the SHARED resolve and the lit-texel path by itself.
    All three paths run at 8192^2 too, group1 included (measured: about 4 s per case there, two oracle frames included)."""
    import tiny_renderer_amd as T
    pipe, size, grid = cfg
    mesh, texs = diablo
    if grid > 1:
        mesh = T.instanced_grid(mesh, grid)
    _full_size(mesh, texs, pipe, size, path, view(0.0, 0.0), view(0.11, 0.23), interior=AUTO_INTERIOR[(pipe, size)])


@pytest.mark.gpu
@pytest.mark.parametrize("path", FUSED_PATHS)
def test_african_head_default_800_fused(african_head, path):
    """BASELINE.json configs[0]."""
    mesh, texs = african_head
    _full_size(mesh, texs, "default", 800, path, view(0.0, 0.0), view(0.37, -0.5), interior=False)  # (8 or 16 waves)


@pytest.mark.gpu
@pytest.mark.parametrize("path", FUSED_PATHS)
def test_diablo_phong_2048_fused(diablo, path):
    """BASELINE.json configs[1]."""
    mesh, texs = diablo
    _full_size(mesh, texs, "phong", 2048, path, view(0.0, 0.0), view(0.37, -0.5), interior=False)  # (shared resolve)


@pytest.mark.gpu
@pytest.mark.parametrize("path", FUSED_PATHS)
@pytest.mark.parametrize("pipe", ALL)
def test_diablo_800_fused(diablo, pipe, path):
    """test_diablo_800's two views -- angles (0, 0) and (0.7, -1.1) -- as the two views of the five frames."""
    mesh, texs = diablo
    _full_size(mesh, texs, pipe, 800, path, view(0.0, 0.0), view(0.7, -1.1), interior=False)  # (8 or 16 waves)


# ---- 2. a real model through BOTH forms of the four-wave column kernels -------------------------------------------------
#
# No real model reaches the general four-wave column kernels by itself (800^2: 8 or 16 waves; 2048^2: the shared resolve;
# 4096^2: the interior form), and the interior form's closures beside phong and shadow meet a real model nowhere else.  The
# layout is pinned here and the size decides the form: 768 = 6 x 128 = 48 x 16 is whole tiles, 800 is not.

FOUR_COLUMNS = dict(tile_waves=4, tile_mode=1)
LIT_PIPES = H.LIT_PIPES


def _both_forms_cases():
    """(size, pipeline, TR_LIT, path): every pipeline through group2 and single2, phong and shadow through group1 as well,
    the two texel closures once more on the lit path -- the cases of one (size, pipeline) side by side, sharing an oracle."""
    out = []
    for size in (768, 800):
        for pipe in ALL:
            paths = FUSED_PATHS if pipe in ("phong", "shadow") else ("group2", "single2")
            out += [(size, pipe, None, path) for path in paths]
            if pipe in LIT_PIPES:
                out.append((size, pipe, "1", "group2"))
    return out


_both_forms_oracle = {}


@pytest.mark.gpu
@pytest.mark.parametrize("size,pipe,force_lit,path", _both_forms_cases())
def test_diablo_both_forms_of_the_column_kernels(diablo, monkeypatch, size, pipe, force_lit, path):
    """test_diablo_800_fused's two views in the four-wave column layout at 768^2 (6 x 48 whole tiles) and 800^2: at 768^2
    default, phong, shadow and the lit path's FS_LIT run the interior form, darboux and the closures per fragment have
    none, and occlusion is the mixed case -- an interior depth pass before a general colour pass, for which the query must
    say no; at 800^2 everything runs the general kernels.  H.expect_interior says which, fused_pair asserts it."""
    mesh, texs = diablo
    if force_lit is not None:
        monkeypatch.setenv("TR_LIT", force_lit)
    lit = H.lit_path(size, size, texs, pipe)
    assert lit == (force_lit == "1"), "1024^2 images: these frames take the lit path only when told to"
    a, b = view(0.0, 0.0), view(0.7, -1.1)
    if (size, pipe) not in _both_forms_oracle:   # (one entry: the cases of a size and pipeline follow each other)
        _both_forms_oracle.clear()
        _both_forms_oracle[(size, pipe)] = oracle_views(size, size, mesh, texs, pipe, five_frames(a, b))
    interior = H.expect_interior(size, size, pipe, 4, 1, lit=lit)
    assert interior == (size == 768 and (pipe in ("default", "phong", "shadow") or lit))
    _full_size(mesh, texs, pipe, size, path, a, b, interior, expect=_both_forms_oracle[(size, pipe)],
               lit=lit if pipe in LIT_PIPES else None, **FOUR_COLUMNS)


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["group2", "group1"])
@pytest.mark.parametrize("pipe", ["phong", "shadow"])
def test_headline_layout_in_the_general_form_at_full_size(diablo, pipe, path):
    """4096 x 4088: the 32 x 256 tiles and the layout a 4096^2 scene chooses by itself (AUTO_INTERIOR above: 4 waves,
    columns), but the top tile row is half a tile high -- the general MODE 2 and MODE 1 kernels, the depth pass included,
    at the size of the headline workload."""
    mesh, texs = diablo
    _full_size(mesh, texs, pipe, (4096, 4088), path, view(0.0, 0.0), view(0.11, 0.23), interior=False)


# ---- 3. a bin-length ladder: every n across every threshold, in one frame ------------------------------------------
#
# Resident-record budgets the ladder relies on: a tile whose bin holds n <= NMAX records shades from LDS (RESIDENT), a
# larger one takes the chunked path.  NMAX = lds_rec_bytes_for(WAVES, tile_waves_per_eu(FS, WAVES, MODE != 0, SHARED),
# SHARED) / (P * 16), P = rec_pieces_for_fs(FS) (6; darboux 9), as the constants stand:
#
#   WAVES  FS (pipeline pass)           resolve   waves/SIMD  MODE 0 -> NMAX   waves/SIMD  MODE 1, 2 -> NMAX
#     4    FS_PHONG  (phong)            columns       7            68              8             41
#     4    FS_PHONG                     shared        7            57              7             57
#     4    FS_DARBOUX (darboux, P = 9)  columns       4            56              5             56
#     4    FS_DARBOUX                   shared        4            56              5             56
#     4    FS_SHADOW2 (shadow, colour)  columns       7            68              7             68
#     4    FS_SHADOW2                   shared        7            57              7             57
#     4    FS_DEPTH  (shadow, depth)    columns       7            68              8             41
#     4    FS_DEPTH                     shared        7            57              7             57
#     8    P = 6 / P = 9                either        -           256 / 170        -            256 / 170
#    16    P = 6 / P = 9                either        -           426 / 284        -            426 / 284
#
# Other thresholds on n: shared_tile = n >= 2 * WAVES (8, 16, 32) && n <= SHARED_MAX_SLOTS (4093); the staging chunks
# (multiples of NMAX); k_order's work-list buckets; the empty list's chunks of 32 tiles.
LADDER_W = 128
# The ladder's other widths -- every polygon ends at column 123, so the designed bins hold at each: 125 has a partial tile
# column (the lanes of columns 125 ... 127 are dead) and, no multiple of 4, takes the byte-store arm; 124 takes the dword
# arm with a partial last strip.  Neither is a frame of whole tiles: what 128 runs in the interior form they run in the
# general one.
LADDER_WIDTHS = (LADDER_W, 125, 124)
DENSE = list(range(1, 449))
COUNTS = DENSE + [1000, 4092, 4093, 4094] + [0] * 8 + [50]
LADDER_SEED = 7
LADDER_Z = (-0.3, -0.15, 0.0, 0.15, 0.3)
# Records per pass pool: no polygon is higher than 14 pixels or wider than a tile, so under the camera and under the lights
# below it meets at most two tiles.  (The automatic capacity is an estimate from the frame's size -- 1.3 records per polygon
# here -- which the light's slightly smaller view of the ladder, where polygons straddle tile rows, exceeds: the pools
# would grow and the frames be rendered again, correct but twice the launches the cases assert.)
LADDER_POOL = 2 * sum(COUNTS)
LADDER_LIGHTS = ((0.0, 0.0, 1.0), (0.012, 0.0, 1.1), (-0.012, 0.0, 1.1))


def ladder_mesh(counts, seed, width=LADDER_W):
    """A frame `width` <= 128 pixels wide and 16 * len(counts) high is one column of 128x16 tiles; tile k (counted from the
    bottom row of the raster, the order of the tile kernel's tile index) receives exactly counts[k] polygons, each wholly
    inside the tile's rectangle (>= 4 pixels from its left and right edge, >= 1 from the lower and upper one), front
    facing, with integer raster vertices that are not collinear (so each covers its own vertices' pixels at least).
    Mixed within a tile: tiny ones (box at most 8 pixels wide: scan-line items of the shared resolve), medium ones, and
    ones wider than four 8-pixel chunks (whole-wave visits); depths from the coarse grid LADDER_Z, constant over most
    polygons (tilted ones only where they still face the camera in object space), so that overlapping fragments tie
    exactly and polygon order decides.  The polygons are shuffled: a tile's polygon indices are neither contiguous nor
    ordered by size.
    Object-space vertices come from the wanted raster positions -- the same at every width -- through the inverse
    (float64) of the oracle's vpmv for camera angle 0 in a frame of that width.  Returns (mesh, textures); mesh["tile_of"][t] is the tile polygon t was made for."""
    from oracle import oracle as O
    assert 124 <= width <= 128, "every polygon must lie inside the frame's one tile column"
    rng = np.random.default_rng(seed)
    counts = np.asarray(counts, np.int64)
    Hh = 16 * len(counts)
    n = int(counts.sum())
    tile_of = np.repeat(np.arange(len(counts)), counts)
    kind = rng.random(n)
    tiny, wide = kind < 0.6, kind >= 0.85
    w = np.where(tiny, rng.integers(1, 8, n), np.where(wide, rng.integers(40, 111, n), rng.integers(9, 31, n)))
    h = np.where(tiny, rng.integers(1, 6, n), np.where(wide, rng.integers(3, 14, n), rng.integers(2, 11, n)))
    x0 = 4 + (rng.random(n) * (120 - w)).astype(np.int64)            # x0 >= 4, x0 + w <= 123
    y0 = 16 * tile_of + 1 + (rng.random(n) * (14 - h)).astype(np.int64)  # y0 >= 1, y0 + h <= 14 inside the tile
    a = (rng.random(n) * h).astype(np.int64)                         # 0 .. h - 1
    b = (rng.random(n) * (w + 1)).astype(np.int64)                   # 0 .. w
    # counter-clockwise with y up: (w, a) x (b, h) = w * h - a * b >= w > 0
    px = np.stack([x0, x0 + w, x0 + b], 1)
    py = np.stack([y0, y0 + a, y0 + h], 1)
    turn = rng.integers(0, 3, n)                                     # which vertex comes first
    sel = (np.arange(3)[None, :] + turn[:, None]) % 3
    px, py = np.take_along_axis(px, sel, 1), np.take_along_axis(py, sel, 1)
    zgrid = np.asarray(LADDER_Z, np.float64)
    zflat = np.repeat(zgrid[rng.integers(0, len(zgrid), n)][:, None], 3, 1)
    ztilt = zgrid[rng.integers(0, len(zgrid), (n, 3))]
    tilt = rng.random(n) < 1.0 / 3.0
    # raster position (px + 0.5, py + 0.5) truncates to (px, py) whatever the last bits of the float32 transform do
    cam = H.camera(0.0)
    err, u = O.prepare(0, width, Hh, H.light(0.0), *cam)
    assert err == 0
    M = np.array(u.vpmv, np.float64).reshape(4, 4).T                # column major
    xs, ys = px + 0.5, py + 0.5

    def unproject(z):
        a00, a01 = M[0, 0] - xs * M[3, 0], M[0, 1] - xs * M[3, 1]
        a10, a11 = M[1, 0] - ys * M[3, 0], M[1, 1] - ys * M[3, 1]
        b0 = -((M[0, 2] - xs * M[3, 2]) * z + (M[0, 3] - xs * M[3, 3]))
        b1 = -((M[1, 2] - ys * M[3, 2]) * z + (M[1, 3] - ys * M[3, 3]))
        det = a00 * a11 - a01 * a10
        return (b0 * a11 - a01 * b1) / det, (a00 * b1 - b0 * a10) / det

    def facing(x, y):   # z of the object-space face normal: what the back-face test looks at with the camera on +z
        return (x[:, 1] - x[:, 0]) * (y[:, 2] - y[:, 0]) - (x[:, 2] - x[:, 0]) * (y[:, 1] - y[:, 0])

    fx, fy = unproject(zflat)
    tx, ty = unproject(ztilt)
    # the perspective moves a vertex with its depth: a tilted polygon that is small on the screen may face away in
    # object space (and would be culled before binning) -- those stay flat
    tilt &= facing(tx, ty) > 0.5 * facing(fx, fy)
    assert (facing(fx, fy) > 0).all()
    z = np.where(tilt[:, None], ztilt, zflat)
    ox, oy = np.where(tilt[:, None], tx, fx), np.where(tilt[:, None], ty, fy)
    order = rng.permutation(n)
    pos = np.stack([ox, oy, z], -1)[order].reshape(-1, 3).astype(np.float32)
    nrm = rng.standard_normal((n * 3, 3))
    nrm[:, 2] = np.abs(nrm[:, 2]) + 0.5                              # towards the camera, mostly
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    tex = np.concatenate([rng.uniform(0.05, 0.95, (n * 3, 2)), np.zeros((n * 3, 1))], 1).astype(np.float32)
    idx = np.arange(n * 3, dtype=np.uint32).reshape(n, 3).repeat(3, axis=1)
    texs = [rng.integers(0, 256, (32, 32, 3), dtype=np.uint8) for _ in range(4)]
    return {"pos": pos, "tex": tex, "nrm": nrm, "idx": idx, "tile_of": tile_of[order]}, texs


def ladder_views(n=3, width=LADDER_W):
    """The ladder's views at one of LADDER_WIDTHS -- the same at each: test_ladder_design_holds checks them width by width.
    Camera at angle 0 (the bins keep their designed lengths), n slightly different lights.  The lights that leave the
    camera's axis are also farther away than the camera: the light's view of the ladder is then a little smaller than the
    camera's and every lookup of the shadow pipeline stays inside the shadow buffer (on the axis at distance 1 the polygons
    of the first and the last tile sit one pixel from its edge; the oracle reports any lookup out of range)."""
    assert width in LADDER_WIDTHS, "a width the design test does not cover"
    out = np.stack([view(0.0, 0.0)] * n)
    out[:, 0:3] = LADDER_LIGHTS[:n]
    return out


_ladder = {}
# pipeline -> the widths a parity test renders it at (test_ladder_parity, ..._general_form, ..._default_and_lit)
LADDER_ORACLE_WIDTHS = {"phong": LADDER_WIDTHS, "shadow": LADDER_WIDTHS, "darboux": (LADDER_W,),
                        "default": (LADDER_W, 125), "normal_map": (LADDER_W, 125)}


def ladder(width=LADDER_W):
    if ("mesh", width) not in _ladder:
        _ladder[("mesh", width)] = ladder_mesh(COUNTS, LADDER_SEED, width)
    return _ladder[("mesh", width)]


def ladder_oracle(pipe, width=LADDER_W):
    """The oracle's three ladder frames of a pipeline at a width, rendered once per session."""
    if (pipe, width) not in _ladder:
        mesh, texs = ladder(width)
        _ladder[(pipe, width)] = oracle_views(width, 16 * len(COUNTS), mesh, texs, pipe, ladder_views(3, width))
    return _ladder[(pipe, width)]


def check_ladder_design(counts, seed, width=LADDER_W):
    mesh, texs = ladder(width) if (list(counts) == COUNTS and seed == LADDER_SEED) else ladder_mesh(counts, seed, width)
    Hh = 16 * len(counts)
    o = oracle_views(width, Hh, mesh, texs, "phong", ladder_views(1, width))[0]
    assert o["err"] == 0
    assert o["tri_kept"] == sum(counts) == mesh["idx"].shape[0], "a polygon was culled"
    win = o["winner"]
    ys, xs = np.nonzero(win != NO_WINNER)
    # every polygon that wins a pixel wins it only inside its own tile's rows (winner rows count from the bottom)
    assert np.array_equal(mesh["tile_of"][win[ys, xs]], ys // 16), "a polygon won a pixel outside its tile"
    assert xs.min() >= 4 and xs.max() <= 123
    lit = np.bincount(ys // 16, minlength=len(counts)) > 0
    assert np.array_equal(lit, np.asarray(counts) > 0), "a busy tile without lit pixels, or an empty one with"
    # (the frame getter flips: tile k's rows of the image are counted from the bottom)
    rows = o["rgb"].any(-1).any(-1).reshape(len(counts), 16).any(-1)[::-1]
    assert np.array_equal(rows | ~lit, np.ones(len(counts), bool)) and not rows[np.asarray(counts) == 0].any()
    # a tile of n polygons shows many of them: the bins' order matters in every tile
    shown = np.array([np.unique(win[16 * k:16 * k + 16][win[16 * k:16 * k + 16] != NO_WINNER]).size for k in range(len(counts))])
    assert (shown >= np.minimum(np.asarray(counts), 12) * 0.5).all()


def test_ladder_counts_cover_the_thresholds():
    """The ladder must reach beyond the largest resident-record budget there is (426: sixteen waves, P = 6): a future
    larger budget makes this fail loudly rather than the ladder go blind."""
    assert DENSE == list(range(1, max(DENSE) + 1)) and max(DENSE) > 426 + 1
    assert COUNTS[len(DENSE):len(DENSE) + 4] == [1000, 4092, 4093, 4094]      # around SHARED_MAX_SLOTS
    assert COUNTS[-9:] == [0] * 8 + [50]                                      # an empty chunk between busy tiles


def test_ladder_design_holds(built):
    """CPU: the ladder is the input it claims to be -- nothing culled or degenerate, every polygon inside its own tile's
    rows, every busy tile lit -- at every width the parity tests render it.  (A condition on the generator, not on the
    code under test.)"""
    for width in LADDER_WIDTHS:
        check_ladder_design(COUNTS, LADDER_SEED, width)
    # the three lights of the parity tests: no lookup outside the shadow buffer or (default, normal_map) the 32 x 32 images,
    # the same polygons kept
    for pipe, widths in LADDER_ORACLE_WIDTHS.items():
        for width in widths:
            for o in ladder_oracle(pipe, width):
                assert o["err"] == 0 and o["tri_kept"] == sum(COUNTS) and o["rgb"].any(), (pipe, width)


@pytest.mark.gpu
def test_ladder_bins_hold_the_designed_counts(built):
    """GPU, input check: the polygons the tile kernel finds in each tile's bin (column 2 of the tile stamps; MODE 0) are
    COUNTS tile for tile -- n is known exactly, in every tile, at the whole-tile width and at one with a partial tile."""
    import tiny_renderer_amd as T
    for width in (LADDER_W, 125):
        mesh, texs = ladder(width)
        q = ladder_views(1, width)[0]
        gpu = T.Scene(width, 16 * len(COUNTS), mesh, texs, "phong", tile_stamps=True, bin_capacity=LADDER_POOL)
        gpu.clear()
        gpu.set_light_direction(q[0:3])
        gpu.set_camera(q[3:6], q[6:9], q[9:12])
        gpu.render()
        assert gpu.sync() == 0
        stamps = gpu.debug_tile_stamps()
        assert stamps.shape[0] == len(COUNTS)
        got = stamps[:, 2].astype(np.int64)
        bad = np.nonzero(got != np.asarray(COUNTS))[0]
        assert bad.size == 0, \
            "width %d: tiles %s hold %s polygons, designed %s" % (width, bad[:8], got[bad[:8]], np.asarray(COUNTS)[bad[:8]])
        gpu.close()


def _ladder_note(flipped):
    Hh = 16 * len(COUNTS)

    def note(row):
        k = ((Hh - 1 - row) if flipped else row) // 16
        return " = tile %d with n = %d" % (k, COUNTS[k])
    return note


@pytest.mark.gpu
@pytest.mark.parametrize("pipe", ["phong", "darboux", "shadow"])
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("waves", [4, 8, 16])
@pytest.mark.parametrize("path", FUSED_PATHS + ("tap0",))
def test_ladder_parity(built, path, waves, mode, pipe):
    """Every bin length 1 ... 448, 1000, 4092 ... 4094, eight empty tiles and one more busy tile, through every path, layout
    and resolve: phong (P = 6), darboux (P = 9, the pair closure and its redo pass), shadow (depth pass + colour pass).  A
    failure names the tile and its n: the threshold that broke."""
    import tiny_renderer_amd as T
    mesh, texs = ladder()
    W, Hh = LADDER_W, 16 * len(COUNTS)
    views, expect = ladder_views(), ladder_oracle(pipe)
    if path == "tap0":   # today's render_pair: MODE 0, winner compare
        gpu = T.Scene(W, Hh, mesh, texs, pipe, winner_tap=True, tile_waves=waves, tile_mode=mode, bin_capacity=LADDER_POOL)
        for q, o in zip(views, expect):
            gpu.clear()
            gpu.set_light_direction(q[0:3])
            gpu.set_camera(q[3:6], q[6:9], q[9:12])
            gpu.render()
            wg = gpu.read_winner_u32()
            assert np.array_equal(wg, o["winner"]), "winner differs at %s" % _where(wg != o["winner"], _ladder_note(False))
            assert_fused_parity([_grab(gpu, pipe)], [o], pipe, _ladder_note(False), _ladder_note(True))
        gpu.close()
        return
    kept, want = fused_pair(W, Hh, mesh, texs, pipe, views, path=path, expect=expect, tile_waves=waves, tile_mode=mode,
                            interior=H.expect_interior(W, Hh, pipe, waves, mode), frames_per_launch=3, bin_capacity=LADDER_POOL)
    assert len(kept) == 3
    assert_fused_parity(kept, want, pipe, _ladder_note(False), _ladder_note(True))


def _ladder_case(width, pipe, path, interior, lit=None):
    """One ladder case in the four-wave column layout at a width: the form and (lit given) k_lit asserted, z, shadow and
    rgb bits against the oracle's."""
    mesh, texs = ladder(width)
    kept, want = fused_pair(width, 16 * len(COUNTS), mesh, texs, pipe, ladder_views(3, width), path=path,
                            expect=ladder_oracle(pipe, width), interior=interior, lit=lit, frames_per_launch=3,
                            bin_capacity=LADDER_POOL, **FOUR_COLUMNS)
    assert len(kept) == 3
    assert_fused_parity(kept, want, pipe, _ladder_note(False), _ladder_note(True))


@pytest.mark.gpu
@pytest.mark.parametrize("pipe", ["phong", "shadow"])
@pytest.mark.parametrize("width", [125, 124])
@pytest.mark.parametrize("path", FUSED_PATHS)
def test_ladder_parity_general_form(built, path, width, pipe):
    """The ladder through the GENERAL four-wave column kernels of MODE 1 and MODE 2 -- FS_PHONG, FS_DEPTH, FS_SHADOW2: what
    a 1080p or a 4100 wide frame gets in that layout -- at widths with real partial tiles (LADDER_WIDTHS).  At 128 the
    same cases of test_ladder_parity run the interior form, so these are the only ones in which the general kernels meet a
    bin beyond their resident budget (NMAX 41 or 68 in the table above), the staging chunks' multiples and the empty
    chunks.  A failure names the tile and its n."""
    assert not H.expect_interior(width, 16 * len(COUNTS), pipe, 4, 1)
    _ladder_case(width, pipe, path, interior=False)


@pytest.mark.gpu
@pytest.mark.parametrize("width,pipe,force_lit,path",
                         [(w, p, f, path) for w in (LADDER_W, 125) for p, f in (("default", None), ("normal_map", "1"))
                          for path in FUSED_PATHS] + [(LADDER_W, "normal_map", "0", "group2")])
def test_ladder_parity_default_and_lit(built, monkeypatch, width, pipe, force_lit, path):
    """The ladder through the two closures whose interior form met short bins only: FS_DEFAULT, and FS_LIT -- normal_map
    on the lit-texel path (TR_LIT=1 as in test_lit_texel_path_on_small_frames; the profile must show k_lit) -- in the
    interior form at 128 and the general one at 125.  One more case takes normal_map OFF the lit path at 128: FS_NORMAL_MAP
    has no interior form, and the query must say so."""
    if force_lit is not None:
        monkeypatch.setenv("TR_LIT", force_lit)
    lit = (force_lit == "1") if pipe == "normal_map" else None
    interior = H.expect_interior(width, 16 * len(COUNTS), pipe, 4, 1, lit=bool(lit))
    assert interior == (width == LADDER_W and force_lit != "0")
    _ladder_case(width, pipe, path, interior, lit)


# ---- 4. the remaining MODE-0-only stress inputs get fused twins ------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("path", ["group2", "single2"])
@pytest.mark.parametrize("seed", FAR_SEEDS)
def test_far_vertices_and_slivers_fused(built, seed, path):
    """test_far_vertices_and_slivers_gpu's soups, sizes, layouts and pipelines (f32 rounding of the edge functions, the
    block rejection margins) through the fused kernels; a second light makes the frames of a group differ."""
    (W, Hh), waves, pipe, mesh, texs = far_case(seed)
    views = np.stack([view(0.0, 0.4), view(0.0, 0.9), view(0.0, 0.4)])
    expect = oracle_views(W, Hh, mesh, texs, pipe, views)
    assert all(o["err"] == 0 for o in expect), "the reference would panic on this soup"
    assert (expect[0]["winner"] != NO_WINNER).sum() > 1000
    mode = 1 + seed % 2
    # (seed 0 -- 8192 x 48, phong, 4 waves, columns -- runs the interior form; 4096 x 130 and 1000^2 have partial tiles)
    interior = H.expect_interior(W, Hh, pipe, waves, mode, lit=H.lit_path(W, Hh, texs, pipe))
    assert interior == (seed == 0)
    kept, want = fused_pair(W, Hh, mesh, texs, pipe, views, path=path, expect=expect, interior=interior, tile_waves=waves,
                            tile_mode=mode, frames_per_launch=3)
    assert_fused_parity(kept, want, pipe)


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["group2", "group1"])
@pytest.mark.parametrize("pipe", ["phong", "shadow"])
def test_many_polygons_in_one_tile_fused(built, pipe, path):
    """test_many_polygons_in_one_tile_render_the_first_time's sphere (20 088 polygons shrunk into the four tiles that meet
    in the middle of a 512x512 frame: thousands of records per bin, far beyond the shared key's slot field) in three views
    by ONE launch of each kernel per pass -- fused_pair asserts the launch counts: a second tile-kernel launch would be the
    frames rendered again after an overflow."""
    import tiny_renderer_amd as T
    mesh, texs = T.synthetic_scene(n_lat=62, n_lon=162, tex_size=256)
    mesh = dict(mesh, pos=(mesh["pos"] * np.float32(0.04)).astype(np.float32))
    views = np.stack([view(0.3, 0.2), view(0.0, 0.0), view(-0.4, 0.3)])
    kept, want = fused_pair(512, 512, mesh, texs, pipe, views, path=path, frames_per_launch=3)
    assert len(kept) == 3
    for o in want:
        ys, xs = np.nonzero(o["winner"] != NO_WINNER)
        tiles = {(int(x) // 128, int(y) // 16) for x, y in zip(xs, ys)}
        assert len(tiles) <= 6 and mesh["idx"].shape[0] // 2 // len(tiles) > 1500, len(tiles)
    assert_fused_parity(kept, want, pipe)


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["group2", "single2"])
@pytest.mark.parametrize("pipe", ["phong", "occlusion"])
def test_every_tile_heavy_fused(synthetic, pipe, path):
    """test_every_tile_heavy's two frames: the work list consists of its heaviest buckets only, no empty unit at all."""
    mesh, texs = synthetic
    for (W, Hh), a, b in (((256, 64), view(0.0, 0.0), view(0.0, 0.3)), ((384, 200), view(0.9, -0.4), view(0.0, 0.0))):
        kept, want = fused_pair(W, Hh, mesh, texs, pipe, np.stack([a, b, a]), path=path, frames_per_launch=3)
        assert_fused_parity(kept, want, pipe)


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["group2", "single2"])
@pytest.mark.parametrize("size", [(801, 603), (130, 70), (64, 64), (1, 1), (4100, 36)])
def test_ragged_sizes_fused(small_synthetic, size, path):
    """test_ragged_sizes' five sizes: widths that are not multiples of 4 / 16 / the tile take the byte-store paths."""
    mesh, texs = small_synthetic
    views = np.stack([view(0.2, 0.3), view(-0.5, 0.0), view(0.2, 0.3)])
    kept, want = fused_pair(size[0], size[1], mesh, texs, "phong", views, path=path, frames_per_launch=3)
    # (at 1x1 every vertex truncates to pixel (0, 0): every polygon is degenerate and the frame is the cleared one, whatever
    # the view -- the only case here that may be empty)
    assert_fused_parity(kept, want, "phong", allow_empty=(size == (1, 1)))


@pytest.mark.gpu
@pytest.mark.parametrize("pipe", ALL)
def test_instanced_group_matches_the_oracle(small_synthetic, pipe):
    """An instance table through a fused launch against the ORACLE rendering the host-built mesh apply_instances(mesh,
    table) (test_instancing.py compares instanced with replicated on the GPU: both sides the code under test)."""
    import tiny_renderer_amd as T
    mesh, texs = small_synthetic
    table = T.grid_instances(3)
    views = np.stack([view(0.3, 0.7), view(0.0, 0.2), view(0.3, 0.7), view(0.1, 0.4), view(0.0, 0.2)])
    kept, want = fused_pair(640, 480, mesh, texs, pipe, views, path="group2", oracle_mesh=T.apply_instances(mesh, table),
                            instances=table, frames_per_launch=4)
    assert len(kept) == 4
    assert_fused_parity(kept, want, pipe)
