"""GPU parity over general cameras, lights and texture shapes (the table of tests/view_cases.py).

Every other GPU test draws its views from helpers.camera / helpers.light: a camera on the unit circle of the plane y = 0
looking at the origin with up = (0, 1, 0) and a unit light in the same plane -- w of every vertex inside [1.0, 1.4] -- and
four square power-of-two images of one size.  Here: elevated, tilted, rolled, near (inside the mesh) and far cameras,
cameras that look AWAY from the mesh (w < 0: raster coordinates that saturate, i32 differences that wrap) or whose plane
w = 0 cuts it, 3-D lights of length 0.25 ... 6 (the depth pass's camera distance), images that are not square, not a
multiple of the interleaved set's blocks, 1 x 1, or of different sizes (the plain texel path), and uv that reach texel
column 0 and the last column / row exactly.

Every compare is bit equality with the CPU oracle -- winner where the scene has a tap, z bits, shadow bits, rgb -- through
assert_fused_parity (specular: exact where the build has the exact powf, else 1 LSB; the rule of test_gpu_parity.py), by
the four paths of test_fused_parity.py: tap0 (per-frame kernel, MODE 0, winner compared), group2, group1, single2.

Undefined cases are asserted, never skipped: where the oracle reports a reference panic the library must report the
matching status (TR_E_OOB_LOOKUP from tr_scene_sync or a getter for w == 0 / a texture or shadow lookup out of range;
TR_E_SINGULAR from the call that upstream would panic in) and stay usable: a defined frame rendered afterwards on the same
scene matches the oracle.  tests/test_view_space_cpu.py asserts on the CPU which cases of the table are defined and that at
most one in eight of any group is not.  Shadow / occlusion subset: the two case lights ("unit3d", "longest") keep every
shadow-buffer lookup inside for all designed cameras except "straddle_moved" (undefined for both lights, asserted as such);
"straddle_w0" is undefined for every pipeline (w == 0 at the equator vertices)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import helpers as H
from tests import view_cases as VC
from tests.test_fused_parity import (ALL, FUSED_PATHS, NO_WINNER, TWO_PASS, _grab, _tile_launches, _where,
                                     assert_fused_parity, fused_pair, oracle_views)

PATHS = ("tap0",) + FUSED_PATHS
SIGNALS = (-6, -11, -9, -15, 124, 134, 137, 139)    # a child that aborted, faulted or ran into its time limit
GOOD_VIEW = VC.GOOD_VIEW


def _set_view(s, q):
    s.set_light_direction(q[0:3])
    s.set_camera(q[3:6], q[6:9], q[9:12])


def _tap0(W, Hh, mesh, texs, pipe, views, expect, one_launch=False, **opts):
    """The per-frame kernel with a winner tap (MODE 0): every distinct view against the oracle, winner included."""
    import tiny_renderer_amd as T
    gpu = T.Scene(W, Hh, mesh, texs, pipe, winner_tap=True, **opts)
    for i, (q, o) in enumerate(zip(views, expect)):
        if any(q.tobytes() == p.tobytes() for p in views[:i]):
            continue
        gpu.profile_enable(True)
        gpu.clear()
        _set_view(gpu, q)
        gpu.render()
        assert gpu.sync() == 0
        if one_launch:
            ran = _tile_launches(gpu.profile_read())
            n_pass = 2 if pipe in TWO_PASS else 1
            assert ran["k_tile"][0] + ran["k_tile_depth"][0] == n_pass and ran["k_bin"][0] == n_pass, ran
        gpu.profile_enable(False)
        wg = gpu.read_winner_u32()
        assert np.array_equal(wg, o["winner"]), "winner differs at %s" % _where(wg != o["winner"], None)
        assert_fused_parity([_grab(gpu, pipe)], [o], pipe, allow_empty=True)
    gpu.close()


def assert_reports_panic(W, Hh, mesh, texs, pipe, q, o, path, good=None, **opts):
    """The reference would panic on view `q` (oracle status o["err"]): the library must report the matching status -- from
    the render call for a singular camera, from tr_scene_sync / a getter for a lookup out of range or w == 0 -- and a
    defined frame rendered afterwards on the same scene must match the oracle."""
    import tiny_renderer_amd as T
    from tiny_renderer_amd import _lib
    from oracle import oracle as O
    assert o["err"] != 0
    singular = bool(o["err"] & (O.E_SINGULAR | O.E_ROTATION | O.E_VEC_W_NONZERO))
    want = _lib.TR_E_SINGULAR if singular else _lib.TR_E_OOB_LOOKUP
    if good is None:
        good = oracle_views(W, Hh, mesh, texs, pipe, [GOOD_VIEW])[0]
    # (a scene on which the ordinary view is undefined too -- a texture lookup that leaves its image wherever the mesh is
    # seen from -- must report its status again instead)
    assert good["err"] != 0 or (good["winner"] != NO_WINNER).sum() > 100
    group = path in ("group2", "group1")
    kw = dict(winner_tap=True) if path == "tap0" else dict(auto_group=False) if path == "single2" else \
        dict(store_depth=(path == "group1"), frames_per_launch=3)
    gpu = T.Scene(W, Hh, mesh, texs, pipe, **kw, **opts)
    issued = False
    with pytest.raises(T.TinyRendererError) as e:
        if group:
            gpu.render_frames(np.stack([q, q]))
        else:
            gpu.clear()
            _set_view(gpu, q)
            gpu.render()
        issued = True
        gpu.sync()
        gpu.get_frame_buffer()
    assert e.value.code == want, "oracle status %#x, library status %d (%s)" % (o["err"], e.value.code, e.value)
    assert issued != singular, "a singular view is refused by the call itself, a lookup out of range by sync / the getters"
    if singular:
        # (the failure is also the frame's status, as test_render_frames_arguments_and_a_singular_camera shows: one sync
        # reports it, or has nothing to report where the call itself queued nothing)
        try:
            gpu.sync()
        except T.TinyRendererError as again:
            assert again.code == want
    # ... and the scene stays usable
    for _ in range(2 if good["err"] else 1):
        try:
            if group:
                gpu.render_frames(np.stack([GOOD_VIEW, GOOD_VIEW]))
            else:
                gpu.clear()
                _set_view(gpu, GOOD_VIEW)
                gpu.render()
            status = gpu.sync()
        except T.TinyRendererError as again:
            status = again.code
        assert status == (want if good["err"] else 0)
    if not good["err"]:
        if group:
            gpu.select_frame(0)
        assert_fused_parity([_grab(gpu, pipe)], [good], pipe, allow_empty=True)
    gpu.close()


def check_views(W, Hh, mesh, texs, pipe, views, path, expect=None, min_cover=1000, one_launch=False, **opts):
    """`views` through one of PATHS against the oracle; the undefined ones through assert_reports_panic.  one_launch: no pass
    may have been rendered twice (fused_pair asserts that for its paths by itself)."""
    views = np.ascontiguousarray(views, np.float32).reshape(-1, 12)
    if expect is None:
        expect = oracle_views(W, Hh, mesh, texs, pipe, views)
    ok = [i for i, o in enumerate(expect) if o["err"] == 0]
    for i, o in enumerate(expect):
        if o["err"] == 0:
            assert (o["winner"] != NO_WINNER).sum() >= min_cover, "view %d covers too little to prove anything" % i
        elif not any(views[i].tobytes() == views[k].tobytes() for k in range(i)):
            assert_reports_panic(W, Hh, mesh, texs, pipe, views[i], o, path, **opts)
    if not ok:
        return
    v, x = views[ok], [expect[i] for i in ok]
    if path == "tap0":
        _tap0(W, Hh, mesh, texs, pipe, v, x, one_launch=one_launch, **opts)
        return
    kept, want = fused_pair(W, Hh, mesh, texs, pipe, v, path=path, expect=x, frames_per_launch=max(len(v), 2), **opts)
    # (allow_empty: a frame may be lit from behind and black throughout; the cover is asserted from the winner above)
    assert_fused_parity(kept, want, pipe, allow_empty=True)


# ---- 1. cameras x lights x pipelines ---------------------------------------------------------------------------------

_oracle_cache = {}


def camera_case(model, mesh, texs, size, cam, pipe):
    """Views light A, light B, light A of a camera, and the oracle's frames for them (once per session)."""
    key = (model, cam, pipe)
    if key not in _oracle_cache:
        a, b = (VC.case_view(cam, ln) for ln in VC.CASE_LIGHTS)
        views = np.stack([a, b, a])
        _oracle_cache[key] = (views, oracle_views(size, size if model == "diablo" else size * 5 // 8, mesh, texs, pipe, views))
    return _oracle_cache[key]


@pytest.mark.gpu
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("pipe", ALL)
@pytest.mark.parametrize("cam", list(VC.CAMERAS))
def test_cameras_and_lights(small_synthetic, cam, pipe, path):
    """Every camera of the table x every pipeline x the two case lights at 640x400 on the small sphere; the lights are
    two frames of one fused launch."""
    mesh, texs = small_synthetic
    views, expect = camera_case("sphere", mesh, texs, 640, cam, pipe)
    check_views(640, 400, mesh, texs, pipe, views, path, expect=expect, min_cover=10000)


@pytest.mark.gpu
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("pipe", ALL)
@pytest.mark.parametrize("cam", VC.DIABLO_CAMERAS)
def test_cameras_and_lights_diablo(diablo, cam, pipe, path):
    """Four of the cameras (elevated, distance 3, inside, behind-7) on diablo at 800x800."""
    mesh, texs = diablo
    views, expect = camera_case("diablo", mesh, texs, 800, cam, pipe)
    check_views(800, 800, mesh, texs, pipe, views, path, expect=expect, min_cover=10000)


# ---- 2. near-zero and negative w -------------------------------------------------------------------------------------

NEAR_W_SIZES = ((320, 200), (1030, 70), (4096, 130), (8192, 48))
NEAR_W_PIPES = ("default", "phong", "normal_map")


def pool_from_oracle(o, W, Hh):
    """A pool no pass can overflow: the polygons the oracle kept (its tri_kept count) times the 128 x 16 tiles of the
    frame -- every kept polygon in every tile -- plus 64."""
    return int(o["tri_kept"]) * ((W + 127) // 128) * ((Hh + 15) // 16) + 64


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("waves", [4, 8, 16])
@pytest.mark.parametrize("seed", VC.NEAR_W_SEEDS)
def test_near_zero_and_negative_w(built, seed, waves, mode):
    """near_w_soup: vertices at w = +-1 ulp around 0, +-2e-5 and -0.3 -- raster coordinates up to saturation, wrapping i32
    differences in edge_setup, a pixel term that is not linear in the pixel where pair_masks and the 8x8 block rejection
    assume it is.  Size rotates with the seed, pipeline with seed and waves; all four paths; these polygons cover every
    tile, so bin_capacity is pinned from the oracle's counts and the profile must show ONE launch per kernel and pass."""
    W, Hh = NEAR_W_SIZES[seed % 4]
    pipe = NEAR_W_PIPES[(seed + waves // 8) % 3]
    mesh, texs = VC.near_w_soup(seed)
    views = VC.near_w_views()
    expect = oracle_views(W, Hh, mesh, texs, pipe, views)
    pool = pool_from_oracle(expect[0], W, Hh)
    for path in PATHS:
        check_views(W, Hh, mesh, texs, pipe, views, path, expect=expect, min_cover=10000, one_launch=True,
                    tile_waves=waves, tile_mode=mode, bin_capacity=pool)


@pytest.mark.gpu
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("pipe", ["shadow", "darboux"])
def test_sphere_behind_the_camera(small_synthetic, pipe, mode, path):
    """The behind-camera sphere (w < 0 throughout: every polygon's box is the whole frame) in shadow and darboux with the
    pools pinned: one launch per kernel and pass in both resolves."""
    mesh, texs = small_synthetic
    W, Hh = 320, 200
    views = np.stack([VC.case_view("behind7", "unit3d"), VC.case_view("behind7", "longest")])
    expect = oracle_views(W, Hh, mesh, texs, pipe, views)
    assert all(o["err"] == 0 for o in expect)
    pool = mesh["idx"].shape[0] * ((W + 127) // 128) * ((Hh + 15) // 16) + 64
    check_views(W, Hh, mesh, texs, pipe, views, path, expect=expect, min_cover=W * Hh, one_launch=True, tile_waves=8,
                tile_mode=mode, bin_capacity=pool)


# ---- 3. random sweep -------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("seed", VC.RANDOM_SEEDS)
def test_random_views(small_synthetic, seed):
    """Five random views per seed (look_from 0.2 ... 12 from a look_at off the origin, any up, lights 0.25 ... 6 long) as ONE
    render_frames call of mixed views: the frames of a fused launch have different matrices.  Pipeline, size and path
    rotate with the seed; tap0 runs for every seed as well."""
    mesh, texs = small_synthetic
    pipe, (W, Hh), views = VC.random_case(seed)
    expect = oracle_views(W, Hh, mesh, texs, pipe, views)
    for path in ("tap0", FUSED_PATHS[seed % 3]):
        check_views(W, Hh, mesh, texs, pipe, views, path, expect=expect, min_cover=2000)


# ---- 4. texture shapes: a fresh child process per environment leg ----------------------------------------------------
#
# TR_PLAIN_TEXELS is read once per process and TR_LIT when a scene is made: each leg runs in a child of its own.
#   packed  TR_LIT=0            the interleaved set where the four images have one size, the closures per fragment
#   plain   TR_PLAIN_TEXELS=1   image by image for every shape
#   lit     TR_LIT=1            k_lit for the normal-map and specular closures where there is a set
LEGS = {"packed": {"TR_LIT": "0"}, "plain": {"TR_PLAIN_TEXELS": "1"}, "lit": {"TR_LIT": "1"}}
LIT_PIPES = ("normal_map", "specular")
_leg_results = {}


def leg_cases(leg):
    return [(shape, pipe) for shape in VC.TEXTURE_SHAPES for pipe in (LIT_PIPES if leg == "lit" else VC.TEXTURE_PIPES)]


def texture_leg_worker(leg, out_path):
    """Runs in the child: every shape x pipeline of a leg through all paths; writes {"shape/pipe": "ok" | failure text}."""
    import traceback
    import tiny_renderer_amd as T
    mesh, _ = T.synthetic_scene(n_lat=12, n_lon=24, tex_size=64)
    W, Hh = VC.TEXTURE_SIZE
    views = VC.texture_views()
    out = {}
    for shape, pipe in leg_cases(leg):
        texs = VC.shape_textures(shape)
        same = len(set(VC.TEXTURE_SHAPES[shape])) == 1
        try:
            expect = oracle_views(W, Hh, mesh, texs, pipe, views)
            for path in PATHS:
                check_views(W, Hh, mesh, texs, pipe, views, path, expect=expect, min_cover=10000)
            # k_lit runs exactly when forced AND the images have one size (no set, no lit path)
            gpu = T.Scene(W, Hh, mesh, texs, pipe, winner_tap=True)
            gpu.profile_enable(True)
            gpu.clear()
            _set_view(gpu, GOOD_VIEW)
            gpu.render()
            try:
                gpu.sync()
            except T.TinyRendererError:
                assert expect[0]["err"] != 0    # (a scene without a defined view: only the launch count matters here)
            lit = gpu.profile_read().get("k_lit", {"launches": 0})["launches"]
            gpu.close()
            want_lit = 1 if (leg == "lit" and pipe in LIT_PIPES and same) else 0
            assert lit == want_lit, "k_lit launches: %d, expected %d" % (lit, want_lit)
            out["%s/%s" % (shape, pipe)] = "ok"
        except Exception:
            out["%s/%s" % (shape, pipe)] = traceback.format_exc()
        with open(out_path, "w") as f:
            json.dump(out, f)


def run_leg(leg, tmp_dir):
    """The child of a leg is started ONCE per session, whatever becomes of it: its outcome -- a time limit and any other
    exception included -- is cached before anything can raise.  After a child that ended by a signal or ran into its time
    limit no further child is started (the card may be in a bad state): the remaining legs fail without running."""
    if leg in _leg_results:
        return _leg_results[leg]
    stopped = [k for k, r in _leg_results.items() if r[0] in SIGNALS or r[0] is None]
    if stopped:
        _leg_results[leg] = (None, "not started: the child of leg %s ended abnormally (%r)" % (stopped[0], _leg_results[stopped[0]][0]), {})
        return _leg_results[leg]
    _leg_results[leg] = (None, "the child of leg %s was started and its outcome never recorded" % leg, {})
    out_path = os.path.join(str(tmp_dir), "leg_%s.json" % leg)
    env = {k: v for k, v in os.environ.items() if k not in ("TR_LIT", "TR_PLAIN_TEXELS")}
    env.update(LEGS[leg])
    code = "import sys; from tests.test_view_space_parity import texture_leg_worker as w; w(sys.argv[1], sys.argv[2])"
    try:
        p = subprocess.run([sys.executable, "-c", code, leg, out_path], cwd=H.REPO, env=env, timeout=300,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        status, tail = p.returncode, p.stdout[-4000:]
    except subprocess.TimeoutExpired as e:      # (subprocess.run has killed the child and waited for it)
        out = e.stdout.decode(errors="replace") if isinstance(e.stdout, bytes) else (e.stdout or "")
        status, tail = 124, "time limit of 300 s reached\n" + out[-4000:]
    except Exception as e:
        status, tail = None, "the child could not be run: %r" % (e,)
    res = {}
    try:
        if os.path.isfile(out_path):
            with open(out_path) as f:
                res = json.load(f)
    except Exception as e:
        tail += "\n(result file unreadable: %r)" % (e,)
    _leg_results[leg] = (status, tail, res)
    return _leg_results[leg]


@pytest.fixture(scope="module")
def leg_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("texture_legs")


@pytest.mark.gpu
@pytest.mark.parametrize("leg,shape,pipe", [(leg, s, p) for leg in LEGS for (s, p) in leg_cases(leg)])
def test_texture_shapes(built, leg_dir, leg, shape, pipe):
    """Every TEXTURE_SHAPES entry x {default, phong, normal_map, specular, darboux, shadow} x {interleaved set, plain
    images, lit path where it applies}, two views, all four paths, in a child process per leg; the profile shows k_lit
    exactly when it is forced and the images have one size."""
    code, tail, res = run_leg(leg, leg_dir)
    assert code == 0, "the child of leg %s ended with status %r:\n%s" % (leg, code, tail)
    assert res.get("%s/%s" % (shape, pipe)) == "ok", res.get("%s/%s" % (shape, pipe), "no result:\n" + tail)


# ---- 5. uv edges -----------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("pipe", VC.TEXTURE_PIPES)
@pytest.mark.parametrize("with_v0", [False, True])
def test_uv_edges(built, with_v0, pipe, path):
    """uv_edge_mesh: u = 0 exactly, the last column and row, row 0 through v = 1 -- bit for bit, under three lights; with the
    v = 0 corner (1 - v = 1.0: the row index is the image's height) both sides report the lookup out of range.  (The
    v = 0 half of this group is undefined by design: the one group exempt from the one-in-eight rule.)"""
    mesh, texs = VC.uv_edge_mesh(with_v0)
    views = VC.uv_edge_views()
    expect = oracle_views(320, 240, mesh, texs, pipe, views)
    assert all((o["err"] != 0) == with_v0 for o in expect)
    check_views(320, 240, mesh, texs, pipe, views[:1] if with_v0 else views, path, expect=expect[:1] if with_v0 else expect,
                min_cover=30000)


# ---- 6. the designed singular case -----------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("cam", ["elevated", "rolled"])
def test_occlusion_antiparallel_light_is_singular(small_synthetic, cam, path):
    """Occlusion under a light along -z: rotation_between((0, 0, 1), light) does not exist and the reference's unwrap()
    panics (shader.rs:921), whatever the camera.  TR_E_SINGULAR from the render call itself, by every path, and the scene
    renders an ordinary view afterwards.  (Undefined by design, like the v = 0 corner: exempt from the one-in-eight rule.)"""
    from oracle import oracle as O
    mesh, texs = small_synthetic
    q = VC.view_row(VC.ANTIPARALLEL_LIGHT, VC.CAMERAS[cam])
    o = oracle_views(640, 400, mesh, texs, "occlusion", [q])[0]
    assert o["err"] & O.E_ROTATION
    assert_reports_panic(640, 400, mesh, texs, "occlusion", q, o, path)
