"""CPU side of the view / light / texture-shape table (tests/view_cases.py): the EXPECTED side of
tests/test_view_space_parity.py pinned independently, and the conditions on the table itself.

* the oracle against the numpy second restatement (tests/golden/second_opinion.py): every camera x pipeline x case
  light, every texture shape, the uv edges, random views, and the near-w soups at 320x200 where raster coordinates
  saturate and i32 differences really wrap (counted);
* the oracle against the host emulation (the product's stage functions through the kernels' decomposition) at <= 320x200
  over every group of the table, all seven pipelines; where the oracle reports a reference panic the emulation must
  report one too;
* the defined share: every designed case that must be defined is, at most one case in eight of any parametrised group of
  the GPU file is undefined upstream, every defined case covers enough pixels, and the view a scene renders after an
  undefined one (GOOD_VIEW) is defined on every mesh it is used with;
* the fixed seeds of the older soup tests that skip on an oracle error are all defined today: those skips are dead."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import emul_bind as E
from tests import view_cases as VC
from tests.test_fused_parity import ALL, NO_WINNER, TWO_PASS, oracle_views

SINGLE_PASS = ("default", "phong", "normal_map", "specular", "darboux")
# (camera, light, pipeline) cases of the sphere that are undefined upstream, exactly:
#   straddle_w0: w == 0 at the equator vertices, every pipeline and light;
#   straddle_moved: the light's view of fragments the camera sees through w < 0 leaves the shadow buffer.
UNDEFINED_SPHERE = {("straddle_w0", ln, p) for ln in VC.CASE_LIGHTS for p in ALL} | \
                   {("straddle_moved", ln, p) for ln in VC.CASE_LIGHTS for p in TWO_PASS}
UNDEFINED_DIABLO = {("elevated", "unit3d", p) for p in TWO_PASS}


@pytest.fixture(scope="module")
def sphere(built):
    import tiny_renderer_amd as T
    return T.synthetic_scene(n_lat=12, n_lon=24, tex_size=256)


def oracle_one(W, Hh, mesh, texs, pipe, q):
    return oracle_views(W, Hh, mesh, texs, pipe, [q])[0]


def emul_matches(W, Hh, mesh, texs, pipe, q, o):
    """The emulation's frame of view q is the oracle's, bit for bit; or both report a panic."""
    e, z, sh, fb, win = E.render(W, Hh, mesh, texs, pipe, list(q[0:3]), (list(q[3:6]), list(q[6:9]), list(q[9:12])))
    if o["err"]:
        assert e != 0, "the oracle reports %#x, the emulation nothing" % o["err"]
        return
    assert e == 0, "the emulation reports %#x, the oracle nothing" % e
    assert np.array_equal(win, o["winner"]), "winner differs at %d pixels" % int((win != o["winner"]).sum())
    assert np.array_equal(z.view(np.uint32), o["z"])
    if pipe in TWO_PASS:
        assert np.array_equal(sh.view(np.uint32), o["shadow"])
    assert np.array_equal(fb, o["rgb"])


def texture_case_undefined(shape, pipe):
    """The one texture case that is undefined upstream: darboux reads the smaller tangent map outside its range."""
    return shape == "tangent_smaller" and pipe == "darboux"


def share_ok(errs):
    """At most one case in eight of a group is undefined upstream."""
    bad = sum(1 for e in errs if e)
    assert 8 * bad <= len(errs), "%d of %d cases are undefined upstream" % (bad, len(errs))
    return bad


# ---- the table itself ------------------------------------------------------------------------------------------------

def test_table_is_what_it_claims():
    d = {k: float(np.linalg.norm(np.subtract(f, a))) for k, (f, a, u) in VC.CAMERAS.items()}
    assert abs(d["inside"] - 0.3) < 1e-6 and abs(d["distance3"] - 3.0) < 0.01 and 9.0 < d["distance10"] < 10.5
    assert np.linalg.norm(VC.CAMERAS["off_origin"][1]) > 0.5
    assert abs(np.linalg.norm(VC.CAMERAS["tilted_up"][2]) - 1.0) > 0.04
    lens = sorted(float(np.linalg.norm(v)) for v in VC.LIGHTS.values())
    assert lens[0] <= 0.26 and lens[-1] >= 5.9
    assert any(v[1] < 0 for v in VC.LIGHTS.values()) and any(v[2] < 0 for v in VC.LIGHTS.values())
    assert all(abs(v[1]) > 0.1 for v in VC.LIGHTS.values())       # none in the plane y = 0
    # w of a unit-sphere vertex: behind7 -- negative throughout; the straddles -- both signs
    for name, lo, hi in (("behind7", -0.6, -0.2), ("straddle", -0.1, 0.25), ("straddle_moved", -0.2, 0.2)):
        f, a, u = (np.array(v, np.float64) for v in VC.CAMERAS[name])
        nz = (f - a) / np.linalg.norm(f - a)
        w = [1.0 - float(np.dot(nz, p - f)) / 5.0 for p in (nz * 0.8, -nz * 0.8)]
        assert lo <= min(w) and max(w) <= hi, (name, w)
    for seed in range(40):
        q = VC.random_view(np.random.default_rng(seed))
        dist, off = np.linalg.norm(q[3:6] - q[6:9]), np.linalg.norm(q[6:9])
        cosang = abs(np.dot(q[9:12], q[3:6] - q[6:9])) / (np.linalg.norm(q[9:12]) * dist)
        assert 0.19 < dist < 12.1 and off <= 0.5001 and cosang < np.cos(np.radians(9.9))
        assert 0.249 < np.linalg.norm(q[0:3]) < 6.001
    mesh, _ = VC.near_w_soup(3)
    z = mesh["pos"][:, 2]
    assert (z == np.nextafter(np.float32(5), np.float32(0))).any() or (z == np.nextafter(np.float32(5), np.float32(10))).any()
    assert (z == np.float32(6.5)).sum() == 20
    mesh, texs = VC.uv_edge_mesh(True)
    assert (mesh["tex"][:, 0] == 0.0).any() and (mesh["tex"][:, 1] == 1.0).any() and (mesh["tex"][:, 1] == 0.0).any()
    u = mesh["tex"][:, 0] * np.float32(VC.UV_EDGE_SIDE)
    assert ((u > VC.UV_EDGE_SIDE - 1) & (u < VC.UV_EDGE_SIDE)).any()
    assert not (VC.uv_edge_mesh(False)[0]["tex"][:, 1] == 0.0).any()


# ---- cameras x lights x pipelines ------------------------------------------------------------------------------------

@pytest.mark.parametrize("pipe", ALL)
def test_cameras_defined_share_and_emulation(sphere, pipe):
    """At the GPU test's own size (640x400) the oracle's status of every camera x light case is the documented one; at
    320x200 the emulation equals the oracle for every case (or panics with it)."""
    mesh, texs = sphere
    for cam in VC.CAMERAS:
        for ln in VC.CASE_LIGHTS:
            q = VC.case_view(cam, ln)
            o = oracle_one(640, 400, mesh, texs, pipe, q)
            assert (o["err"] != 0) == ((cam, ln, pipe) in UNDEFINED_SPHERE), (cam, ln, pipe, hex(o["err"]))
            if not o["err"]:
                assert (o["winner"] != NO_WINNER).sum() >= 10000
            emul_matches(320, 200, mesh, texs, pipe, q, oracle_one(320, 200, mesh, texs, pipe, q))
    good = oracle_one(640, 400, mesh, texs, pipe, VC.GOOD_VIEW)
    assert good["err"] == 0 and (good["winner"] != NO_WINNER).sum() > 100


def test_antiparallel_light_is_singular(sphere):
    """The designed singular case of the GPU file: occlusion, light along -z -- the oracle reports the missing rotation for
    both cameras and the emulation reports a status too; every other pipeline is indifferent to it."""
    mesh, texs = sphere
    for cam in ("elevated", "rolled"):
        q = VC.view_row(VC.ANTIPARALLEL_LIGHT, VC.CAMERAS[cam])
        o = oracle_one(640, 400, mesh, texs, "occlusion", q)
        assert o["err"] & O.E_ROTATION
        emul_matches(320, 200, mesh, texs, "occlusion", q, o)
        assert oracle_one(640, 400, mesh, texs, "phong", q)["err"] == 0
    good = oracle_one(640, 400, mesh, texs, "occlusion", VC.GOOD_VIEW)
    assert good["err"] == 0


def test_cameras_undefined_share():
    n = len(VC.CAMERAS) * len(VC.CASE_LIGHTS) * len(ALL)
    assert 8 * len(UNDEFINED_SPHERE) <= n
    assert not any(c[0] in VC.DEFINED_CAMERAS and c[2] in SINGLE_PASS for c in UNDEFINED_SPHERE)
    assert 8 * len(UNDEFINED_DIABLO) <= len(VC.DIABLO_CAMERAS) * len(VC.CASE_LIGHTS) * len(ALL)


@pytest.mark.parametrize("pipe", ALL)
def test_diablo_cameras_defined_share(diablo, pipe):
    mesh, texs = diablo
    for cam in VC.DIABLO_CAMERAS:
        for ln in VC.CASE_LIGHTS:
            q = VC.case_view(cam, ln)
            o = oracle_one(800, 800, mesh, texs, pipe, q)
            assert (o["err"] != 0) == ((cam, ln, pipe) in UNDEFINED_DIABLO), (cam, ln, pipe, hex(o["err"]))
            if not o["err"]:
                assert (o["winner"] != NO_WINNER).sum() >= 10000
    good = oracle_one(800, 800, mesh, texs, pipe, VC.GOOD_VIEW)
    assert good["err"] == 0 and (good["winner"] != NO_WINNER).sum() > 100


class WrapCount:
    """second_opinion.wrap_i32 with a count of the differences it actually changed."""

    def __init__(self, S):
        self.inner, self.changed = S.wrap_i32, 0

    def __call__(self, d):
        r = self.inner(d)
        self.changed += int(np.count_nonzero(np.asarray(r) != np.asarray(d)))
        return r


def restatement_matches(W, Hh, mesh, texs, pipe, q, monkeypatch=None):
    """The numpy restatement's frame of view q is the oracle's (z bits, shadow bits, winner, rgb), or both panic.  Returns
    (oracle frame, number of i32 differences that wrapped in the restatement)."""
    from tests.golden import second_opinion as S
    o = oracle_one(W, Hh, mesh, texs, pipe, q)
    count = WrapCount(S)
    if monkeypatch is not None:
        monkeypatch.setattr(S, "wrap_i32", count)
    b = S.Scene(W, Hh, mesh, texs, pipe)
    b.clear()
    b.set_light_direction(q[0:3])
    b.set_camera(q[3:6], q[6:9], q[9:12])
    if o["err"]:
        with pytest.raises(S.Panic):
            b.render()
        return o, count.changed
    b.render()
    assert np.array_equal(b.buf["z"].view(np.uint32).reshape(Hh, W), o["z"])
    if pipe in TWO_PASS:
        assert np.array_equal(b.buf["shadow"].view(np.uint32).reshape(Hh, W), o["shadow"])
    assert np.array_equal(np.asarray(b.winner).reshape(Hh, W), o["winner"])
    assert np.array_equal(b.get_frame_buffer(), o["rgb"])
    return o, count.changed


@pytest.mark.parametrize("pipe", ALL)
@pytest.mark.parametrize("cam", list(VC.CAMERAS))
def test_second_restatement_agrees(built, cam, pipe):
    """Every camera x pipeline x both case lights at 96x60 on an 8 x 12 sphere; the status is the documented one."""
    import tiny_renderer_amd as T
    mesh, texs = T.synthetic_scene(n_lat=8, n_lon=12, tex_size=32)
    for ln in VC.CASE_LIGHTS:
        o, _ = restatement_matches(96, 60, mesh, texs, pipe, VC.case_view(cam, ln))
        # (whether a shadow-buffer lookup leaves the buffer depends on the frame's size and the mesh: only the single-pass
        # status is the one documented for the 640x400 cases)
        if pipe in SINGLE_PASS:
            assert (o["err"] != 0) == ((cam, ln, pipe) in UNDEFINED_SPHERE), (cam, ln, pipe, hex(o["err"]))
        if not o["err"]:
            assert (o["winner"] != NO_WINNER).sum() > 300
    if pipe == "occlusion":
        o, _ = restatement_matches(96, 60, mesh, texs, pipe, VC.view_row(VC.ANTIPARALLEL_LIGHT, VC.CAMERAS[cam]))
        assert o["err"] & O.E_ROTATION


@pytest.mark.parametrize("seed", [2, 5, 7, 4])
def test_second_restatement_where_differences_wrap(built, seed, monkeypatch):
    """The near-w soups at 320x200, where raster coordinates saturate to i32::MIN and the differences of
    to_barycentric_coord (scene.rs:178-186; a release build wraps) really wrap: counted, so that the agreement is not
    vacuous.  Seeds 2, 5, 7 are the ones the product's pair masks lost fragments on; 4 is undefined (w == 0)."""
    from tests.golden import second_opinion as S
    assert S.wrap_i32(2147483647 - (-2147483648)) == -1
    assert S.wrap_i32(-2147483648 - 5) == 2147483643
    assert S.wrap_i32(12 - 40) == -28
    mesh, texs = VC.near_w_soup(seed)
    wrapped = 0
    for k, q in enumerate(VC.near_w_views()):
        pipe = ("default", "phong", "normal_map")[(seed + k) % 3]
        o, n = restatement_matches(320, 200, mesh, texs, pipe, q, monkeypatch)
        assert (o["err"] != 0) == (seed == 4)
        wrapped += n
    assert seed == 4 or wrapped > 0, "no difference wrapped: the compare says nothing about wrapping"


@pytest.mark.parametrize("shape", list(VC.TEXTURE_SHAPES))
def test_second_restatement_texture_shapes(built, shape):
    """Every shape x pipeline x both texture views at 120x80: non-square and mixed-size images, and the tangent map indexed
    with coordinates scaled by normal_map's size (util.rs:60-64), larger (defined) and smaller (panics)."""
    import tiny_renderer_amd as T
    mesh, _ = T.synthetic_scene(n_lat=8, n_lon=12, tex_size=32)
    texs = VC.shape_textures(shape)
    for q in VC.texture_views():
        for pipe in VC.TEXTURE_PIPES:
            o, _ = restatement_matches(120, 80, mesh, texs, pipe, q)
            assert (o["err"] != 0) == texture_case_undefined(shape, pipe)


@pytest.mark.parametrize("with_v0", [False, True])
def test_second_restatement_uv_edges(built, with_v0):
    mesh, texs = VC.uv_edge_mesh(with_v0)
    for q in VC.uv_edge_views():
        for pipe in VC.TEXTURE_PIPES:
            o, _ = restatement_matches(160, 120, mesh, texs, pipe, q)
            assert (o["err"] != 0) == with_v0


@pytest.mark.parametrize("seed", VC.RANDOM_SEEDS[:14])
def test_second_restatement_random_views(sphere, seed):
    """Two pipelines' worth of random views (fourteen seeds: every pipeline twice), two views each, at 96x60."""
    import tiny_renderer_amd as T
    mesh, texs = T.synthetic_scene(n_lat=8, n_lon=12, tex_size=32)
    pipe, _, views = VC.random_case(seed)
    for q in views[:2]:
        restatement_matches(96, 60, mesh, texs, pipe, q)


# ---- near-zero and negative w ----------------------------------------------------------------------------------------

def test_near_w_soups(built):
    """Seven of the eight soups are defined, one has a vertex at w == 0 exactly; the emulation equals the oracle at 320x200
    and 1030x70 and no covered pixel lies outside the pair masks."""
    errs = []
    before = E.mask_counts()
    for seed in VC.NEAR_W_SEEDS:
        mesh, texs = VC.near_w_soup(seed)
        q, q2 = VC.near_w_views()
        o2 = oracle_one(320, 200, mesh, texs, "phong", q2)
        emul_matches(320, 200, mesh, texs, "phong", q2, o2)
        for k, pipe in enumerate(("default", "phong", "normal_map")):
            for W, Hh in ((320, 200), (1030, 70)):
                o = oracle_one(W, Hh, mesh, texs, pipe, q)
                if not o["err"]:
                    assert (o["winner"] != NO_WINNER).sum() >= 10000
                emul_matches(W, Hh, mesh, texs, pipe, q, o)
            errs.append(o["err"])
            # (the GPU test's sizes: the status does not depend on the size, the cover does)
            for W, Hh in ((4096, 130), (8192, 48)):
                if k == 0:
                    o2 = oracle_one(W, Hh, mesh, texs, pipe, q)
                    assert bool(o2["err"]) == bool(o["err"]) and (o["err"] or (o2["winner"] != NO_WINNER).sum() >= 10000)
        good = oracle_one(320, 200, mesh, texs, "phong", VC.GOOD_VIEW)
        assert good["err"] == 0 and (good["winner"] != NO_WINNER).sum() > 100
    assert share_ok(errs) == 3                      # seed 4, three pipelines
    assert E.mask_counts()[0] == before[0], "covered pixels outside the pair masks"


# ---- random sweep ----------------------------------------------------------------------------------------------------

def test_random_views_defined_share_and_emulation(sphere):
    mesh, texs = sphere
    errs = []
    for seed in VC.RANDOM_SEEDS:
        pipe, (W, Hh), views = VC.random_case(seed)
        for q in views:
            o = oracle_one(W, Hh, mesh, texs, pipe, q)
            errs.append(o["err"])
            if not o["err"]:
                assert (o["winner"] != NO_WINNER).sum() >= 2000
            if seed % 2 == 0:
                w, h = min(W, 320), min(Hh, 200)
                emul_matches(w, h, mesh, texs, pipe, q, oracle_one(w, h, mesh, texs, pipe, q))
    share_ok(errs)
    assert {VC.random_case(s)[0] for s in VC.RANDOM_SEEDS} == set(ALL)


# ---- texture shapes and uv edges -------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", list(VC.TEXTURE_SHAPES))
def test_texture_shapes_emulation(built, shape, monkeypatch):
    """Every shape x pipeline: defined except darboux with the smaller tangent map; the emulation (interleaved set where
    the images have one size, and plain images) equals the oracle."""
    import tiny_renderer_amd as T
    mesh, _ = T.synthetic_scene(n_lat=12, n_lon=24, tex_size=64)
    texs = VC.shape_textures(shape)
    assert [(t.shape[1], t.shape[0]) for t in texs] == VC.TEXTURE_SHAPES[shape]
    W, Hh = VC.TEXTURE_SIZE
    for q in VC.texture_views():
        for pipe in VC.TEXTURE_PIPES:
            o = oracle_one(W, Hh, mesh, texs, pipe, q)
            assert (o["err"] != 0) == texture_case_undefined(shape, pipe), (shape, pipe, hex(o["err"]))
            if not o["err"]:
                assert (o["winner"] != NO_WINNER).sum() >= 10000
            for plain in ("0", "1"):
                monkeypatch.setenv("TR_EMUL_PLAIN_TEXELS", plain)
                emul_matches(W, Hh, mesh, texs, pipe, q, o)
    for pipe in VC.TEXTURE_PIPES:
        if not texture_case_undefined(shape, pipe):
            continue
        good = oracle_one(W, Hh, mesh, texs, pipe, VC.GOOD_VIEW)
        assert good["err"] != 0     # (no view of this scene is defined: the GPU test expects the status again)


def test_texture_shapes_undefined_share():
    """(test_texture_shapes_emulation asserts that the oracle's status IS texture_case_undefined, case by case.)"""
    cases = [(s, p) for s in VC.TEXTURE_SHAPES for p in VC.TEXTURE_PIPES]
    assert 8 * sum(texture_case_undefined(s, p) for s, p in cases) <= len(cases)


@pytest.mark.parametrize("with_v0", [False, True])
def test_uv_edges(built, with_v0, monkeypatch):
    """(The v = 0 half of the uv-edge group is undefined by design -- the lookup out of range is what it is there for --
    and so is the antiparallel occlusion light: the two groups exempt from the one-in-eight rule.)"""
    mesh, texs = VC.uv_edge_mesh(with_v0)
    for q in VC.uv_edge_views():
        for pipe in VC.TEXTURE_PIPES:
            o = oracle_one(320, 240, mesh, texs, pipe, q)
            assert (o["err"] != 0) == with_v0
            assert bool(o["err"] & O.E_TEX_OOB) == with_v0
            if not with_v0:
                assert (o["winner"] != NO_WINNER).sum() >= 30000
            for plain in ("0", "1"):
                monkeypatch.setenv("TR_EMUL_PLAIN_TEXELS", plain)
                emul_matches(320, 240, mesh, texs, pipe, q, o)


def test_uv_edges_reach_the_border_texels(built):
    """With a one-colour border in the colour image, default-pipeline pixels of every border (column 0, the last column,
    row 0, the last row) appear in the frame: the corners of uv_edge_mesh reach them."""
    mesh, texs = VC.uv_edge_mesh(False)
    s = VC.UV_EDGE_SIDE
    img = np.zeros((s, s, 3), np.uint8)
    img[:, 0] = (255, 0, 0)
    img[:, s - 1] = (0, 255, 0)
    img[0, 1:s - 1] = (0, 0, 255)
    img[s - 1, 1:s - 1] = (255, 255, 0)
    o = oracle_one(320, 240, mesh, [img, texs[1], texs[2], texs[3]], "default", VC.view_row([0.0, 0.0, 1.0], VC.UV_EDGE_CAMERA))
    assert o["err"] == 0
    rgb = o["rgb"].reshape(-1, 3)
    for ch in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0)):
        hit = np.all((rgb > 0) == np.array(ch, bool), axis=1)
        assert hit.sum() > 50, "border %r is not reached" % (ch,)


# ---- the older soup tests' skips are dead ----------------------------------------------------------------------------

def test_fixed_soup_seeds_are_defined(built):
    """test_far_vertices_and_slivers_gpu, test_far_vertices_and_slivers_fused, test_resolve_matches_serial_order_gpu, its
    frame-group twin and test_pair_masks_never_lose_a_fragment skip (or assert) on an oracle error: with today's
    generators -- the tests' own (tie_case, tie_group_case, far_case and the seed ranges of test_random_meshes.py and
    test_emulation.py) -- none of their fixed seeds is undefined, so none of those skips is ever taken.
    test_resolve_matches_serial_order_cpu is a hypothesis test: it has no fixed seeds, its early return on an oracle
    error can be taken on any run and cannot be shown dead."""
    from tests import test_random_meshes as R
    from tests.test_emulation import MASK_SEEDS
    undefined = []
    for seed in R.FAR_SEEDS:
        (W, Hh), _, pipe, mesh, texs = R.far_case(seed)
        for la in (0.4, 0.9):           # (the gpu test's light, and the two of the fused twin)
            if R.oracle_frame(W, Hh, mesh, texs, pipe, 0.0, la)[0]:
                undefined.append(("far_case", seed, la))
    for seed in MASK_SEEDS:
        (W, Hh), _, _, mesh, texs = R.far_case(seed, base=7000)
        if R.oracle_frame(W, Hh, mesh, texs, "phong", 0.0, 0.4)[0]:
            undefined.append(("far_case 7000", seed))
    for seed in R.TIE_SEEDS:
        (W, Hh), pipe, ca, mesh, texs = R.tie_case(seed)
        if R.oracle_frame(W, Hh, mesh, texs, pipe, ca, 0.4)[0]:
            undefined.append(("tie_case", seed))
    for seed in R.TIE_GROUP_SEEDS:
        (W, Hh), pipe, views, mesh, texs = R.tie_group_case(seed)
        for ca, la in views:
            if R.oracle_frame(W, Hh, mesh, texs, pipe, ca, la)[0]:
                undefined.append(("tie_group_case", seed, ca, la))
    assert undefined == [], "seeds on which those tests skip today: %r" % (undefined,)
