"""The distance-field rule on the host: tr_distance_host against tests/distance_cases.py's all-pairs minimum in numpy,
the points that pin the cap, the integer square root over every field value, tr_distance_ramp_host against the ramp in
numpy, the refusals with their full texts, the builders, and the conditions of the GPU cases asserted on the oracle's
frames of those very cases.

Everything here needs no GPU.  tests/test_distance.py compares the device with tr_distance_host."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import distance_cases as DC
from tests import helpers as H
from tests import ramp_cases as RC

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAR = DC.FAR


@pytest.fixture(scope="module")
def T(built):
    import tiny_renderer_amd as T
    return T


def test_entry_points_declared_exported_and_typed(T):
    from tiny_renderer_amd import _lib
    header = open(os.path.join(REPO, "include", "tiny_renderer.h")).read()
    for word in ("} tr_distance_params;", "} tr_distance_ramp_params;", "#define TR_DIST_MAX_RADIUS 255u", "#define TR_DIST_FAR 0xFFFFu",
                 "#define TR_DIST_SEED_DRAWN 0u", "#define TR_DIST_SEED_KEY 1u", "#define TR_DIST_INVERT 0x1u", "#define TR_DIST_REPEAT 0x1u",
                 "#define TR_DIST_KEEP_SEEDS 0x2u", "#define TR_ABI_VERSION 3",
                 "int tr_scene_distance(tr_scene *s, const tr_distance_params *p, void *out);",
                 "int tr_scene_get_distance(tr_scene *s, const tr_distance_params *p, uint16_t *host);",
                 "int tr_scene_distance_ramp(tr_scene *s, const tr_distance_ramp_params *p, void *out /* or NULL */);",
                 "int tr_scene_get_distance_ramped(tr_scene *s, const tr_distance_ramp_params *p, uint8_t *rgb);"):
        assert word in header, word
    raw = C.CDLL(_lib.library_path())
    sigs = {"tr_scene_distance": [C.c_void_p] * 3, "tr_scene_get_distance": [C.c_void_p] * 3, "tr_scene_distance_ramp": [C.c_void_p] * 3,
            "tr_scene_get_distance_ramped": [C.c_void_p] * 3,
            "tr_distance_host": [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
            "tr_distance_ramp_host": [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p],
            "tr_distance_positions": [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]}
    for name, args in sigs.items():
        assert hasattr(raw, name), name + " is not exported"
        assert _lib.SYMBOLS[name] == (C.c_int, args), name
    # exports.map lets every tr_ name out and nothing else
    exports = open(os.path.join(REPO, "tiny_renderer_amd", "csrc", "exports.map")).read()
    assert "global: tr_*;" in exports and "local: *;" in exports
    assert C.sizeof(T.DistanceParams) == 32 and C.sizeof(T.DistanceRampParams) == 64
    assert T.load_library().tr_abi_version() == 3
    src = open(os.path.join(REPO, "tiny_renderer_amd", "csrc", "tr_scene.cpp")).read()
    assert "sizeof(tr_distance_params) == 32" in src and "sizeof(tr_distance_ramp_params) == 64" in src
    names = re.search(r"kKernelNames\[\] = \{([^}]*)\}", src).group(1)
    assert '"k_dist"' in names and '"k_dist_apply"' in names and len(names.split(",")) <= 32     # (Scene.profile_read reads 32 records)
    kernels = open(os.path.join(REPO, "tiny_renderer_amd", "csrc", "tr_kernels.hip")).read()
    for k in ("k_dist_mask", "k_dist_row", "k_dist", "k_dist_apply"):
        assert re.search(r"void %s\(" % k, kernels), k
    for name in ("distance_host", "distance_ramp_host", "distance_params", "distance_ramp_params", "distance_positions", "ramp_glow", "ramp_stroke",
                 "ramp_rings", "mask_dilate", "mask_erode", "DIST_FAR"):
        assert hasattr(T, name) and name in T.__all__, name
    for name in ("distance", "get_distance", "distance_ramp", "get_distance_ramped", "pinned_field"):
        assert callable(getattr(T.Scene, name)), name


def both_seed_kinds(T, mask, R, what):
    """tr_distance_host on a frame whose seeds are `mask`, under DRAWN and under KEY, with and without INVERT, against
    the all-pairs minimum."""
    rgb, z = DC.frame_of(mask, np.random.default_rng(mask.size))
    # (the all-pairs minimum grows with pixels times seeds: the complement of a sparse mask runs on the smaller frames)
    near, near_inv = DC.nearest_np(mask), DC.nearest_np(~mask) if mask.size <= DC.INVERT_PIXELS or 2 * mask.sum() > mask.size else None
    for radius in ([R] if isinstance(R, int) else R):
        want = DC.cap_np(near, radius)
        for seed, zz in (("drawn", z), ("key", z), ("key", None)):
            got = T.distance_host(rgb, zz, T.distance_params(radius, seed, 150))
            assert got.dtype == np.uint16 and got.shape == mask.shape
            assert np.array_equal(got, want), "%s R %d %s: %d values differ" % (what, radius, seed, int((got != want).sum()))
            if near_inv is not None:
                want_inv = DC.cap_np(near_inv, radius)
                got = T.distance_host(rgb, zz, T.distance_params(radius, seed, 150, invert=True))
                assert np.array_equal(got, want_inv), "%s R %d %s inverted: %d values differ" % (what, radius, seed, int((got != want_inv).sum()))


@pytest.mark.parametrize("W,Hh", DC.HOST_SIZES, ids=["%dx%d" % s for s in DC.HOST_SIZES])
def test_host_rule_equals_the_all_pairs_minimum(T, W, Hh):
    """A random 1 % mask (at least one seed) under every radius of the issue, both seed kinds, with and without INVERT."""
    rng = np.random.default_rng(W * 1000 + Hh)
    mask = rng.random((Hh, W)) < 0.01
    mask[rng.integers(0, Hh), rng.integers(0, W)] = True
    both_seed_kinds(T, mask, DC.HOST_RADII, "%d x %d" % (W, Hh))


@pytest.mark.parametrize("kind", DC.PATTERNS)
def test_planted_seed_patterns(T, kind):
    """Every planted pattern on frames that hold it: 384 x 48 has the mask-word and tile edges 63, 64, 127, 128 and room
    for two seeds 2 R + 1 apart along x; 40 x 300 has it along y.  The 50 % mask runs on the smaller frames: the all-pairs
    minimum grows with pixels times seeds."""
    rng = np.random.default_rng(len(kind))
    frames = ((131, 19), (256, 48)) if kind in ("half", "all") else ((384, 48), (40, 300), (131, 19))
    for W, Hh in frames:
        for R in (5, 16, 255) if kind != "half" else (2, 255):
            mask = DC.planted(kind, W, Hh, R, rng)
            both_seed_kinds(T, mask, R, "%s on %d x %d" % (kind, W, Hh))
    if kind == "none":
        f = T.distance_host(*DC.frame_of(np.zeros((19, 131), bool)), T.distance_params(255))
        assert (f == FAR).all(), "a frame without seeds is FAR everywhere"
    if kind == "all":
        f = T.distance_host(*DC.frame_of(np.ones((19, 131), bool)), T.distance_params(1))
        assert (f == 0).all(), "every pixel a seed"


def test_points_that_pin_the_cap(T):
    """One seed; the offsets of the issue.  Along x the row pass decides (255 exactly against none at R = 255), along y
    the column pass, and the diagonals both."""
    def field(R, W, Hh, sx, sy, seed="key"):
        mask = np.zeros((Hh, W), bool)
        mask[sy, sx] = True
        rgb, z = DC.frame_of(mask)
        return T.distance_host(rgb, z, T.distance_params(R, seed, 100))
    for seed in ("key", "drawn"):
        f = field(5, 20, 20, 7, 6, seed)
        assert f[6 + 4, 7 + 3] == 25 and f[6, 7 + 5] == 25 and f[6 + 1, 7 + 5] == FAR and f[6 + 5, 7] == 25 and f[6 + 5, 7 + 1] == FAR
        assert f[6, 7] == 0 and f[6, 7 - 5] == 25 and f[6 - 5, 7] == 25 and f[6, 7 - 6] == FAR
        f = field(255, 300, 300, 10, 20, seed)
        assert f[20 + 204, 10 + 153] == 65025 and f[20 + 180, 10 + 180] == 64800 and f[20 + 181, 10 + 181] == FAR
        assert f[20, 10 + 255] == 65025 and f[20, 10 + 256] == FAR and f[20 + 255, 10] == 65025 and f[20 + 256, 10] == FAR
        assert f[20 + 1, 10 + 255] == FAR and f[20 + 255, 10 + 1] == FAR
        # the same from the far corner: the seed lies to the right and below
        f = field(255, 300, 300, 290, 280, seed)
        assert f[280 - 204, 290 - 153] == 65025 and f[280, 290 - 255] == 65025 and f[280, 290 - 256] == FAR and f[280 - 255, 290] == 65025
        # R = 254: 254 is kept, 255 is not
        f = field(254, 300, 3, 10, 1, seed)
        assert f[1, 10 + 254] == 254 * 254 and f[1, 10 + 255] == FAR and f[0, 10 + 254] == FAR
    assert FAR == T.DIST_FAR == 0xFFFF and 255 * 255 < FAR


def test_the_integer_square_root_over_every_field_value_and_the_positions(T):
    d2 = np.arange(65026, dtype=np.uint32).astype(np.uint16)
    want = np.array([math.isqrt(int(v) << 16) for v in range(65026)], np.uint32)
    for step in (1, 256, 65536, 40000):
        dq, p = T.distance_positions(d2, step)
        assert np.array_equal(dq, want), "dq"
        ref = np.array([(int(q) * step) >> 8 for q in want], np.uint64)
        assert ref.max() < 2 ** 32 and np.array_equal(p.astype(np.uint64), ref), "p at step %d" % step
    assert want[-1] == 65280 and want[1] == 256 and want[2] == 362
    assert np.array_equal(DC.isqrt_np(d2.astype(np.int64) << 16), want.astype(np.int64)), "the numpy restatement"
    dq, p = T.distance_positions(np.array([65025], np.uint16), 65536)
    assert int(p[0]) == 65280 * 65536 >> 8 == 16711680
    from tiny_renderer_amd import _lib
    L = T.load_library()
    bad = np.array([65026], np.uint16)
    out = np.zeros(1, np.uint32)
    assert L.tr_distance_positions(256, 1, bad.ctypes.data, out.ctypes.data, None) == _lib.TR_E_INVALID
    assert L.tr_last_error().decode() == "tr_distance_positions: a field value above 65025 has no position"
    for step in (0, 65537):
        assert L.tr_distance_positions(step, 1, d2.ctypes.data, out.ctypes.data, None) == _lib.TR_E_INVALID
        assert L.tr_last_error().decode() == "tr_distance_positions: step must be 1..65536"


def ramp_frame(seed=3):
    """A random 61 x 45 frame around a drawn disc and a bright bar: seeds under either kind, pixels at every distance up
    to FAR."""
    rng = np.random.default_rng(seed)
    W, Hh = 61, 45
    rgb = rng.integers(0, 120, (Hh, W, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:Hh, 0:W]
    disc = (xx - 20) ** 2 + (yy - 18) ** 2 < 40
    z = np.where(disc, rng.random((Hh, W), np.float32), RC.F32_MIN).astype(np.float32)
    rgb[30:33, 40:55] = (250, 240, 130)
    return rgb, z


@pytest.mark.parametrize("mode", RC.MODES)
def test_ramp_host_equals_the_numpy_rule_in_every_byte(T, mode):
    rgb, z = ramp_frame()
    rng = np.random.default_rng(len(mode))
    for n, step in ((2, 20), (17, 256), (256, 3000), (1024, 65536)):
        tab = RC.random_table(rng, n)
        for opacity in (0, 77, 256):
            for seed, invert in (("drawn", False), ("key", False), ("drawn", True)):
                for repeat, keep, alpha in ((False, False, 0), (True, False, 130), (False, True, 255), (True, True, 255)):
                    R = 12 if n != 1024 else 255
                    field = DC.field_np(DC.seeds_np(rgb, z, seed, 200, invert), R)
                    far = DC.far_of(alpha)
                    want = DC.ramp_np(rgb, field, tab, step, mode, opacity, far, repeat, keep)
                    p = T.distance_ramp_params(R, step, seed, 200, invert, mode, opacity, far, repeat, keep)
                    got = T.distance_ramp_host(rgb, z, tab, p)
                    assert np.array_equal(got, want), (mode, n, step, opacity, seed, invert, repeat, keep, alpha)
                    # `out` aliased to `rgb`: the field is complete before a colour changes, KEY seeds included
                    assert np.array_equal(T.distance_ramp_host(rgb, z, tab, p, in_place=True), want), "in place"
                    if opacity == 0:
                        assert np.array_equal(want, rgb)


def test_the_facts_of_the_ramp(T):
    rgb, z = ramp_frame()
    mask = DC.seeds_np(rgb, z)
    field = DC.field_np(mask, 6)
    # keep_seeds: a glow around the model without touching it; far alpha 0 leaves what is out of reach
    tab, step = T.ramp_glow((255, 200, 40), 6)
    out = T.distance_ramp_host(rgb, z, tab, T.distance_ramp_params(6, step, keep_seeds=True, mode="add"))
    assert np.array_equal(out[mask], rgb[mask]) and np.array_equal(out[field == FAR], rgb[field == FAR])
    ring = (field > 0) & (field <= 4)
    assert (out[ring].astype(int) >= rgb[ring]).all() and (out[ring] != rgb[ring]).any()
    # a stroke: opaque up to the width under NORMAL
    tab, step = T.ramp_stroke((10, 20, 30), 3)
    out = T.distance_ramp_host(rgb, z, tab, T.distance_ramp_params(6, step, keep_seeds=True))
    assert (out[(field > 0) & (field <= 9)] == (10, 20, 30)).all() and np.array_equal(out[field >= 16], rgb[field >= 16])
    # rings under repeat: the wrap is seamless and the ring comes back every `spacing` pixels
    tab, step = T.ramp_rings((0, 0, 0), 4, 1)
    assert step == 256 and tab.shape == (5, 4) and tab[:, 3].tolist() == [255, 0, 0, 0, 255]
    out = T.distance_ramp_host(rgb, z, tab, T.distance_ramp_params(12, step, repeat=True))
    assert (out[(field == 16) | (field == 64)] == 0).all()
    # the thresholds of a field
    assert np.array_equal(T.mask_dilate(field, 3), DC.nearest_np(mask) <= 9)
    inner = T.distance_host(rgb, z, T.distance_params(6, invert=True))
    assert np.array_equal(T.mask_erode(inner, 2), DC.nearest_np(~mask) > 4)
    assert T.mask_erode(inner, 2).sum() < mask.sum() and not (T.mask_erode(inner, 2) & ~mask).any()


def test_refusals_with_their_full_texts(T):
    from tiny_renderer_amd import _lib
    L = T.load_library()
    rgb, z = ramp_frame()
    Hh, W, _ = rgb.shape
    out16 = np.full((Hh, W), 0xAAAA, np.uint16)
    out8 = np.full((Hh, W, 3), 0xAA, np.uint8)
    tab = RC.random_table(np.random.default_rng(1), 16)

    def text():
        return L.tr_last_error().decode()

    def fparams(seed=0, threshold=0, radius=4, flags=0, res=(0, 0, 0, 0)):
        return T.DistanceParams(seed, threshold, radius, flags, (C.c_uint32 * 4)(*res))

    def rparams(field=None, step=256, mode=0, opacity=256, far=0, flags=0, res=(0, 0, 0)):
        return T.DistanceRampParams(field or fparams(), step, mode, opacity, far, flags, (C.c_uint32 * 3)(*res))

    bad_field = ((dict(seed=2), ": seed must be TR_DIST_SEED_DRAWN or TR_DIST_SEED_KEY"), (dict(threshold=256), ": threshold must be 0..255"),
                 (dict(radius=0), ": radius must be 1..TR_DIST_MAX_RADIUS"), (dict(radius=256), ": radius must be 1..TR_DIST_MAX_RADIUS"),
                 (dict(flags=2), ": unknown flags"), (dict(res=(0, 0, 0, 1)), ": reserved must be 0"))
    bad_ramp = ((dict(step=0), ": step must be 1..65536"), (dict(step=65537), ": step must be 1..65536"),
                (dict(mode=7), ": mode must be TR_LAYER_NORMAL .. TR_LAYER_DIFFERENCE"), (dict(opacity=257), ": opacity must be 0..256"),
                (dict(flags=4), ": unknown flags"), (dict(res=(0, 1, 0)), ": reserved must be 0"))

    def host_field(p):
        return L.tr_distance_host(W, Hh, rgb.ctypes.data, z.ctypes.data, C.addressof(p) if p is not None else None, out16.ctypes.data)

    def host_ramp(p, n=16):
        return L.tr_distance_ramp_host(W, Hh, rgb.ctypes.data, z.ctypes.data, C.addressof(p) if p is not None else None, n, tab.ctypes.data, out8.ctypes.data)

    for kw, why in bad_field:
        assert host_field(fparams(**kw)) == _lib.TR_E_INVALID and text() == "tr_distance_host" + why, kw
        assert host_ramp(rparams(fparams(**kw))) == _lib.TR_E_INVALID and text() == "tr_distance_ramp_host" + why, kw
    for kw, why in bad_ramp:
        assert host_ramp(rparams(**kw)) == _lib.TR_E_INVALID and text() == "tr_distance_ramp_host" + why, kw
    assert host_field(None) == _lib.TR_E_INVALID and text() == "tr_distance_host: null argument"
    assert host_ramp(None) == _lib.TR_E_INVALID and text() == "tr_distance_ramp_host: null argument"
    for n in (1, 1025):
        assert host_ramp(rparams(), n) == _lib.TR_E_INVALID and text() == "tr_distance_ramp_host: the table's length n must be 2..TR_RAMP_MAX_N"
    good, key = fparams(), fparams(seed=1, threshold=9)
    assert L.tr_distance_host(0, Hh, rgb.ctypes.data, z.ctypes.data, C.addressof(good), out16.ctypes.data) == _lib.TR_E_INVALID
    assert text() == "tr_distance_host: the frame's width and height must be 1..32768"
    assert L.tr_distance_host(W, Hh, rgb.ctypes.data, None, C.addressof(good), out16.ctypes.data) == _lib.TR_E_INVALID
    assert text() == "tr_distance_host: null argument"
    assert L.tr_distance_host(W, Hh, None, None, C.addressof(key), out16.ctypes.data) == _lib.TR_E_INVALID and text() == "tr_distance_host: null argument"
    assert L.tr_distance_host(W, Hh, rgb.ctypes.data, None, C.addressof(key), None) == _lib.TR_E_INVALID and text() == "tr_distance_host: null argument"
    assert (out16 == 0xAAAA).all() and (out8 == 0xAA).all(), "a refused call wrote its output"
    # z may be NULL under KEY
    assert L.tr_distance_host(W, Hh, rgb.ctypes.data, None, C.addressof(key), out16.ctypes.data) == 0
    # the Python builders refuse the same in the same words
    for kw, why in ((dict(radius=0), "radius must be 1..TR_DIST_MAX_RADIUS"), (dict(radius=4, threshold=256), "threshold must be 0..255"),
                    (dict(radius=4, seed="colour"), "seed must be TR_DIST_SEED_DRAWN or TR_DIST_SEED_KEY")):
        with pytest.raises(ValueError, match=re.escape(why)):
            T.distance_params(**kw)
    for kw, why in ((dict(step=0), "step must be 1..65536"), (dict(opacity=300), "opacity must be 0..256"), (dict(mode="burn"), "mode must be"),
                    (dict(far=(1, 2, 3)), "far must be four values")):
        with pytest.raises(ValueError, match=re.escape(why)):
            T.distance_ramp_params(4, **kw)
    with pytest.raises(ValueError):
        T.distance_host(rgb, None, T.distance_params(4))
    with pytest.raises(ValueError):
        T.distance_host(rgb, z, T.distance_ramp_params(4))
    for call in (lambda: T.ramp_glow((1, 2, 3), 0), lambda: T.ramp_glow((1, 2, 3), 9, "cubic"), lambda: T.ramp_stroke((1, 2), 3),
                 lambda: T.ramp_rings((1, 2, 3), 4, 4), lambda: T.mask_dilate(np.zeros((2, 2), np.uint8), 1)):
        with pytest.raises(ValueError):
            call()


def test_the_builders(T):
    for radius in (1, 7, 24, 255):
        tab, step = T.ramp_glow((255, 200, 40, 180), radius, "smooth")
        assert tab.shape == (256, 4) and tab.dtype == np.uint8 and 1 <= step <= 65536
        assert tab[0].tolist() == [255, 200, 40, 180] and tab[-1, 3] == 0 and (np.diff(tab[:, 3].astype(int)) <= 0).all()
        # the last entry is reached at the radius and not a whole pixel before it
        _, p = T.distance_positions(np.array([radius * radius, (radius - 1) * (radius - 1)], np.uint16), step)
        assert p[0] >= 255 * 256 and (radius == 1 or p[1] < 255 * 256)
    for kind in ("linear", "exp"):
        tab, _ = T.ramp_glow((1, 2, 3), 10, kind)
        assert tab[0, 3] == 255 and tab[-1, 3] == 0
    tab, step = T.ramp_stroke((9, 8, 7, 200), 20)
    assert step == 256 and tab.shape == (22, 4) and (tab[:21, 3] == 200).all() and tab[21, 3] == 0


@pytest.mark.parametrize("W,Hh", DC.SIZES, ids=["%dx%d" % s for s in DC.SIZES])
def test_the_conditions_of_the_gpu_cases(T, small_synthetic, W, Hh):
    """The oracle's frame of each GPU case at R = 4 under DRAWN: seeds, near pixels and FAR pixels hold at least 1 % of
    the frame each, and a tile of the 128 x 16 grid is all FAR -- so the sphere cases are not empty.  On that frame the host
    rule equals the all-pairs minimum under both seed kinds."""
    from oracle import oracle as O
    mesh = T.apply_instances(small_synthetic[0], DC.table(W, Hh))
    s = O.Scene(W, Hh, mesh, small_synthetic[1], "phong")
    s.clear()
    s.set_light_direction(H.light(DC.LIGHT)), s.set_camera(*H.camera(DC.CAM)), s.render()
    z, fb = s.z_f32(), s.get_frame_buffer()
    s.close()
    field = T.distance_host(fb, z, T.distance_params(4))
    assert np.array_equal(field, DC.field_np(DC.seeds_np(fb, z), 4))
    n = W * Hh
    assert 100 * int((field == 0).sum()) >= n, "seeds hold %d of %d pixels" % (int((field == 0).sum()), n)
    assert 100 * int(((field > 0) & (field <= 16)).sum()) >= n, "near pixels"
    assert 100 * int((field == FAR).sum()) >= n, "FAR pixels"
    up = field[::-1]                                                     # (the tile grid counts rows from the bottom)
    tiles = [up[j:j + 16, i:i + 128] for j in range(0, Hh, 16) for i in range(0, W, 128)]    # (the grid's tiles, clipped by the frame)
    assert any((t == FAR).all() for t in tiles), "no 128 x 16 tile of the grid is all FAR"
    if W % 128:
        assert (up[:, W // 128 * 128:] == 0).any(), "no seed in the partial tile column"
    for thr in (1, 128):
        got = T.distance_host(fb, None, T.distance_params(16, "key", thr, invert=thr == 128))
        assert np.array_equal(got, DC.field_np(DC.seeds_np(fb, z, "key", thr, thr == 128), 16)), thr


@pytest.mark.skipif(shutil.which(os.environ.get("CXX", "g++")) is None, reason="no host C++ compiler")
def test_the_host_check_program_compiles_and_passes(tmp_path):
    """scripts/distance_host_check.cpp, built for the host without a sanitizer (the same program is what runs under
    -fsanitize=address,undefined by hand: its header has the line)."""
    exe = str(tmp_path / "distance_host_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-ffp-contract=off", "-I" + os.path.join(REPO, "include"),
                           "-I" + os.path.join(REPO, "tiny_renderer_amd", "csrc"), os.path.join(REPO, "scripts", "distance_host_check.cpp"), "-o", exe])
    done = subprocess.run([exe], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout + done.stderr
    m = re.search(r"distance: (\d+) roots, (\d+) fields, (\d+) ramps, 0 mismatches", done.stdout)
    assert m and int(m.group(1)) == 65026 and int(m.group(2)) >= 40 and int(m.group(3)) >= 40
