"""Outlines on the host: tr_outline_host and tr_outline_kinds against the rule in numpy and against answers written out by
hand, every refusal with its text, and the proof that the GPU cases of tests/test_outline.py are not vacuous.

The rule, from the words of include/tiny_renderer.h, is restated in tests/outline_cases.py.  The contract is exact, so
every comparison is np.array_equal."""
import ctypes as C
import fnmatch
import os
import re

import numpy as np
import pytest

from tests import helpers as H
from tests import outline_cases as OC

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32_MIN = OC.F32_MIN
SIL, STEP, CREASE = OC.SIL, OC.STEP, OC.CREASE
NAMES = ("tr_scene_outline", "tr_scene_get_outlined", "tr_outline_host", "tr_outline_kinds")


def test_entry_points_declared_exported_and_typed(built):
    import tiny_renderer_amd as T
    from tiny_renderer_amd import _lib
    from tiny_renderer_amd.scene import OutlineParams
    header = open(os.path.join(REPO, "include", "tiny_renderer.h")).read()
    assert re.search(r"int\s+tr_scene_outline\(tr_scene \*s, const tr_outline_params \*p, void \*out", header)
    assert re.search(r"int\s+tr_scene_get_outlined\(tr_scene \*s, const tr_outline_params \*p, uint8_t \*rgb\);", header)
    assert re.search(r"int\s+tr_outline_host\(uint32_t width, uint32_t height, const float \*z", header)
    assert re.search(r"int\s+tr_outline_kinds\(uint32_t width, uint32_t height, const float \*z, const tr_outline_params \*p, uint8_t \*kinds\);", header)
    for word in ("#define TR_OUTLINE_MAX_RADIUS 3", "#define TR_OUTLINE_CREASES 0x1u", "#define TR_OUTLINE_ONLY    0x2u",
                 "} tr_outline_params;", "#define TR_ABI_VERSION 3"):
        assert word in header, word
    exports = open(os.path.join(REPO, "tiny_renderer_amd", "csrc", "exports.map")).read()
    patterns = re.search(r"global:([^}]*?)local:", exports, re.S).group(1).replace(";", " ").split()
    raw = C.CDLL(_lib.library_path())
    for name in NAMES:
        assert any(fnmatch.fnmatchcase(name, p) for p in patterns), name + " is not in exports.map"
        assert hasattr(raw, name), name + " is not exported"
        assert name in _lib.SYMBOLS
    assert _lib.SYMBOLS["tr_scene_outline"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p])
    assert _lib.SYMBOLS["tr_scene_get_outlined"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p])
    assert _lib.SYMBOLS["tr_outline_host"] == (C.c_int, [C.c_uint32, C.c_uint32] + [C.c_void_p] * 4)
    assert _lib.SYMBOLS["tr_outline_kinds"] == (C.c_int, [C.c_uint32, C.c_uint32] + [C.c_void_p] * 3)
    for name in ("outline_host", "outline_kinds", "outline_params", "OutlineParams"):
        assert name in T.__all__ and hasattr(T, name), name
    assert callable(T.Scene.outline) and callable(T.Scene.get_outlined)
    assert C.sizeof(OutlineParams) == 32
    assert T.load_library().tr_abi_version() == 3 and T.load_library().tr_pipeline_count() == 7


def planted_field(W, Hh, seed):
    """Patches of smooth depth with steps between them, undrawn pixels singly and in patches, NaN and infinities."""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:Hh, 0:W].astype(np.float32)
    z = (50.0 + 0.75 * xs - 0.5 * ys + rng.normal(0.0, 0.4, (Hh, W))).astype(np.float32)
    z[:, W // 2:] += np.float32(9.0)
    z[Hh // 3:2 * Hh // 3, W // 4:W // 4 + 7] -= np.float32(15.0)
    z[rng.random((Hh, W)) < 0.08] = F32_MIN
    z[2:9, W - 12:W - 4] = F32_MIN
    z[Hh - 3:, :5] = F32_MIN
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    for k, v in enumerate((nan, inf, -inf, nan, np.finfo(np.float32).max)):
        z[1 + 3 * k, 4 + k] = v
        z[Hh - 2 - 3 * k, W - 3 - 2 * k] = v
    z[0, 0], z[0, W - 1], z[Hh - 1, W - 1] = nan, inf, np.float32(60.0)
    return z


@pytest.mark.parametrize("W,Hh", [(37, 23), (130, 19)])
def test_host_rule_equals_the_numpy_rule(built, W, Hh):
    import tiny_renderer_amd as T
    rng = np.random.default_rng(W)
    z = planted_field(W, Hh, W + Hh)
    rgb = rng.integers(0, 256, (Hh, W, 3), dtype=np.uint8)
    keep_z, keep_rgb = z.copy(), rgb.copy()
    seen = 0
    for step, crease in ((1.0, None), (1.0, 0.5), (0.0, 0.0), (12.0, 3.0)):
        want_k = OC.kinds_np(z, step, crease)
        got_k = T.outline_kinds(z, T.outline_params(depth_step=step, crease=crease))
        assert np.array_equal(got_k, want_k), "kinds at %r: %d differ" % ((step, crease), int((got_k != want_k).sum()))
        seen |= int(np.bitwise_or.reduce(want_k.reshape(-1)))
        for radius in (0, 1, 2, 3):
            for only in (False, True):
                for opacity in (0, 100, 256):
                    kw = dict(radius=radius, depth_step=step, crease=crease, ink=OC.INK, opacity=opacity, only=only, paper=OC.PAPER)
                    want = OC.rule_np(z, rgb, **kw)
                    got = T.outline_host(z, rgb, T.outline_params(**kw))
                    assert np.array_equal(got, want), "%r: %d bytes differ" % (kw, int((got != want).sum()))
                    assert np.array_equal(T.outline_host(z, rgb, T.outline_params(**kw), in_place=True), want), "out == rgb"
    assert seen == SIL | STEP | CREASE, "a kind never occurs"
    assert np.array_equal(OC.bits(z), OC.bits(keep_z)) and np.array_equal(rgb, keep_rgb), "the arguments are left alone"
    # opacity 0 without ONLY is the frame itself, opacity 256 puts the ink's own bytes
    p = dict(radius=2, depth_step=1.0, ink=OC.INK)
    assert np.array_equal(T.outline_host(z, rgb, T.outline_params(opacity=0, **p)), rgb)
    inked = OC.inked_np(OC.kinds_np(z, 1.0), 2)[::-1]
    full = T.outline_host(z, rgb, T.outline_params(**p))
    assert inked.any() and not inked.all() and (full[inked] == np.array(OC.INK, np.uint8)).all() and np.array_equal(full[~inked], rgb[~inked])


def empty(W, Hh):
    return np.full((Hh, W), F32_MIN, np.float32)


def test_known_answer_square_on_an_empty_frame(built):
    import tiny_renderer_amd as T
    W, Hh = 16, 12
    z = empty(W, Hh)
    z[3:8, 4:9] = 7.0
    k = T.outline_kinds(z, T.outline_params(depth_step=1.0, crease=0.0))
    ring = np.zeros((Hh, W), bool)
    ring[3:8, 4:9] = True
    ring[4:7, 5:8] = False
    assert np.array_equal(k, np.where(ring, SIL, 0))
    rgb = np.full((Hh, W, 3), 200, np.uint8)
    out = T.outline_host(z, rgb, T.outline_params(radius=1, depth_step=1.0))
    inked = np.zeros((Hh, W), bool)
    inked[2:9, 3:10] = True
    inked[5, 6] = False                                   # the square's centre: two pixels from the ring
    assert np.array_equal((out == 0).all(-1)[::-1], inked) and np.array_equal(out[~inked[::-1]], rgb[~inked[::-1]])


def test_known_answer_a_vertical_step_inks_the_nearer_side(built):
    import tiny_renderer_amd as T
    z = np.full((8, 12), 10.0, np.float32)
    z[:, 6:] = 30.0                                       # larger z is nearer: columns 6.. stand in front
    k = T.outline_kinds(z, T.outline_params(depth_step=5.0, crease=100.0))
    want = np.zeros((8, 12), np.uint8)
    want[:, 6] = STEP
    assert np.array_equal(k, want)
    assert not T.outline_kinds(z, T.outline_params(depth_step=20.0)).any(), "fl(z0 - zq) > depth_step is strict"
    assert np.array_equal(T.outline_kinds(z, T.outline_params(depth_step=np.nextafter(np.float32(20.0), np.float32(0.0)))), want)


def test_known_answer_planes_have_no_crease_and_a_roof_has_one(built):
    import tiny_renderer_amd as T
    ys, xs = np.mgrid[0:10, 0:17].astype(np.float32)
    plane = (0.25 * xs + 0.5 * ys).astype(np.float32)     # exact in f32: the second difference is exactly 0
    assert not T.outline_kinds(plane, T.outline_params(depth_step=1.0, crease=0.0)).any()
    roof = (-0.5 * np.abs(xs - 8.0)).astype(np.float32)
    k = T.outline_kinds(roof, T.outline_params(depth_step=1.0, crease=0.0))
    want = np.zeros((10, 17), np.uint8)
    want[:, 8] = CREASE
    assert np.array_equal(k, want)
    assert not T.outline_kinds(roof, T.outline_params(depth_step=1.0)).any(), "no CREASE without TR_OUTLINE_CREASES"
    assert not T.outline_kinds(roof, T.outline_params(depth_step=1.0, crease=1.0)).any(), "|second difference| = 1 is not > 1"
    # a depth step is left to STEP: with depth_step below the roof's slope no axis across the ridge is flat
    k = T.outline_kinds(roof, T.outline_params(depth_step=0.25, crease=0.0))
    assert not (k & CREASE).any() and (k & STEP).any()


def test_known_answer_the_frames_border_is_not_a_silhouette(built):
    import tiny_renderer_amd as T
    z = np.full((6, 9), 3.0, np.float32)                  # every pixel drawn: every existing neighbour is drawn
    assert not T.outline_kinds(z, T.outline_params(depth_step=1.0, crease=0.0)).any()
    z = empty(9, 6)
    z[0, 0] = 3.0                                         # a corner pixel alone: its two existing neighbours are not drawn
    assert T.outline_kinds(z, T.outline_params(depth_step=1.0))[0, 0] == SIL
    z[0, 1] = z[1, 0] = 3.0
    assert T.outline_kinds(z, T.outline_params(depth_step=1.0))[0, 0] == 0


def test_known_answer_nan_seeds_no_step_and_is_no_step(built):
    import tiny_renderer_amd as T
    z = np.full((7, 7), 5.0, np.float32)
    z[3, 3] = np.nan
    assert not T.outline_kinds(z, T.outline_params(depth_step=0.0, crease=0.0)).any()
    z[3, 3] = -np.inf                                     # ... while an infinitely far pixel is a step for its four neighbours
    k = T.outline_kinds(z, T.outline_params(depth_step=0.0))
    want = np.zeros((7, 7), np.uint8)
    want[2, 3] = want[4, 3] = want[3, 2] = want[3, 4] = STEP
    assert np.array_equal(k, want)


def test_refusals_with_their_texts(built):
    import tiny_renderer_amd as T
    from tiny_renderer_amd import _lib
    L = T.load_library()
    z, rgb, kinds = np.zeros((2, 2), np.float32), np.zeros((2, 2, 3), np.uint8), np.zeros((2, 2), np.uint8)
    nan, inf = float("nan"), float("inf")
    bad = [("struct_size", 28, "struct_size is not sizeof(tr_outline_params)"), ("radius", 4, "radius must be 0..TR_OUTLINE_MAX_RADIUS"),
           ("flags", 4, "unknown flags"), ("flags", 0x80000001, "unknown flags"), ("opacity", 257, "opacity must be 0..256"),
           ("depth_step", -1.0, "depth_step must be finite and >= 0"), ("depth_step", nan, "depth_step must be finite and >= 0"),
           ("depth_step", inf, "depth_step must be finite and >= 0"), ("crease", -0.5, "crease must be finite and >= 0"),
           ("crease", nan, "crease must be finite and >= 0"), ("crease", inf, "crease must be finite and >= 0")]
    calls = (("tr_outline_host", lambda q: L.tr_outline_host(2, 2, z.ctypes.data, rgb.ctypes.data, rgb.ctypes.data, q)),
             ("tr_outline_kinds", lambda q: L.tr_outline_kinds(2, 2, z.ctypes.data, q, kinds.ctypes.data)),
             ("tr_scene_outline", None), ("tr_scene_get_outlined", None))
    for who, call in calls:
        if call is None:
            continue
        for field, v, text in bad:
            q = T.outline_params()
            setattr(q, field, v)
            assert call(C.addressof(q)) == _lib.TR_E_INVALID, (who, field, v)
            assert L.tr_last_error().decode() == who + ": " + text
        for field in ("ink", "paper"):
            q = T.outline_params()
            getattr(q, field)[3] = 1
            assert call(C.addressof(q)) == _lib.TR_E_INVALID
            assert L.tr_last_error().decode() == who + ": the fourth byte of ink and of paper must be 0"
        assert call(None) == _lib.TR_E_INVALID and L.tr_last_error().decode() == who + ": null argument"
    p = T.outline_params()
    q = C.addressof(p)
    assert L.tr_outline_host(2, 2, None, rgb.ctypes.data, rgb.ctypes.data, q) == _lib.TR_E_INVALID
    assert L.tr_last_error() == b"tr_outline_host: null argument"
    assert L.tr_outline_host(2, 2, z.ctypes.data, None, rgb.ctypes.data, q) == _lib.TR_E_INVALID
    assert L.tr_outline_host(2, 2, z.ctypes.data, rgb.ctypes.data, None, q) == _lib.TR_E_INVALID
    assert L.tr_outline_kinds(2, 2, None, q, kinds.ctypes.data) == _lib.TR_E_INVALID
    assert L.tr_last_error() == b"tr_outline_kinds: null argument"
    assert L.tr_outline_kinds(2, 2, z.ctypes.data, q, None) == _lib.TR_E_INVALID
    for w, h in ((0, 5), (5, 0), (0, 0)):
        assert L.tr_outline_host(w, h, None, None, None, q) == 0 and L.tr_outline_kinds(w, h, None, q, None) == 0
    assert L.tr_scene_outline(None, q, None) == _lib.TR_E_INVALID and L.tr_last_error() == b"tr_scene_outline: null scene"
    assert L.tr_scene_get_outlined(None, q, rgb.ctypes.data) == _lib.TR_E_INVALID and L.tr_last_error() == b"tr_scene_get_outlined: null scene"


def test_python_rejects_what_the_host_can_decide():
    import tiny_renderer_amd as T
    for kw in (dict(radius=-1), dict(radius=4), dict(radius=1.5), dict(radius=True), dict(opacity=257), dict(opacity=-1),
               dict(depth_step=-1.0), dict(depth_step=float("nan")), dict(depth_step=1e39), dict(crease=-1.0), dict(crease=float("inf")),
               dict(ink=(0, 0)), dict(ink=(0, 0, 256)), dict(paper=(-1, 0, 0))):
        with pytest.raises(ValueError):
            T.outline_params(**kw)
    s = T.Scene.__new__(T.Scene)
    s.width, s.height, s._h, s._pinned = 64, 64, None, []
    z, rgb = np.zeros((4, 4), np.float32), np.zeros((4, 4, 3), np.uint8)
    for call in (lambda: s.outline(None), lambda: s.get_outlined({}), lambda: T.outline_host(z, rgb, None), lambda: T.outline_kinds(z, 3),
                 lambda: T.outline_host(z, rgb[:-1], T.outline_params())):
        with pytest.raises(ValueError):
            call()
    p = T.outline_params(radius=2, depth_step=3.0, crease=0.5, ink=(1, 2, 3), opacity=7, only=True, paper=(4, 5, 6))
    assert (p.struct_size, p.radius, p.flags, p.opacity, bytes(p.ink), bytes(p.paper), p.depth_step, p.crease) == (
        32, 2, 3, 7, b"\x01\x02\x03\x00", b"\x04\x05\x06\x00", 3.0, 0.5)
    assert T.outline_params().flags == 0


@pytest.mark.parametrize("W,Hh", OC.SIZES)
def test_the_gpu_cases_are_not_vacuous(built, small_synthetic, W, Hh):
    """The oracle's frame of the GPU cases: at the thresholds the GPU tests use every kind occurs on at least 32 pixels
    and the ink covers between 1 % and 50 % of the frame at every radius; seeds lie in more than one tile and ink crosses
    a tile border."""
    import tiny_renderer_amd as T
    from oracle import oracle as O
    mesh = T.apply_instances(small_synthetic[0], OC.table(W, Hh))
    s = O.Scene(W, Hh, mesh, small_synthetic[1], "phong")
    s.clear()
    s.set_light_direction(H.light(OC.LIGHT)), s.set_camera(*H.camera(OC.CAM)), s.render()
    z, fb = s.z_f32(), s.get_frame_buffer()
    s.close()
    k = T.outline_kinds(z, T.outline_params(depth_step=OC.DEPTH_STEP, crease=OC.CREASE_T))
    assert np.array_equal(k, OC.kinds_np(z, OC.DEPTH_STEP, OC.CREASE_T))
    for bit, name in ((SIL, "SIL"), (STEP, "STEP"), (CREASE, "CREASE")):
        assert int(((k & bit) != 0).sum()) >= 32, name
    for kw in OC.gpu_params():
        inked = OC.inked_np(OC.kinds_np(z, kw["depth_step"], kw.get("crease")), kw["radius"])
        assert 0.01 <= inked.mean() <= 0.50, (kw, inked.mean())
        assert np.array_equal(T.outline_host(z, fb, T.outline_params(**kw)), OC.rule_np(z, fb, **kw))
    seed = k != 0
    tiles = [(j, i) for j in range(0, Hh, 16) for i in range(0, W, 128) if seed[j:j + 16, i:i + 128].any()]
    assert len(tiles) >= 2, "the seeds lie in one tile"
    inked3 = OC.inked_np(k, 3)
    crosses = False
    for j, i in tiles:
        own = np.zeros_like(seed)
        own[j:j + 16, i:i + 128] = seed[j:j + 16, i:i + 128]
        spread = OC.inked_np(np.where(own, 1, 0).astype(np.uint8), 3)
        spread[j:j + 16, i:i + 128] = False
        crosses |= bool(spread.any())
    assert crosses and inked3.any(), "no ink crosses a tile border"
