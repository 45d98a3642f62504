"""Depth of field: tr_scene_depth_of_field (k_dof), tr_dof_host and tr_dof_coc against the rule in numpy.

The rule, from the words of include/tiny_renderer.h: the circle of confusion of a pixel is background_radius where its z
bits are those of f32::MIN and min(max_radius, (((|z - focus|) - range) * scale) as u32) elsewhere, in f32 with every
operation rounded once; wt[r] = 32768 // (2r + 1)^2; the output at p sums, over every q inside the frame within
max_radius of p in both axes and with max(|dx|, |dy|) <= coc(q), sw += wt[coc(q)] and sc += wt[coc(q)] * F_q[c], and is
(sc + sw // 2) // sw; TR_DOF_SHOW_COC writes coc * 255 // max_radius.  The contract is exact: every comparison is
np.array_equal.

On the CPU the host entry points are pinned against that numpy restatement.  On the GPU the expectation is tr_dof_host
applied to a snapshot of the very frame (colour and z) that is then rendered again and blurred: reading a scene makes
its depth real and lowers flags, so the frame that is blurred is a fresh one."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import helpers as H
from tests import test_composite as TC

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32_MIN_BITS = np.uint32(0xFF7FFFFF)
F32_MIN = F32_MIN_BITS.view(np.float32)
bits, drive, scene, snap, clean_flags, tiles_any = TC.bits, TC.drive, TC.scene, TC.snap, TC.clean_flags, TC.tiles_any
WT = [32768 // (2 * r + 1) ** 2 for r in range(9)]


def P(focus, scale, R=4, bg=0, flags=0, rng=0.0):
    from tiny_renderer_amd.scene import dof_params
    return dof_params(focus, scale, max_radius=R, background_radius=bg, flags=flags, range=rng)


# ------------------------------------------------------------------------------------------------------------------
# The rule in numpy
# ------------------------------------------------------------------------------------------------------------------

def coc_np(z, focus, scale, R, bg=0, rng=0.0):
    """The circles of z (any shape), int64."""
    z = np.ascontiguousarray(z, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        d = (z - np.float32(focus)).astype(np.float32)
        a = np.abs(d).astype(np.float32)
        b = (a - np.float32(rng)).astype(np.float32)
        c = (b * np.float32(scale)).astype(np.float32)
        # `as u32`: NaN and negatives 0, truncating, saturating
        u = np.where(np.isnan(c), 0.0, np.clip(np.trunc(np.nan_to_num(c.astype(np.float64), nan=0.0)), 0.0, 4294967295.0)).astype(np.int64)
    out = np.minimum(u, R)
    return np.where(bits(z) == F32_MIN_BITS, bg, out).astype(np.int64)


def rule(z, rgb, focus, scale, R=4, bg=0, flags=0, rng=0.0):
    """z [H, W] y up, rgb [H, W, 3] row 0 = top.  Returns the blurred frame."""
    z = np.ascontiguousarray(z, np.float32)
    Hh, W = z.shape
    coc = coc_np(z, focus, scale, R, bg, rng)
    if flags & 1:
        v = (coc * 255 // R).astype(np.uint8)[::-1]
        return np.ascontiguousarray(np.repeat(v[..., None], 3, -1))
    F = rgb[::-1].astype(np.int64)                        # z's orientation
    w = np.array(WT, np.int64)[coc]
    pc = np.full((Hh + 2 * R, W + 2 * R), -1, np.int64)   # outside the frame: a circle no distance satisfies
    pc[R:R + Hh, R:R + W] = coc
    pw = np.zeros((Hh + 2 * R, W + 2 * R), np.int64)
    pw[R:R + Hh, R:R + W] = w
    pf = np.zeros((Hh + 2 * R, W + 2 * R, 3), np.int64)
    pf[R:R + Hh, R:R + W] = F
    sw = np.zeros((Hh, W), np.int64)
    sc = np.zeros((Hh, W, 3), np.int64)
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            sl = (slice(R + dy, R + dy + Hh), slice(R + dx, R + dx + W))
            ok = pc[sl] >= max(abs(dx), abs(dy))
            ww = np.where(ok, pw[sl], 0)
            sw += ww
            sc += ww[..., None] * pf[sl]
    assert sw.min() >= 113 and (sc + sw[..., None] // 2).max() < 2 ** 32
    out = ((sc + sw[..., None] // 2) // sw[..., None]).astype(np.uint8)
    return np.ascontiguousarray(out[::-1])


# ------------------------------------------------------------------------------------------------------------------
# CPU
# ------------------------------------------------------------------------------------------------------------------

BAD = [("struct_size", 24), ("struct_size", 32), ("max_radius", 0), ("max_radius", 9), ("background_radius", 5), ("flags", 2),
       ("flags", 0x80000001), ("focus", float("nan")), ("focus", float("inf")), ("focus", float("-inf")),
       ("range", -1.0), ("range", float("nan")), ("range", float("inf")),
       ("scale", 0.0), ("scale", -2.0), ("scale", float("nan")), ("scale", float("inf"))]


def test_entry_points_declared_exported_and_typed(built):
    import tiny_renderer_amd as T
    from tiny_renderer_amd import _lib
    from tiny_renderer_amd.scene import DofParams, dof_params
    header = open(os.path.join(REPO, "include", "tiny_renderer.h")).read()
    assert re.search(r"int\s+tr_scene_depth_of_field\(tr_scene \*s, const tr_dof_params \*p, void \*out", header)
    assert re.search(r"int\s+tr_scene_get_depth_of_field\(tr_scene \*s, const tr_dof_params \*p, uint8_t \*rgb\);", header)
    assert re.search(r"int\s+tr_dof_host\(uint32_t width, uint32_t height, const float \*z", header)
    assert re.search(r"int\s+tr_dof_coc\(const tr_dof_params \*p, uint32_t n, const float \*z, uint8_t \*coc\);", header)
    for word in ("#define TR_DOF_MAX_RADIUS 8", "#define TR_DOF_SHOW_COC 0x1u", "} tr_dof_params;", "#define TR_ABI_VERSION 3"):
        assert word in header, word
    exports = open(os.path.join(REPO, "tiny_renderer_amd", "csrc", "exports.map")).read()
    assert re.search(r"global:\s*tr_\*;", exports)
    raw = C.CDLL(_lib.library_path())
    for name in ("tr_scene_depth_of_field", "tr_scene_get_depth_of_field", "tr_dof_host", "tr_dof_coc"):
        assert hasattr(raw, name), name + " is not exported"
        assert name in _lib.SYMBOLS
    assert _lib.SYMBOLS["tr_scene_depth_of_field"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p])
    assert _lib.SYMBOLS["tr_scene_get_depth_of_field"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p])
    assert _lib.SYMBOLS["tr_dof_host"] == (C.c_int, [C.c_uint32, C.c_uint32] + [C.c_void_p] * 4)
    assert _lib.SYMBOLS["tr_dof_coc"] == (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p])
    assert C.sizeof(DofParams) == 28
    L = T.load_library()
    assert L.tr_abi_version() == 3
    p = dof_params(focus=1.0, scale=2.0)
    assert (p.struct_size, p.max_radius, p.background_radius, p.flags, p.focus, p.range, p.scale) == (28, 4, 0, 0, 1.0, 0.0, 2.0)
    with pytest.raises(TypeError):
        dof_params()                                      # focus and scale are required
    assert L.tr_scene_depth_of_field(None, C.addressof(p), None) == _lib.TR_E_INVALID and b"null" in L.tr_last_error()
    assert L.tr_scene_get_depth_of_field(None, C.addressof(p), None) == _lib.TR_E_INVALID
    for name in ("depth_of_field_host", "dof_coc", "dof_params", "DofParams"):
        assert hasattr(T, name) and name in T.__all__, name
    assert callable(T.Scene.depth_of_field) and callable(T.Scene.get_depth_of_field)


def test_host_refuses_every_invalid_parameter(built):
    import tiny_renderer_amd as T
    from tiny_renderer_amd import _lib
    L = T.load_library()
    z, rgb, out = np.zeros((2, 2), np.float32), np.zeros((2, 2, 3), np.uint8), np.zeros((2, 2, 3), np.uint8)
    coc = np.zeros(4, np.uint8)
    host = lambda q: L.tr_dof_host(2, 2, z.ctypes.data, rgb.ctypes.data, out.ctypes.data, C.addressof(q) if q is not None else None)
    assert host(P(1.0, 2.0)) == 0
    assert host(None) == _lib.TR_E_INVALID and b"null" in L.tr_last_error()
    for field, v in BAD:
        q = P(1.0, 2.0)
        setattr(q, field, v)
        assert host(q) == _lib.TR_E_INVALID and L.tr_last_error(), (field, v)
        assert L.tr_dof_coc(C.addressof(q), 4, z.ctypes.data, coc.ctypes.data) == _lib.TR_E_INVALID, (field, v)
    q = P(1.0, 2.0)
    assert L.tr_dof_host(2, 2, None, rgb.ctypes.data, out.ctypes.data, C.addressof(q)) == _lib.TR_E_INVALID
    assert L.tr_dof_host(2, 2, z.ctypes.data, rgb.ctypes.data, rgb.ctypes.data, C.addressof(q)) == _lib.TR_E_INVALID   # out == rgb
    assert L.tr_dof_host(0, 5, None, None, None, C.addressof(q)) == 0 and L.tr_dof_host(5, 0, None, None, None, C.addressof(q)) == 0
    assert L.tr_dof_coc(C.addressof(q), 0, None, None) == 0
    # python: ValueError before anything reaches the library
    from tiny_renderer_amd.scene import dof_params
    for kw in (dict(max_radius=0), dict(max_radius=9), dict(max_radius=2.5), dict(max_radius=True), dict(background_radius=5),
               dict(background_radius=-1), dict(flags=2), dict(focus=float("nan")), dict(focus=float("inf")), dict(range=-1.0),
               dict(range=float("nan")), dict(scale=0.0), dict(scale=-1.0), dict(scale=float("inf")), dict(scale=1e39)):
        with pytest.raises(ValueError):
            dof_params(**dict(dict(focus=1.0, scale=2.0), **kw))
    s = T.Scene.__new__(T.Scene)
    s.width, s.height, s._h, s._pinned = 64, 64, None, []
    with pytest.raises(ValueError):
        s.depth_of_field(None)
    with pytest.raises(ValueError):
        s.get_depth_of_field((1.0, 2.0))
    with pytest.raises(ValueError):
        T.depth_of_field_host(z, rgb[:-1], q)


def test_weight_table(built):
    """wt through the library: a single pixel of circle r on black with colour 255 and the rounding of its own tap."""
    import tiny_renderer_amd as T
    assert WT == [32768, 3640, 1310, 668, 404, 270, 193, 145, 113]
    # two pixels side by side: the left one of circle r and white, the right one of circle 0 and black; at the right
    # one sw = wt[r] + wt[0], sc = 255 * wt[r]: the output pins wt[r]
    for r in range(1, 9):
        z = np.array([[float(r), 0.0]], np.float32)       # focus 0, scale 1: coc = z
        rgb = np.array([[[255, 255, 255], [0, 0, 0]]], np.uint8)
        got = T.depth_of_field_host(z, rgb, P(0.0, 1.0, R=8))
        want = (255 * WT[r] + (WT[r] + WT[0]) // 2) // (WT[r] + WT[0])
        assert got[0, 1].tolist() == [want] * 3 and got[0, 0].tolist() == [255] * 3, r


def edge_values(focus, rng, scale):
    """z values whose circle sits on an edge of the rule."""
    f, b, s = np.float32(focus), np.float32(rng), np.float32(scale)
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    out = [F32_MIN, nan, -nan, inf, -inf, np.float32(0.0), np.float32(-0.0), np.finfo(np.float32).max, np.nextafter(F32_MIN, np.float32(0)),
           f, f + b, f - b, np.nextafter(f + b, inf), np.nextafter(f - b, -inf), np.float32(1e-45), np.float32(-1e-45)]
    # products that land just below and just at an integer
    for k in range(1, 11):
        t = np.float32(f + b + np.float32(k) / s)
        out += [t, np.nextafter(t, inf), np.nextafter(t, -inf)]
        t = np.float32(f - b - np.float32(k) / s)
        out += [t, np.nextafter(t, inf), np.nextafter(t, -inf)]
    return np.array(out, np.float32)


def test_coc_equals_the_numpy_restatement(built):
    import tiny_renderer_amd as T
    rng_ = np.random.default_rng(11)
    seen = set()
    for focus, rng, scale in ((100.0, 0.0, 1.0), (100.0, 2.5, 0.75), (-3.0, 0.125, 3.0), (0.0, 0.0, 1e-3), (7.0, 1.0, 1e30), (1e30, 0.0, 1.0)):
        z = np.concatenate([edge_values(focus, rng, scale), (focus + rng_.normal(0.0, 6.0 / min(scale, 10.0), 4000)).astype(np.float32),
                            rng_.normal(0.0, 1e4, 500).astype(np.float32)])
        for R in range(1, 9):
            for bg in (0, R):
                got = T.dof_coc(P(focus, scale, R=R, bg=bg, rng=rng), z)
                want = coc_np(z, focus, scale, R, bg, rng)
                assert got.dtype == np.uint8 and np.array_equal(got.astype(np.int64), want), (focus, rng, scale, R, bg)
                assert got[0] == bg and got[1] == 0 and got[2] == 0 and got[3] == R and got[4] == R   # f32::MIN, NaN, NaN, inf, -inf
                seen |= set(got.tolist())
    assert seen == set(range(9))
    # z exactly at focus +- range is sharp, and the first z whose product reaches 1 has circle 1
    assert T.dof_coc(P(10.0, 1.0, rng=2.0), np.array([12.0, 8.0, 13.0, 7.0, 12.999999, 7.000001], np.float32)).tolist() == [0, 0, 1, 1, 0, 0]
    z2 = rng_.normal(0.0, 3.0, (5, 7)).astype(np.float32)
    assert T.dof_coc(P(0.0, 1.0), z2).shape == (5, 7)


def planted_field(W, Hh, seed):
    """z around 100 in depth layers with undrawn regions and the edge values planted: a near object (z 110), a far one
    (z 90) and a ramp between them."""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:Hh, 0:W]
    z = (90.0 + 20.0 * xs / max(W - 1, 1) + rng.normal(0.0, 0.4, (Hh, W))).astype(np.float32)
    z[rng.random((Hh, W)) < 0.1] = F32_MIN
    if Hh > 8 and W > 20:
        z[Hh // 2:Hh // 2 + 4, W // 3:W // 3 + 9] = F32_MIN      # an undrawn patch
        z[2:Hh // 2, W // 2:W // 2 + 6] = 100.0                    # an object in focus in front of / behind the ramp
        z[Hh // 2 + 1:Hh - 2, 4:10] = 118.0                        # a blurred object over a sharp region
        ev = edge_values(100.0, 1.0, 0.5)
        n = min(len(ev), W - 2)
        z[0, 1:1 + n] = ev[:n]
        z[Hh - 1, 1:1 + n] = ev[::-1][:n]
    return z


@pytest.mark.parametrize("W,Hh", [(37, 29), (1, 1), (200, 40)])
def test_host_rule_equals_the_numpy_rule_on_planted_fields(built, W, Hh):
    import tiny_renderer_amd as T
    rng = np.random.default_rng(W)
    z = planted_field(W, Hh, W + Hh)
    rgb = rng.integers(0, 256, (Hh, W, 3), dtype=np.uint8)
    keep_z, keep_rgb = z.copy(), rgb.copy()
    changed = 0
    for R in range(1, 9):
        for bg in (0, R):
            kw = dict(focus=100.0, scale=0.5, R=R, bg=bg, rng=1.0)
            want = rule(z, rgb, **kw)
            got = T.depth_of_field_host(z, rgb, P(**kw))
            assert np.array_equal(got, want), "R %d bg %d: %d bytes differ" % (R, bg, int((got != want).sum()))
            changed += int((got != rgb).sum())
            show = T.depth_of_field_host(z, rgb, P(flags=1, **kw))
            assert np.array_equal(show, rule(z, rgb, flags=1, **kw))
    assert W == 1 or changed > 1000
    for focus, scale, rng_ in ((90.0, 3.0, 0.0), (110.0, 0.25, 4.0), (100.0, 1e30, 0.0), (100.0, 1e-30, 0.0)):
        kw = dict(focus=focus, scale=scale, R=5, bg=2, rng=rng_)
        assert np.array_equal(T.depth_of_field_host(z, rgb, P(**kw)), rule(z, rgb, **kw)), kw
    assert np.array_equal(bits(z), bits(keep_z)) and np.array_equal(rgb, keep_rgb), "the arguments are left alone"


def test_a_sharp_object_in_front_of_a_blurred_one_and_the_reverse(built):
    """Scatter as gather: a blurred pixel spreads over a sharp neighbour, a sharp pixel does not spread over a blurred
    one -- whichever of the two is nearer."""
    import tiny_renderer_amd as T
    W, Hh = 40, 12
    for near_sharp in (True, False):
        z = np.full((Hh, W), 100.0 if near_sharp else 104.0, np.float32)    # left half
        z[:, W // 2:] = 104.0 if near_sharp else 100.0
        rgb = np.zeros((Hh, W, 3), np.uint8)
        rgb[:, :W // 2] = (200, 40, 10)
        rgb[:, W // 2:] = (10, 90, 250)
        p = dict(focus=100.0, scale=1.0, R=4)
        got = T.depth_of_field_host(z, rgb, P(**p))
        assert np.array_equal(got, rule(z, rgb, **p))
        sharp = slice(0, W // 2) if near_sharp else slice(W // 2, W)
        soft = slice(W // 2, W) if near_sharp else slice(0, W // 2)
        edge_sharp = got[:, sharp][:, -1 if near_sharp else 0]
        edge_soft = got[:, soft][:, 0 if near_sharp else -1]
        assert (edge_sharp != rgb[:, sharp][:, 0]).any(), "the blurred side does not spread over the sharp side"
        # on the blurred side next to the border the sharp pixels (circle 0) never qualify at a distance >= 1: what is
        # there is the mean of blurred pixels only, all of one colour
        assert np.array_equal(edge_soft, rgb[:, soft][:, 0]), "a sharp pixel spread"


def test_contract_cases(built):
    import tiny_renderer_amd as T
    rng = np.random.default_rng(5)
    W, Hh = 37, 29
    z = planted_field(W, Hh, 3)
    rgb = rng.integers(0, 256, (Hh, W, 3), dtype=np.uint8)
    # every circle 0 (a range that swallows everything, background 0): the frame byte for byte
    sharp = P(100.0, 1.0, R=8, rng=1e30)
    with np.errstate(invalid="ignore"):
        zf = np.where((np.abs(z) < 1e6) | (bits(z) == F32_MIN_BITS), z, np.float32(100.0)).astype(np.float32)
    assert (bits(zf) == F32_MIN_BITS).any()
    assert not T.dof_coc(sharp, zf).any()
    assert np.array_equal(T.depth_of_field_host(zf, rgb, sharp), rgb)
    # a constant colour stays constant under any circles: (sw * c + sw / 2) / sw == c
    for c in (0, 1, 127, 128, 254, 255):
        flat = np.full((Hh, W, 3), c, np.uint8)
        flat[..., 1] = 255 - c
        for R in (1, 5, 8):
            got = T.depth_of_field_host(z, flat, P(100.0, 0.5, R=R, bg=R // 2))
            assert np.array_equal(got, flat), (c, R)
    # a single bright pixel of circle r on black (everything else circle 0) spreads over exactly the (2r + 1)^2 square,
    # clipped at the frame
    for r in range(1, 9):
        for (py, px) in ((14, 18), (0, 0), (Hh - 1, W - 2), (3, W - 1)):
            z1 = np.zeros((Hh, W), np.float32)
            z1[py, px] = float(r)
            one = np.zeros((Hh, W, 3), np.uint8)
            one[Hh - 1 - py, px] = 255
            got = T.depth_of_field_host(z1, one, P(0.0, 1.0, R=8))
            lit = got.any(-1)[::-1]
            ys, xs = np.mgrid[0:Hh, 0:W]
            assert np.array_equal(lit, (np.abs(ys - py) <= r) & (np.abs(xs - px) <= r)), (r, py, px)
            assert np.array_equal(got, rule(z1, one, 0.0, 1.0, R=8))
    # TR_DOF_SHOW_COC
    for R in (1, 3, 8):
        p = P(100.0, 0.5, R=R, bg=1, flags=1)
        got = T.depth_of_field_host(z, rgb, p)
        want = (T.dof_coc(p, z).astype(np.int64) * 255 // R).astype(np.uint8)[::-1]
        assert np.array_equal(got, np.repeat(want[..., None], 3, -1))


# ------------------------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------------------------

AT = TC.DST_AT


@pytest.fixture(scope="module")
def other_synthetic(built):
    import tiny_renderer_amd as T
    return T.synthetic_scene(n_lat=9, n_lon=17, tex_size=128, radius=0.75)


def host(f, p):
    import tiny_renderer_amd as T
    return T.depth_of_field_host(f["z"], f["fb"], p)


def params_for(f, R, bg=0, flags=0, near=False):
    """focus and scale from the snapshot's z quantiles, so that the frame holds sharp pixels, partly blurred pixels and
    pixels at max_radius -- asserted.  The focus lies on the model's far parts (its silhouette), or with near=True on
    its near parts, so that the silhouette is blurred."""
    import tiny_renderer_amd as T
    z = f["z"][bits(f["z"]) != F32_MIN_BITS]
    assert z.size > 50
    lo, hi = (np.quantile(z, 0.05), np.quantile(z, 0.85)) if near else (np.quantile(z, 0.15), np.quantile(z, 0.95))
    assert hi > lo
    p = P(float(hi if near else lo), float((R + 1.5) / (hi - lo)), R=R, bg=bg, flags=flags, rng=float((hi - lo) * 0.02))
    coc = T.dof_coc(p, f["z"])[bits(f["z"]) != F32_MIN_BITS]
    assert (coc == 0).any() and (coc == R).any(), "the case holds no sharp pixel or none at max_radius"
    assert R == 1 or ((coc > 0) & (coc < R)).any(), "the case holds no partly blurred pixel"
    return p


def state(s):
    """Everything a call must leave alone: z, winner words, shadow buffer."""
    out = {"z": bits(s.read_z_f32()), "win": s.read_winner_u32() if getattr(s, "_tap", False) else None}
    out["shadow"] = bits(s.read_shadow_f32()) if s.pipeline in ("shadow", "occlusion") else None
    return out


def same_state(a, b):
    for k in a:
        assert (a[k] is None and b[k] is None) or np.array_equal(a[k], b[k]), k + " changed"


def box(img, f):
    Hh, W, _ = img.shape
    return ((img.reshape(Hh // f, f, W // f, f, 3).astype(np.uint32).sum((1, 3)) + f * f // 2) // (f * f)).astype(np.uint8)


def device_buffer(n, fill=0x5A):
    import torch
    t = torch.full((n,), fill, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return t


# where the model stands at the shapes with partial tiles: over the corner of the partial tile column and row
PLACE = {(208, 40): np.array([[0.3, 0.5, 0.0, 0.7]], np.float32), (144, 24): np.array([[0.6, 0.4, 0.0, 0.6]], np.float32)}
RADII = ((1, 0), (3, 3), (8, 0), (8, 2))


def partial_tiles_are_blurred(f, p, want):
    """The drawn pixels with a circle > 0 whose output differs from the input, in the partial tile column and in the
    partial tile row of the frame (z's orientation): both must exist."""
    import tiny_renderer_amd as T
    Hh, W = f["z"].shape
    hit = (bits(f["z"]) != F32_MIN_BITS) & (T.dof_coc(p, f["z"]) > 0) & (want != f["fb"]).any(-1)[::-1]
    assert W % 128 and Hh % 16
    assert hit[:, W // 128 * 128:].any(), "no drawn, blurred pixel changes in the partial tile column"
    assert hit[Hh // 16 * 16:].any(), "no drawn, blurred pixel changes in the partial tile row"


@pytest.mark.gpu
@pytest.mark.parametrize("store_depth", [False, True], ids=["transient", "stored"])
@pytest.mark.parametrize("pipe", ["phong", "shadow"])
@pytest.mark.parametrize("W,Hh", [(256, 48), (384, 48), (128, 16), (200, 40), (208, 40), (144, 24)])
def test_blurred_frame_equals_the_host_rule(small_synthetic, W, Hh, pipe, store_depth):
    """2 x 3 tiles, none with eight neighbours; 3 x 3 with a middle tile; one tile whose halo is all outside the frame;
    the guarded path with a partial last tile column and row; the wide form with partial tiles in x and y (208 x 40), and
    with a 16-pixel tile column over a half tile row (144 x 24) -- there the model stands over the partial tiles.  In
    place, for radii 1, 3 and 8."""
    s = scene(W, Hh, small_synthetic, pipe, PLACE.get((W, Hh), AT), tap=True, store_depth=store_depth)
    drive(s)
    f, before = snap(s), state(s)
    for R, bg in RADII:
        p = params_for(f, R, bg)
        want = host(f, p)
        assert not np.array_equal(want, f["fb"]), "the expectation is the unblurred frame"
        if (W, Hh) in PLACE:
            partial_tiles_are_blurred(f, p, want)
        drive(s)                                          # a fresh frame: depth and flags as a render leaves them
        s.depth_of_field(p)
        assert s.sync() == 0
        got = s.get_frame_buffer()
        assert np.array_equal(got, want), "R %d bg %d: %d bytes differ" % (R, bg, int((got != want).sum()))
        same_state(state(s), before)
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("store_depth", [False, True], ids=["transient", "stored"])
def test_colour_spreads_into_a_fast_cleared_tile_and_clean_neighbourhoods_stay_zero(small_synthetic, store_depth):
    """640 x 64 is 5 x 4 tiles with a small model on the left: tiles next to it have both flags up and receive colour,
    tiles whose whole 3 x 3 neighbourhood is clean come out as zeros and keep their flag."""
    W, Hh = 640, 64
    s = scene(W, Hh, small_synthetic, "phong", TC._small(-0.62, 0.18), store_depth=store_depth)
    drive(s)
    f, flags = snap(s), clean_flags(s)
    assert not (flags & tiles_any(bits(f["z"]) != F32_MIN_BITS)).any()
    p = params_for(f, 8, near=True)                      # the silhouette is blurred: it spreads over the tile's border
    want = host(f, p)
    lit = tiles_any(want[::-1].any(-1))
    spill = lit & flags                                   # flag up on the snapshot, colour in the expectation
    assert spill.any(), "no tile next to the model has its flag up and receives colour"
    near = np.zeros_like(flags)                           # a non-clean tile somewhere in the 3 x 3 neighbourhood
    ty, tx = flags.shape
    for j in range(ty):
        for i in range(tx):
            near[j, i] = (~flags[max(j - 1, 0):j + 2, max(i - 1, 0):i + 2]).any()
    assert (~near).any() and not (lit & ~near).any()
    for place in ("in", "out"):
        drive(s)
        if place == "in":
            s.depth_of_field(p)
            got = s.get_frame_buffer()
            assert np.array_equal(clean_flags(s), ~near), "flags: up exactly where the whole neighbourhood was clean"
        else:
            got = s.get_depth_of_field(p)
        assert np.array_equal(got, want), "%s place: %d bytes differ" % (place, int((got != want).sum()))
        for j, i in zip(*np.nonzero(spill)):
            tile = got[::-1][j * 16:j * 16 + 16, i * 128:i * 128 + 128]
            assert tile.any(), "nothing spread into tile (%d, %d)" % (j, i)
        for j, i in zip(*np.nonzero(~near)):
            assert not got[::-1][j * 16:j * 16 + 16, i * 128:i * 128 + 128].any()
    s.close()


@pytest.mark.gpu
def test_out_of_place_targets_leave_the_scene_alone(small_synthetic):
    import tiny_renderer_amd as T
    W, Hh = 256, 48
    s = scene(W, Hh, small_synthetic, "phong", AT, tap=True)
    drive(s)
    f, before, flags = snap(s), state(s), clean_flags(s)
    p = params_for(f, 3)
    want = host(f, p)
    assert not np.array_equal(want, f["fb"])
    # device memory
    drive(s)
    dev = device_buffer(W * Hh * 3)
    s.depth_of_field(p, out=dev.data_ptr())
    assert s.sync() == 0
    assert np.array_equal(dev.cpu().numpy().reshape(Hh, W, 3), want)
    # memory from tr_host_alloc
    pinned = s.pinned_frame()
    pinned[:] = 0xA5
    s.depth_of_field(p, out=pinned)
    assert s.sync() == 0 and np.array_equal(pinned, want)
    # the getter: any host memory
    assert np.array_equal(s.get_depth_of_field(p), want)
    # ordinary host memory is refused by the asynchronous call
    plain = np.zeros((Hh, W, 3), np.uint8)
    with pytest.raises(T.TinyRendererError):
        s.depth_of_field(p, out=plain)
    assert not plain.any()
    assert np.array_equal(clean_flags(s), flags)
    TC.same(snap(s), f)
    same_state(state(s), before)
    # show the circles, on the device
    show = params_for(f, 3, bg=1, flags=1)
    drive(s)
    assert np.array_equal(s.get_depth_of_field(show), host(f, show))
    drive(s)
    s.depth_of_field(show)
    assert np.array_equal(s.get_frame_buffer(), host(f, show))
    s.close()


@pytest.mark.gpu
def test_in_place_consumers_see_the_blurred_frame(small_synthetic, other_synthetic):
    import tiny_renderer_amd as T
    W, Hh = 512, 64
    mk = lambda ms=None, at=None: scene(W, Hh, ms or small_synthetic, "phong", TC._small(-0.4, 0.1) if at is None else at)
    ref = mk()
    drive(ref)
    f = snap(ref)
    ref.close()
    p = params_for(f, 3)
    once = host(f, p)
    twice = host(dict(f, fb=once), p)
    assert not np.array_equal(once, f["fb"]) and not np.array_equal(twice, once)
    blurred = dict(f, fb=once, win=None)
    s = mk()
    drive(s), s.depth_of_field(p)
    assert np.array_equal(s.resolve(2), box(once, 2))
    # the sparse read-back into a page-locked buffer: the copied flags
    out = s.pinned_frame()
    out[:] = 0x5A
    drive(s), s.depth_of_field(p)
    s.get_frame_buffer_async(out)
    assert s.sync() == 0 and np.array_equal(out, once)
    flags = clean_flags(s)
    assert not (flags & tiles_any(once[::-1].any(-1))).any(), "a tile with colour in it is flagged clean"
    assert np.array_equal(bits(s.read_z_f32()), bits(f["z"]))
    # twice
    s.depth_of_field(p)
    assert np.array_equal(s.get_frame_buffer(), twice), "blurring twice is the rule applied twice"
    s.close()
    # composite: the blurred scene as dst and as src; blur over a merged frame
    o = mk(other_synthetic, TC._small(-0.2, 0.0, 0.2))
    drive(o, light=0.2)
    fo = snap(o)
    fo["win"] = None
    o.close()
    for role in ("dst", "src", "after"):
        a, b = mk(), mk(other_synthetic, TC._small(-0.2, 0.0, 0.2))
        drive(a), drive(b, light=0.2)
        if role == "dst":
            a.depth_of_field(p)
            a.composite(b)
            want, wins = TC.merge(blurred, fo)
            got = a
        elif role == "src":
            a.depth_of_field(p)
            b.composite(a)
            want, wins = TC.merge(fo, blurred)
            got = b
        else:
            a.composite(b)
            a.depth_of_field(p)
            want, wins = TC.merge(dict(f, win=None), fo)
            merged_blur = host(want, p)
            assert not np.array_equal(merged_blur, want["fb"])
            want["fb"] = merged_blur
            got = a
        assert wins.any() and not wins.all()
        TC.same(snap(got), want)
        a.close(), b.close()
    # the rule on the composite agrees with tr_composite_host on the blurred colour
    z, c = T.composite_host(fo["z"], fo["fb"][::-1], f["z"], once[::-1])
    want, _ = TC.merge(fo, blurred)
    assert np.array_equal(c[::-1], want["fb"]) and np.array_equal(bits(z), bits(want["z"]))


@pytest.mark.gpu
def test_over_an_accumulated_frame(small_synthetic):
    W, Hh, n = 256, 48, 4
    par = TC._params(n)
    ref = scene(W, Hh, small_synthetic, "phong", AT, frames_per_launch=4)
    ref.render_frames(par)
    avg = ref.accumulate(3)
    ref.select_frame(0)
    z = ref.read_z_f32()
    ref.close()
    f = {"fb": avg, "z": z}
    p = params_for(f, 3)
    want = host(f, p)
    assert not np.array_equal(want, avg)
    s = scene(W, Hh, small_synthetic, "phong", AT, frames_per_launch=4)
    s.render_frames(par)
    s.accumulate_in_place(3)
    s.depth_of_field(p)
    assert np.array_equal(s.get_frame_buffer(), want)
    assert np.array_equal(bits(s.read_z_f32()), bits(z))
    s.close()


@pytest.mark.gpu
def test_a_cleared_scene_held_back_frames_and_errors(small_synthetic):
    import tiny_renderer_amd as T
    from tiny_renderer_amd import _lib
    L = T.load_library()
    W, Hh = 256, 48
    s = scene(W, Hh, small_synthetic, "phong", AT, tap=True, auto_group=True)
    band = scene(W, Hh, small_synthetic, "phong", AT, band_rows=(16, 32))
    drive(s)
    f = snap(s)
    p = params_for(f, 3, bg=2)
    # frames tr_scene_render holds back are submitted first
    drive(s, cam=1.0), drive(s, cam=2.0), drive(s)
    assert np.array_equal(s.get_depth_of_field(p), host(f, p))
    # errors: nothing changed, nothing queued
    drive(s), drive(band)
    before, flags = snap(s), clean_flags(s)
    for field, v in BAD:
        q = params_for(f, 3, bg=2)
        setattr(q, field, v)
        assert L.tr_scene_depth_of_field(s._h, C.addressof(q), None) == _lib.TR_E_INVALID and L.tr_last_error(), (field, v)
        host_out = np.zeros((Hh, W, 3), np.uint8)
        assert L.tr_scene_get_depth_of_field(s._h, C.addressof(q), host_out.ctypes.data) == _lib.TR_E_INVALID, (field, v)
    assert L.tr_scene_depth_of_field(s._h, None, None) == _lib.TR_E_INVALID
    assert L.tr_scene_depth_of_field(None, C.addressof(p), None) == _lib.TR_E_INVALID
    assert L.tr_scene_depth_of_field(band._h, C.addressof(p), None) == _lib.TR_E_INVALID and b"band" in L.tr_last_error()
    with pytest.raises(T.TinyRendererError):
        band.get_depth_of_field(p)
    # an `out` that overlaps the scene's frame buffer, at its start and inside it; a pinned buffer that is too small
    fb_dev = int(s.frame_buffer_device())
    for off in (0, 3 * W, W * Hh * 3 - 1):
        assert L.tr_scene_depth_of_field(s._h, C.addressof(p), fb_dev + off) == _lib.TR_E_INVALID and b"overlaps" in L.tr_last_error()
    small = L.tr_host_alloc(W * Hh * 3 - 1)
    assert small
    assert L.tr_scene_depth_of_field(s._h, C.addressof(p), small) == _lib.TR_E_INVALID and b"smaller" in L.tr_last_error()
    L.tr_host_free(small)
    plain = np.zeros((Hh, W, 3), np.uint8)
    assert L.tr_scene_depth_of_field(s._h, C.addressof(p), plain.ctypes.data) == _lib.TR_E_INVALID and b"tr_host_alloc" in L.tr_last_error()
    assert s.sync() == 0 and np.array_equal(clean_flags(s), flags)
    TC.same(snap(s), before)
    # logically cleared: zeros out of place, nothing in place
    s.clear()
    dev = device_buffer(W * Hh * 3)
    s.depth_of_field(p, out=dev.data_ptr())
    assert s.sync() == 0 and not dev.cpu().numpy().any()
    assert not s.get_depth_of_field(p).any()
    s.depth_of_field(p)
    assert not s.get_frame_buffer().any() and (bits(s.read_z_f32()) == F32_MIN_BITS).all()
    s.close(), band.close()


# ------------------------------------------------------------------------------------------------------------------
# Paths of k_dof and of the in-place call that the cases above do not reach; each case asserts that it reaches its own
# ------------------------------------------------------------------------------------------------------------------

def device_bytes(ptr, n):
    """A torch view of n bytes of device memory at ptr."""
    import torch

    class View:
        __cuda_array_interface__ = {"shape": (n,), "typestr": "|u1", "data": (int(ptr), False), "version": 2}

    return torch.as_tensor(View(), device="cuda")


@pytest.mark.gpu
@pytest.mark.parametrize("place", ["out", "in"])
def test_state_out_and_a_callers_frame_buffer_aligned_and_not(small_synthetic, place):
    """256 x 48 takes the wide form unless an address says otherwise: `out`, and a caller's frame buffer blurred in place
    (where the two stream-ordered copies write it), at 0, 4 and 16 bytes past a guard.  Every byte of the frame is the
    rule's and no byte of the guards on either side changes."""
    import torch
    W, Hh = 256, 48
    n = W * Hh * 3
    ref = scene(W, Hh, small_synthetic, "phong", AT)
    drive(ref)
    f = snap(ref)
    ref.close()
    p = params_for(f, 8, 2)
    want = host(f, p)
    assert not np.array_equal(want, f["fb"])
    guard = 48
    buf = torch.full((guard + n + guard,), 0xAA, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert buf.data_ptr() % 16 == 0
    for off in (0, 4, 16):      # (ascending: the bytes behind a frame have not held an earlier one)
        at = buf.data_ptr() + guard + off
        if place == "out":
            d = scene(W, Hh, small_synthetic, "phong", AT)
            drive(d)
            d.depth_of_field(p, out=at)
        elif off % 16 == 0:
            d = scene(W, Hh, small_synthetic, "phong", AT, frame_buffer_device=at)
            drive(d)
            d.depth_of_field(p)
        else:
            # the scene's own kernels store whole 16-byte pieces, so it renders into its own buffer; the frame is copied
            # to the odd address and handed over: the launcher must see the alignment and take the guarded form
            d = scene(W, Hh, small_synthetic, "phong", AT)
            drive(d)
            assert d.sync() == 0
            buf[guard + off:guard + off + n] = device_bytes(d.frame_buffer_device(), n)
            torch.cuda.synchronize()
            d.set_frame_buffer_device(at)
            d.depth_of_field(p)
        assert d.sync() == 0
        torch.cuda.synchronize()
        raw = buf.cpu().numpy()
        assert np.array_equal(raw[guard + off:guard + off + n].reshape(Hh, W, 3), want), "offset %d" % off
        assert (raw[:guard] == 0xAA).all() and (raw[guard + off + n:] == 0xAA).all(), "offset %d: a guard byte changed" % off
        got = d.get_frame_buffer()
        assert np.array_equal(got, f["fb"] if place == "out" else want)
        d.close()


VOTE_W, VOTE_H, VOTE_R = 512, 64, 8
VOTE_AT = np.array([[-0.5, 0.0, 0.0, 2.0]], np.float32)    # larger than the frame: its flat middle fills whole tiles


def vote_params(f):
    """Focus on the nearest depth of the snapshot with a range of three tenths of it: the model's middle is sharp, its
    rim partly blurred."""
    z = f["z"][bits(f["z"]) != F32_MIN_BITS]
    near = float(z.max())
    return P(near, 6.0 / (0.3 * near), R=VOTE_R, rng=0.3 * near)


def vote_tiles(f, p, want):
    """[tiles_y, tiles_x] bool each, from the snapshot: (a) every circle of the tile itself is 0, a circle >= 2 lies in
    its halo and a pixel of it changes; (b) the largest circle k_dof stages for it -- the tile and max_radius pixels
    around, inside the frame -- lies strictly between 0 and max_radius; (c) drawn, nothing staged above 0, unchanged."""
    import tiny_renderer_amd as T
    coc = T.dof_coc(p, f["z"]).astype(np.int64)
    R = int(p.max_radius)
    changed = tiles_any((want != f["fb"]).any(-1)[::-1])
    drawn = tiles_any(bits(f["z"]) != F32_MIN_BITS)
    own, staged = np.zeros_like(changed, np.int64), np.zeros_like(changed, np.int64)
    for j, i in np.ndindex(*changed.shape):
        own[j, i] = coc[j * 16:j * 16 + 16, i * 128:i * 128 + 128].max()
        staged[j, i] = coc[max(j * 16 - R, 0):j * 16 + 16 + R, max(i * 128 - R, 0):i * 128 + 128 + R].max()
    return (own == 0) & (staged >= 2) & changed, (staged > 0) & (staged < R), drawn & (staged == 0) & ~changed


def assert_vote_tiles(f, p, want):
    a, b, c = vote_tiles(f, p, want)
    assert a.any(), "no tile with circles of 0 alone takes colour from a circle >= 2 in its halo"
    assert b.any(), "no tile whose tap loops stop between 0 and max_radius"
    assert c.any(), "no drawn tile that is a plain copy"
    return a, b, c


@pytest.mark.gpu
@pytest.mark.parametrize("store_depth", [False, True], ids=["transient", "stored"])
def test_the_vote_counts_the_halo(small_synthetic, store_depth):
    """4 x 4 tiles of the three kinds of vote_tiles: a vote over the tile's own pixels alone would copy the tiles of
    kind (a)."""
    s = scene(VOTE_W, VOTE_H, small_synthetic, "phong", VOTE_AT, store_depth=store_depth)
    drive(s)
    f = snap(s)
    p = vote_params(f)
    want = host(f, p)
    a, b, c = assert_vote_tiles(f, p, want)
    drive(s)
    got = s.get_depth_of_field(p)
    assert np.array_equal(got, want), "out of place: tiles %r differ" % (np.argwhere(tiles_any((got != want).any(-1)[::-1])).tolist(),)
    s.depth_of_field(p)
    got = s.get_frame_buffer()
    assert np.array_equal(got, want), "in place: tiles %r differ" % (np.argwhere(tiles_any((got != want).any(-1)[::-1])).tolist(),)
    s.close()


STALE_W, STALE_H = 512, 64
STALE_FIRST = np.array([[0.0, 0.0, 0.3, 1.0]], np.float32)
STALE_THEN = ((-0.5, 0.0), (0.45, -0.1))


def stale_fields(first, then, flags):
    """What a kernel that ignored the z flags, or the colour flags, of the tiles around its own would read: the first
    frame's z, or colour, in the tiles `flags` calls clean, the second frame's elsewhere."""
    flagged = np.repeat(np.repeat(flags, 16, 0), 128, 1)[:then["z"].shape[0], :then["z"].shape[1]]
    return ({"z": np.where(flagged, first["z"], then["z"]), "fb": then["fb"]},
            {"z": then["z"], "fb": np.where(flagged[::-1, :, None], first["fb"], then["fb"])})


def assert_stale_halo(first, then, flags, p, want):
    """A tile that is clean now and was drawn before lies next to a tile that is drawn now, and either stale field
    would show in the result."""
    was = tiles_any(bits(first["z"]) != F32_MIN_BITS)
    old = flags & was
    assert old.any(), "no tile is clean now and was drawn before"
    reach = False
    for j, i in zip(*np.nonzero(old)):
        reach = reach or (~flags[max(j - 1, 0):j + 2, max(i - 1, 0):i + 2]).any()
    assert reach, "no such tile lies next to a drawn one"
    for name, field in zip(("z", "colour"), stale_fields(first, then, flags)):
        assert not np.array_equal(host(field, p), want), "stale %s would not show" % name


@pytest.mark.gpu
@pytest.mark.parametrize("store_depth", [False, True], ids=["transient", "stored"])
@pytest.mark.parametrize("x,y", STALE_THEN)
def test_a_stale_halo_reads_as_not_drawn(small_synthetic, x, y, store_depth):
    """A large frame first (its depth in memory: stored, or fetched by one read of THAT frame), then the model moved to a
    small place and rendered again with nothing read in between: the tiles it leaves hold the large frame's z behind
    raised flags when k_dof stages its halos.  (Their COLOUR is zeros in memory by then -- a render stores zeros over a
    tile it leaves, measured on a caller's buffer -- so k_dof ignoring the colour flags of its neighbours passes here.)
    The expectation comes from scenes that rendered one frame each."""
    W, Hh = STALE_W, STALE_H
    one = scene(W, Hh, small_synthetic, "phong", STALE_FIRST, store_depth=store_depth)
    drive(one)
    first = snap(one)
    one.close()
    twin = scene(W, Hh, small_synthetic, "phong", TC._small(x, y), store_depth=store_depth)
    drive(twin)
    flags = clean_flags(twin)
    then = snap(twin)
    twin.close()
    p = params_for(then, 8, near=True)
    want = host(then, p)
    assert_stale_halo(first, then, flags, p, want)
    s = scene(W, Hh, small_synthetic, "phong", STALE_FIRST, store_depth=store_depth)
    drive(s)
    if not store_depth:
        assert np.array_equal(bits(s.read_z_f32()), bits(first["z"]))
    assert s.sync() == 0
    s.set_instances(TC._small(x, y))
    drive(s)
    assert np.array_equal(s.get_depth_of_field(p), want), "out of place"
    s.depth_of_field(p)
    assert np.array_equal(s.get_frame_buffer(), want), "in place"
    assert np.array_equal(bits(s.read_z_f32()), bits(then["z"]))
    s.close()


@pytest.mark.gpu
def test_colour_over_undrawn_z_after_an_average_in_place(small_synthetic):
    """z flag up, colour flag down: accumulate_in_place leaves colour of older frames in tiles the newest frame did not
    draw.  background_radius 0 keeps it, 3 spreads it."""
    from tests import test_accumulate as TA
    W, Hh, n = 384, 48, 4
    par = TA.views(n)
    ref = scene(W, Hh, small_synthetic, "phong", frames_per_launch=n)
    ref.render_frames(par)
    avg = TA.oracle(TA.kept(ref, n))
    f = {"fb": avg, "z": ref.read_z_f32()}
    ref.close()
    s = scene(W, Hh, small_synthetic, "phong", frames_per_launch=n)
    s.render_frames(par)
    s.accumulate_in_place(n)
    flags = clean_flags(s)
    mixed = ~tiles_any(bits(f["z"]) != F32_MIN_BITS) & ~flags & tiles_any(avg[::-1].any(-1))
    assert mixed.any(), "no tile holds colour over undrawn z behind a lowered colour flag"
    px = np.repeat(np.repeat(mixed, 16, 0), 128, 1)[::-1]
    want = {bg: host(f, params_for(f, 3, bg)) for bg in (0, 3)}
    assert not np.array_equal(want[0], avg) and not np.array_equal(want[3][px], want[0][px]), "the background radius does not show"
    assert np.array_equal(s.get_depth_of_field(params_for(f, 3, 0)), want[0])
    s.depth_of_field(params_for(f, 3, 3))
    assert np.array_equal(s.get_frame_buffer(), want[3])
    assert not (clean_flags(s) & tiles_any(want[3][::-1].any(-1))).any(), "a tile with colour in it is flagged clean"
    assert np.array_equal(bits(s.read_z_f32()), bits(f["z"]))
    s.close()


@pytest.mark.gpu
def test_a_trusted_buffer_whose_flags_are_up_over_drawn_z(small_synthetic):
    """z flag down, colour flag up (the setup of tests/test_ambient_occlusion.py): two trusted caller's buffers, the
    model on the left rendered into the first, on the right into the second, the first handed over again.  Its colour
    reads as zeros where its flags are up, under the circles of the second frame's z."""
    import torch
    W, Hh = 512, 64
    bufs = [torch.zeros(W * Hh * 3, dtype=torch.uint8, device="cuda") for _ in range(2)]
    torch.cuda.synchronize()
    s = scene(W, Hh, small_synthetic, "phong", TC._small(-0.5, 0.0), frame_buffer_device=bufs[0].data_ptr(),
              trust_frame_buffers=True, auto_group=False)
    drive(s)
    left, flags = s.get_frame_buffer(), clean_flags(s)
    s.set_frame_buffer_device(bufs[1].data_ptr())
    s.set_instances(TC._small(0.5, 0.0))
    drive(s)
    z = s.read_z_f32()
    s.set_frame_buffer_device(bufs[0].data_ptr())
    assert np.array_equal(clean_flags(s), flags), "a trusted buffer keeps its flags"
    assert (flags & tiles_any(bits(z) != F32_MIN_BITS)).any(), "no flag is up over a drawn tile: the case shows nothing"
    f = {"z": z, "fb": left}
    p = params_for(f, 8, bg=2)
    want = host(f, p)
    assert not np.array_equal(want, left)
    s.depth_of_field(p)
    assert np.array_equal(s.resolve(2), box(want, 2)), "a consumer that skips clean tiles lost blurred pixels"
    assert not (clean_flags(s) & tiles_any(want[::-1].any(-1))).any()
    assert np.array_equal(s.get_frame_buffer(), want)
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("buffers", ["own", "callers"])
@pytest.mark.parametrize("store_depth", [False, True], ids=["transient", "stored"])
def test_state_kept_frames_blur_the_selected_frame_only(small_synthetic, store_depth, buffers):
    """Five views at four frames a launch; frame 1 is blurred in place with ITS z (rebuilt from the slot's own
    parameters when depth is transient), every other kept frame and every z stays."""
    import torch
    W, Hh, n = 208, 40, 5
    par = TC._params(n)
    kept, want, p = [], None, None
    for twin in (True, False):
        s = scene(W, Hh, small_synthetic, "phong", AT, frames_per_launch=4, store_depth=store_depth)
        store = torch.zeros(n * (W * Hh * 3 + 64), dtype=torch.uint8, device="cuda") if buffers == "callers" else None
        torch.cuda.synchronize()
        s.render_frames(par, None if store is None else [store.data_ptr() + k * (W * Hh * 3 + 64) for k in range(n)])
        assert s.frames_kept() >= 3
        if twin:
            for back in range(3):
                s.select_frame(back)
                kept.append(snap(s))
            p = params_for(kept[1], 3)
            want = host(kept[1], p)
            assert not np.array_equal(want, kept[1]["fb"]) and not np.array_equal(want, host(dict(kept[1], z=kept[0]["z"]), p))
        else:
            s.select_frame(1)
            s.depth_of_field(p)
            assert np.array_equal(s.get_frame_buffer(), want)
            for back in (0, 2):
                s.select_frame(back)
                TC.same(snap(s), kept[back])
            s.select_frame(1)
            assert np.array_equal(s.get_frame_buffer(), want) and np.array_equal(bits(s.read_z_f32()), bits(kept[1]["z"]))
        s.close()


@pytest.mark.gpu
def test_what_follows_a_blur_in_place(small_synthetic):
    """A render without a clear on top of the blurred frame depth-tests against the unchanged z; resolve after
    TR_DOF_SHOW_COC in place with a background radius reads the undrawn tiles, which are grey now."""
    W, Hh = 512, 64
    mk = lambda: scene(W, Hh, small_synthetic, "phong", TC._small(-0.4, 0.1))
    ref = mk()
    drive(ref)
    f, flags = snap(ref), None
    drive(ref, cam=-0.6)
    f2 = snap(ref)
    ref.close()
    p = params_for(f, 8, near=True)
    blurred = dict(f, fb=host(f, p), win=None)
    want, wins = TC.merge(blurred, dict(f2, win=None))
    assert wins.any() and not wins.all() and not np.array_equal(blurred["fb"], f["fb"])
    s = mk()
    drive(s)
    flags = clean_flags(s)
    s.depth_of_field(p)
    drive(s, cam=-0.6, clear=False)
    TC.same(snap(s), want)
    show = params_for(f, 8, bg=1, flags=1)
    grey = host(f, show)
    undrawn = flags & ~tiles_any(bits(f["z"]) != F32_MIN_BITS)
    assert undrawn.any()
    drive(s)
    assert np.array_equal(clean_flags(s), flags)
    s.depth_of_field(show)
    half = s.resolve(2)
    assert np.array_equal(half, box(grey, 2))
    for j, i in zip(*np.nonzero(undrawn)):
        assert half[::-1][j * 8:j * 8 + 8, i * 64:i * 64 + 64].all(), "the undrawn tile (%d, %d) is not grey in the resolved frame" % (j, i)
    assert not clean_flags(s).any(), "a grey tile kept its flag"
    s.close()


@pytest.mark.gpu
def test_profile_shows_one_launch_per_call(small_synthetic):
    s = scene(256, 48, small_synthetic, "phong", AT)
    s.profile_enable(True)
    drive(s)
    p = P(0.0, 1.0, R=2)
    s.depth_of_field(p)
    s.get_depth_of_field(P(0.0, 1.0, R=8, flags=1))
    assert s.sync() == 0
    prof = s.profile_read()
    assert prof.get("k_dof", {}).get("launches") == 2 and prof["k_dof"]["total_ms"] > 0.0, prof
    s.close()


@pytest.mark.gpu
def test_cli_dof_writes_the_host_rule_of_the_plain_run(african_head, tmp_path):
    import tiny_renderer_amd as T
    from tiny_renderer_amd import cli
    common = ["-p", H.asset_dir("african_head"), "-s", "phong", "--width", "256", "--height", "128", "--camera-angle", "0.3",
              "--light-angle", "0.7"]
    mesh, texs = african_head
    s = scene(256, 128, (mesh, texs), "phong")
    drive(s)
    f = snap(s)
    s.close()
    p = params_for(f, 4)
    plain, soft = (str(tmp_path / n) for n in ("plain.ppm", "dof.ppm"))
    assert cli.main(common + ["--out", plain]) == 0
    assert cli.main(common + ["--dof-focus=%r" % float(p.focus), "--dof-scale=%r" % float(p.scale), "--dof-range=%r" % float(p.range),
                              "--out", soft]) == 0
    hd = b"P6\n256 128\n255\n"
    a, b = (np.frombuffer(open(q, "rb").read()[len(hd):], np.uint8).reshape(128, 256, 3) for q in (plain, soft))
    assert np.array_equal(f["fb"], a)
    assert not np.array_equal(a, b) and np.array_equal(b, T.depth_of_field_host(f["z"], a, p))
