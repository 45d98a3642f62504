"""Shared shadows: tr_scene_render_shadow_pass / tr_scene_render_colour_pass (the two passes of `shadow` and `occlusion`
as calls of their own), tr_scene_shadow_merge (k_shadow_merge) and tr_shadow_merge_host.

The rule, from the words of include/tiny_renderer.h: per pixel `if (zs >= zd) zd = zs` -- the reference's light-space
test (shader.rs:703, 841), a running maximum without culling -- so the shadow buffer of the concatenated mesh A ++ B is A's
merged with B's, and shadow passes, a merge both ways, colour passes and tr_scene_composite give, bit for bit, one scene
of A ++ B.  The contract is exact: every comparison is np.array_equal (floats through their bits).

On the CPU the argument itself is pinned on the oracle.  On the GPU the expectation is either the oracle / a twin scene
that renders the whole frame in one call, or the rule applied to what an identically driven second pair of scenes
returns (reading a shadow buffer makes it plain memory and lowers its flags, so the pair that is merged is not read
before the merge)."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from tests import helpers as H

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TWO_PASS = ("shadow", "occlusion")
ONE_PASS = ("default", "phong", "normal_map", "specular", "darboux")
F32_MIN_BITS = np.uint32(0xFF7FFFFF)
F32_MIN = F32_MIN_BITS.view(np.float32)
NO_WINNER = 0xFFFFFFFF
CAM, LIGHT = 0.3, 0.7


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def rule(zd, zs):
    """if (zs >= zd) zd = zs, on bits (a NaN compares false: dst keeps its value)."""
    zd, zs = np.ascontiguousarray(zd, np.float32), np.ascontiguousarray(zs, np.float32)
    with np.errstate(invalid="ignore"):
        take = zs >= zd
    return np.where(take, bits(zs), bits(zd)).view(np.float32)


def concat(a, b):
    """The mesh A ++ B: arrays concatenated, B's indices offset by A's counts."""
    ia, ib = np.asarray(a["idx"], np.uint32).reshape(-1, 9), np.asarray(b["idx"], np.uint32).reshape(-1, 9).copy()
    n = [np.asarray(a[k]).reshape(-1, 3).shape[0] for k in ("pos", "tex", "nrm")]
    for col in range(9):
        ib[:, col] += np.uint32(n[col % 3])
    out = {k: np.concatenate([np.asarray(a[k], np.float32).reshape(-1, 3), np.asarray(b[k], np.float32).reshape(-1, 3)])
           for k in ("pos", "tex", "nrm")}
    out["idx"] = np.concatenate([ia, ib])
    return out


def n_tri(mesh):
    return np.asarray(mesh["idx"]).reshape(-1, 9).shape[0]


def aim(s, cam=CAM, light=LIGHT):
    s.set_light_direction(H.light(light)), s.set_camera(*H.camera(cam))


def drive(s, cam=CAM, light=LIGHT, clear=True):
    if clear:
        s.clear()
    aim(s, cam, light)
    s.render()


def split(s, cam=CAM, light=LIGHT, clear=True):
    """A frame pass by pass."""
    if clear:
        s.clear()
    aim(s, cam, light)
    s.render_shadow_pass(), s.render_colour_pass()


def oracle_frame(W, Hh, mesh, texs, pipe, cam=CAM, light=LIGHT, band=None, again=None):
    """The oracle's frame after clear + render; again = (cam, light): a second render without a clear on top."""
    from oracle import oracle as O
    s = O.Scene(W, Hh, mesh, texs, pipe)
    if band is not None:
        s.set_output_band(*band)
    drive(s, cam, light)
    if again is not None:
        drive(s, again[0], again[1], clear=False)
    out = {"fb": s.get_frame_buffer(), "z": s.z_f32(), "win": s.winner_u32(), "shadow": s.shadow_f32()}
    s.close()
    return out


def snap(s, strict=True):
    """The frame as the getters return it, shadow buffer included."""
    out = {"fb": s.get_frame_buffer(strict=strict), "z": s.read_z_f32(), "shadow": s.read_shadow_f32()}
    out["win"] = s.read_winner_u32() if getattr(s, "_tap", False) else None
    return out


def same(got, want, rows=None, what=""):
    """Every byte of two frames; rows = (y0, y1), y up: z and winner words inside those rows only (a band scene's)."""
    sl = slice(None) if rows is None else slice(rows[0], rows[1])
    assert np.array_equal(got["fb"], want["fb"]), "%s colour differs in %d bytes" % (what, int((got["fb"] != want["fb"]).sum()))
    assert np.array_equal(bits(got["z"][sl]), bits(want["z"][sl])), what + " z differs"
    assert np.array_equal(bits(got["shadow"]), bits(want["shadow"])), what + " shadow buffer differs"
    if got.get("win") is not None and want.get("win") is not None:
        assert np.array_equal(got["win"][sl], want["win"][sl]), what + " winner differs"


def scene(W, Hh, ms, pipe, at=None, tap=False, **kw):
    import tiny_renderer_amd as T
    s = T.Scene(W, Hh, ms[0], ms[1], pipe, winner_tap=tap, instances=at, **kw)
    s._tap = tap
    return s


def tiles_any(mask):
    """[tiles_y, tiles_x] bool of a [H, W] mask with y up: does the 128 x 16 tile hold a set pixel?"""
    Hh, W = mask.shape
    ty, tx = (Hh + 15) // 16, (W + 127) // 128
    out = np.zeros((ty, tx), bool)
    for j in range(ty):
        for i in range(tx):
            out[j, i] = mask[j * 16:j * 16 + 16, i * 128:i * 128 + 128].any()
    return out


# The pairs.  B stands between the light and A (the light sits at H.light(LIGHT) and looks at the origin), so that B's
# shadow falls on A where the camera sees it.
def _toward_light(d, scale):
    l = np.array(H.light(LIGHT), np.float32)
    return np.array([[d * l[0], 0.1, d * l[2], scale]], np.float32)


A_AT = np.array([[-0.1, 0.0, -0.2, 0.7]], np.float32)
B_AT = _toward_light(0.75, 0.3)


@pytest.fixture(scope="module")
def other_synthetic(built):
    """A second object (another mesh; images of its own, for the scenes that do not have to equal a concatenated one)."""
    import tiny_renderer_amd as T
    return T.synthetic_scene(n_lat=9, n_lon=17, tex_size=128, radius=0.75)


@pytest.fixture(scope="module")
def synthetic_pair(small_synthetic, other_synthetic):
    """(A, B, textures): the two synthetic meshes placed on the host, drawn with A's images (a concatenated scene has one
    set of textures)."""
    import tiny_renderer_amd as T
    return T.apply_instances(small_synthetic[0], A_AT), T.apply_instances(other_synthetic[0], B_AT), small_synthetic[1]


@pytest.fixture(scope="module")
def real_pair(african_head, diablo):
    import tiny_renderer_amd as T
    (A, texs), (B, _) = african_head, diablo
    return A, T.apply_instances(B, _toward_light(0.9, 0.35)), texs


# ------------------------------------------------------------------------------------------------------------------
# CPU
# ------------------------------------------------------------------------------------------------------------------

def test_entry_points_declared_exported_and_typed(built):
    import tiny_renderer_amd as T
    from tiny_renderer_amd import _lib
    header = open(os.path.join(REPO, "include", "tiny_renderer.h")).read()
    assert re.search(r"int\s+tr_scene_render_shadow_pass\(tr_scene \*s\);", header)
    assert re.search(r"int\s+tr_scene_render_colour_pass\(tr_scene \*s\);", header)
    assert re.search(r"int\s+tr_scene_shadow_merge\(tr_scene \*dst, tr_scene \*src\);", header)
    assert re.search(r"int\s+tr_shadow_merge_host\(size_t n, float \*dst, const float \*src\);", header)
    exports = open(os.path.join(REPO, "tiny_renderer_amd", "csrc", "exports.map")).read()
    assert "tr_*" in exports
    raw = C.CDLL(_lib.library_path())
    for name in ("tr_scene_render_shadow_pass", "tr_scene_render_colour_pass", "tr_scene_shadow_merge", "tr_shadow_merge_host"):
        assert hasattr(raw, name), name + " is not exported"
        assert name in _lib.SYMBOLS
    assert _lib.SYMBOLS["tr_scene_render_shadow_pass"] == (C.c_int, [C.c_void_p])
    assert _lib.SYMBOLS["tr_scene_render_colour_pass"] == (C.c_int, [C.c_void_p])
    assert _lib.SYMBOLS["tr_scene_shadow_merge"] == (C.c_int, [C.c_void_p, C.c_void_p])
    assert _lib.SYMBOLS["tr_shadow_merge_host"] == (C.c_int, [C.c_size_t, C.c_void_p, C.c_void_p])
    L = T.load_library()
    # null scenes are refused on the host, with a text
    assert L.tr_scene_shadow_merge(None, None) == _lib.TR_E_INVALID and b"null" in L.tr_last_error()
    assert L.tr_scene_render_shadow_pass(None) == _lib.TR_E_INVALID and b"null" in L.tr_last_error()
    assert L.tr_scene_render_colour_pass(None) == _lib.TR_E_INVALID and b"null" in L.tr_last_error()
    for name in ("shadow_merge_host",):
        assert callable(getattr(T, name))
    for name in ("render_shadow_pass", "render_colour_pass", "shadow_merge"):
        assert callable(getattr(T.Scene, name))
    # the rule lives in a header of its own, shared by the kernel and the host entry point
    assert os.path.isfile(os.path.join(REPO, "tiny_renderer_amd", "csrc", "tr_shadow_merge.h"))


def test_host_rule_equals_the_numpy_rule_on_edge_values(built):
    import tiny_renderer_amd as T
    from tiny_renderer_amd import _lib
    rng = np.random.default_rng(11)
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    special = np.array([0.0, -0.0, 1.0, -1.0, 255.0, inf, -inf, nan, F32_MIN, np.finfo(np.float32).max, 1e-45, -1e-45], np.float32)
    zs = np.repeat(special, len(special))
    zd = np.tile(special, len(special))
    r = rng.normal(0.0, 100.0, 3000).astype(np.float32)
    zs = np.concatenate([zs, r, r[:300], np.array([0x7FC12345], np.uint32).view(np.float32), np.array([1.0], np.float32)])
    zd = np.concatenate([zd, np.roll(r, 1), r[:300], np.array([1.0], np.float32), np.array([0x7FC12345], np.uint32).view(np.float32)])
    want = rule(zd, zs)
    at = {(float(a) if a == a else "nan", float(b) if b == b else "nan", bool(np.signbit(a)), bool(np.signbit(b))): k
          for k, (a, b) in enumerate(zip(zs[:len(special) ** 2], zd[:len(special) ** 2]))}
    b_ = bits(want)
    fmin = float(F32_MIN)
    # the cases by name, on the rule itself: (zs, zd, sign of zs, sign of zd)
    assert b_[at[(fmin, 1.0, True, False)]] == bits(np.float32(1.0))[0]          # f32::MIN in src replaces nothing drawn
    assert b_[at[(1.0, fmin, False, True)]] == bits(np.float32(1.0))[0]          # ... and anything drawn replaces it
    assert b_[at[(fmin, fmin, True, True)]] == F32_MIN_BITS
    assert b_[at[(1.0, 1.0, False, False)]] == bits(np.float32(1.0))[0]          # equal values
    assert b_[at[(0.0, 0.0, False, True)]] == 0x00000000                         # +0.0 into -0.0: src's sign wins
    assert b_[at[(0.0, 0.0, True, False)]] == 0x80000000                         # -0.0 into +0.0: src's sign wins
    assert b_[at[(float(inf), 255.0, False, False)]] == 0x7F800000 and b_[at[(255.0, float(inf), False, False)]] == 0x7F800000
    assert b_[at[(float(-inf), fmin, True, True)]] == F32_MIN_BITS               # -inf < f32::MIN: never enters
    assert b_[at[(fmin, float(-inf), True, True)]] == F32_MIN_BITS
    assert b_[at[("nan", 1.0, False, False)]] == bits(np.float32(1.0))[0]        # a NaN never enters the buffer
    assert np.isnan(want[at[(1.0, "nan", False, False)]])                        # ... and one that is there stays
    assert b_[-2] == bits(np.float32(1.0))[0] and b_[-1] == 0x7FC12345           # payload bits travel untouched
    got = T.shadow_merge_host(zd, zs)
    assert np.array_equal(bits(got), bits(want))
    keep = zd.copy()
    T.shadow_merge_host(zd, zs)
    assert np.array_equal(bits(zd), bits(keep)), "the wrapper leaves its arguments alone"
    # the raw entry point: in place, n == 0, NULL with n > 0
    L = T.load_library()
    z2 = zd.copy()
    assert L.tr_shadow_merge_host(z2.size, z2.ctypes.data, zs.ctypes.data) == 0
    assert np.array_equal(bits(z2), bits(want))
    assert L.tr_shadow_merge_host(0, None, None) == 0
    assert L.tr_shadow_merge_host(0, z2.ctypes.data, None) == 0
    assert L.tr_shadow_merge_host(4, None, zs.ctypes.data) == _lib.TR_E_INVALID and b"null" in L.tr_last_error()
    assert L.tr_shadow_merge_host(4, z2.ctypes.data, None) == _lib.TR_E_INVALID
    assert np.array_equal(bits(z2), bits(want))
    with pytest.raises(ValueError):
        T.shadow_merge_host(zd, zs[:-1])


@functools.lru_cache(maxsize=None)
def _oracle_shadow(key):
    """Oracle shadow buffers, rendered once per (pipeline, mesh, size) and shared (never modified)."""
    pipe, which, W, Hh = key
    return oracle_frame(W, Hh, _oracle_shadow.meshes[which], _oracle_shadow.texs[which[0]], pipe)["shadow"]


_oracle_shadow.meshes, _oracle_shadow.texs = {}, {}


@pytest.mark.parametrize("case", ["real800x800", "synthetic208x40"])
@pytest.mark.parametrize("pipe", TWO_PASS)
def test_merged_oracle_shadow_buffers_equal_the_oracle_of_the_concatenated_mesh(built, request, pipe, case):
    """The argument the feature rests on: oracle shadow_f32(A) merged by the HOST rule with shadow_f32(B) -- same light,
    camera and textures -- is shadow_f32(A ++ B) in every bit; and so it is with B first and A merged second."""
    import tiny_renderer_amd as T
    if case.startswith("real"):
        A, B, texs = request.getfixturevalue("real_pair")
        W = Hh = 800
    else:
        A, B, texs = request.getfixturevalue("synthetic_pair")
        W, Hh = 208, 40
    tag = case[0]
    _oracle_shadow.meshes.update({tag + "A": A, tag + "B": B, tag + "AB": concat(A, B)})
    _oracle_shadow.texs[tag] = texs
    sa, sb, sab = (_oracle_shadow((pipe, tag + k, W, Hh)) for k in ("A", "B", "AB"))
    drawn_a, drawn_b = bits(sa) != F32_MIN_BITS, bits(sb) != F32_MIN_BITS
    assert (drawn_a & drawn_b).any() and (drawn_a & ~drawn_b).any() and (~drawn_a & ~drawn_b).any()
    assert not np.array_equal(bits(sa), bits(sab)) and not np.array_equal(bits(sb), bits(sab))
    assert np.array_equal(bits(T.shadow_merge_host(sa, sb)), bits(sab)), "A <- B is not the buffer of A ++ B"
    assert np.array_equal(bits(T.shadow_merge_host(sb, sa)), bits(sab)), "B <- A is not the buffer of A ++ B"
    assert np.array_equal(bits(rule(sa, sb)), bits(sab))


def test_python_methods_reject_what_the_host_can_decide():
    """Scene.shadow_merge refuses itself, a non-scene, a size mismatch and a one-pass pipeline on either side, and the
    split passes refuse a one-pass pipeline, with ValueError before anything reaches the library (no handles here)."""
    import tiny_renderer_amd as T
    a, b = T.Scene.__new__(T.Scene), T.Scene.__new__(T.Scene)
    for s, (w, h) in ((a, (640, 480)), (b, (640, 482))):
        s.width, s.height, s._h, s._pinned, s.pipeline = w, h, None, [], "shadow"
    for bad in (a, None, b):
        with pytest.raises(ValueError):
            a.shadow_merge(bad)
    with pytest.raises(ValueError):
        b.shadow_merge(a)
    b.height = 480
    for pipe in ONE_PASS:
        b.pipeline = pipe
        with pytest.raises(ValueError):
            a.shadow_merge(b)
        with pytest.raises(ValueError):
            b.shadow_merge(a)
        with pytest.raises(ValueError):
            b.render_shadow_pass()
        with pytest.raises(ValueError):
            b.render_colour_pass()


# ------------------------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------------------------

SIZES = ((256, 32, None), (208, 40, None), (200, 40, None), (256, 48, (16, 32)))
MODES = {"transient": {}, "stored": {"store_depth": True}, "tap": {"tap": True}}


def band_y(Hh, band):
    return None if band is None else (Hh - band[1], Hh - band[0])


@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("W,Hh,band", SIZES, ids=["256x32", "208x40", "200x40", "256x48band"])
@pytest.mark.parametrize("pipe", TWO_PASS)
def test_the_split_is_the_whole(small_synthetic, pipe, W, Hh, band, mode):
    """clear; render_shadow_pass; render_colour_pass is clear; render on a twin scene, and the oracle: frame, z, shadow
    bits and winner -- whole tiles, a ragged right edge, a width that is no multiple of 16, a band."""
    kw = dict(MODES[mode])
    if band is not None:
        kw["band_rows"] = band
    at = np.array([[0.1, 0.0, 0.0, 0.9]], np.float32)
    a, twin = scene(W, Hh, small_synthetic, pipe, at, **kw), scene(W, Hh, small_synthetic, pipe, at, **kw)
    split(a), drive(twin)
    got, want = snap(a), snap(twin)
    same(got, want, what="twin:")
    import tiny_renderer_amd as T
    cpu = oracle_frame(W, Hh, T.apply_instances(small_synthetic[0], at), small_synthetic[1], pipe, band=band)
    assert (cpu["win"] != NO_WINNER).sum() > 200 and (bits(cpu["shadow"]) != F32_MIN_BITS).sum() > 200
    same(got, cpu, band_y(Hh, band), what="oracle:")
    # once more without a clear, under another camera: both passes on top of the frame so far, as render does
    split(a, cam=-0.5, clear=False), drive(twin, cam=-0.5, clear=False)
    same(snap(a), snap(twin), what="on top:")
    a.close(), twin.close()


def _pair(W, Hh, small_synthetic, other_synthetic, pipes=("shadow", "shadow"), at=(A_AT, B_AT), **kw):
    return (scene(W, Hh, small_synthetic, pipes[0], at[0], **kw), scene(W, Hh, other_synthetic, pipes[1], at[1], **kw))


@pytest.mark.gpu
@pytest.mark.parametrize("direction", ["a<-b", "b<-a"])
@pytest.mark.parametrize("W,Hh,band", SIZES, ids=["256x32", "208x40", "200x40", "256x48band"])
@pytest.mark.parametrize("pipes", [("shadow", "occlusion"), ("occlusion", "shadow")], ids=["shadow+occlusion", "occlusion+shadow"])
def test_merge_equals_the_host_rule_on_the_scenes_own_buffers(small_synthetic, other_synthetic, pipes, W, Hh, band, direction):
    """Read before (a twin pair), merged on the device, read after: dst's shadow buffer is the rule's, src is untouched,
    dst's frame, z and winner are untouched.  dst a band scene, src a scene of the whole frame: bands need not match."""
    import tiny_renderer_amd as T
    want = None
    rows_d, rows_s = (band_y(Hh, band), None) if direction == "a<-b" else (None, band_y(Hh, band))
    for twin in (True, False):
        a = scene(W, Hh, small_synthetic, pipes[0], A_AT, tap=True, **({} if band is None else {"band_rows": band}))
        b = scene(W, Hh, other_synthetic, pipes[1], B_AT, tap=True)
        d, s = (a, b) if direction == "a<-b" else (b, a)
        drive(d), drive(s)
        if twin:
            fd, fs = snap(d), snap(s)
            want = dict(fd, shadow=rule(fd["shadow"], fs["shadow"]))
            assert not np.array_equal(bits(want["shadow"]), bits(fd["shadow"])), "the case is vacuous"
            assert np.array_equal(bits(want["shadow"]), bits(T.shadow_merge_host(fd["shadow"], fs["shadow"])))
        else:
            d.shadow_merge(s)
            assert d.sync() == 0
            same(snap(d), want, rows_d, what="dst:")
            same(snap(s), fs, rows_s, what="src:")
        a.close(), b.close()


def _small(x, y, z=0.0, scale=0.4):
    return np.array([[x, y, z, scale]], np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("W", [512, 500], ids=["wide", "narrow"])
def test_flags_the_three_tile_cases_and_the_profile(small_synthetic, other_synthetic, W):
    """W x 64 is 4 x 4 tiles.  dst draws left of the middle, src right of it, overlapping: tiles src left empty (skipped
    on its flag), tiles src drew and dst left empty (dst's flag up: its stale memory must not be read), tiles both drew.
    dst's buffer is stale on purpose: an earlier frame filled it, then a cleared one left most tiles behind their flags.
    k_shadow_merge runs once."""
    Hh = 64
    at = (_small(-0.5, 0.0), _small(0.2, 0.0, 0.15))
    fd = fs = want = None
    for twin in (True, False):
        d, s = _pair(W, Hh, small_synthetic, other_synthetic, at=(_small(0.0, 0.0, 0.0, 1.2), at[1]))
        drive(d)                              # every tile of dst's buffer written once ...
        d.set_instances(at[0])
        d.clear(), aim(d)
        d.render_shadow_pass()                # ... then the pass that counts: most of them stale behind their flags
        drive(s)
        if twin:
            fd, fs = d.read_shadow_f32(), s.read_shadow_f32()
            td, ts = tiles_any(bits(fd) != F32_MIN_BITS), tiles_any(bits(fs) != F32_MIN_BITS)
            assert (~ts & td).any() and (~ts & ~td).any(), "no tile that src left empty"
            assert (ts & ~td).any(), "no tile that src drew and dst left empty"
            assert (ts & td).any(), "no tile both drew"
            want = rule(fd, fs)
        else:
            d.profile_enable(True)
            d.shadow_merge(s)
            prof = d.profile_read()
            d.profile_enable(False)
            assert prof.get("k_shadow_merge", {}).get("launches") == 1 and prof["k_shadow_merge"]["total_ms"] > 0.0, prof
            # the colour pass that follows on the stream reads through the flags the merge left: the picture of a scene
            # whose buffer was never stale, and not the picture without src's shadow
            d.render_colour_pass()
            ref, alone = (scene(W, Hh, small_synthetic, "shadow", at[0]) for _ in range(2))
            ref.clear(), aim(ref)
            ref.render_shadow_pass(), ref.shadow_merge(s), ref.render_colour_pass()
            drive(alone)
            got, rs = snap(d), snap(ref)
            assert np.array_equal(bits(got["shadow"]), bits(want)) and np.array_equal(bits(rs["shadow"]), bits(want))
            assert np.array_equal(bits(s.read_shadow_f32()), bits(fs)), "src was written"
            assert np.array_equal(got["fb"], rs["fb"]) and np.array_equal(bits(got["z"]), bits(rs["z"]))
            assert not np.array_equal(got["fb"], alone.get_frame_buffer()), "src's shadow does not show"
            ref.close(), alone.close()
        d.close(), s.close()


@pytest.mark.gpu
def test_state_clears_on_either_side(small_synthetic, other_synthetic):
    W, Hh = 208, 40
    d, s = _pair(W, Hh, small_synthetic, other_synthetic)
    ref_d, ref_s = _pair(W, Hh, small_synthetic, other_synthetic)
    drive(ref_d), drive(ref_s)
    fd, fs = snap(ref_d), snap(ref_s)
    # src logically cleared: nothing happens, and its clear stays pending
    drive(d), drive(s)
    s.clear()
    d.shadow_merge(s)
    same(snap(d), fd)
    assert (bits(s.read_shadow_f32()) == F32_MIN_BITS).all()
    # dst with a pending clear: the clear is made real, dst takes src's buffer; its z / colour clear stays pending
    drive(s)
    d.clear()
    d.shadow_merge(s)
    assert np.array_equal(bits(d.read_shadow_f32()), bits(fs["shadow"]))
    assert not d.get_frame_buffer().any() and (bits(d.read_z_f32()) == F32_MIN_BITS).all()
    same(snap(s), fs)
    # a scene nothing was ever rendered into holds the zeros it was created with (Buffer::new): the rule against those
    fresh = scene(W, Hh, small_synthetic, "shadow", A_AT)
    fresh.shadow_merge(s)
    assert np.array_equal(bits(fresh.read_shadow_f32()), bits(rule(np.zeros((Hh, W), np.float32), fs["shadow"])))
    for q in (d, s, ref_d, ref_s, fresh):
        q.close()


def _sequence(a, b, n_a, cam=CAM, light=LIGHT):
    """The full sequence of include/tiny_renderer.h: a holds the picture of both afterwards."""
    for q in (a, b):
        q.clear(), aim(q, cam, light)
    a.render_shadow_pass(), b.render_shadow_pass()
    a.shadow_merge(b), b.shadow_merge(a)
    a.render_colour_pass(), b.render_colour_pass()
    a.composite(b, winner_base=n_a)


def _headline(pair, pipe, W, Hh, oracle=True):
    A, B, texs = pair
    n_a = n_tri(A)
    AB = concat(A, B)
    a, b, both = (scene(W, Hh, (m, texs), pipe, tap=True) for m in (A, B, AB))
    _sequence(a, b, n_a)
    drive(both)
    got, want = snap(a), snap(both)
    assert (want["win"] >= n_a).any() and (want["win"] < n_a).any() and (want["win"] == NO_WINNER).any()
    same(got, want, what="concatenated scene:")
    assert np.array_equal(bits(b.read_shadow_f32()), bits(want["shadow"])), "src holds the merged buffer too"
    if oracle:
        same(got, oracle_frame(W, Hh, AB, texs, pipe), what="oracle:")
    # the same pair without the merge: B throws no shadow on A, and the picture is another
    drive(a), drive(b)
    a.composite(b, winner_base=n_a)
    plain = snap(a)
    assert np.array_equal(plain["win"], want["win"]) and np.array_equal(bits(plain["z"]), bits(want["z"]))
    assert not np.array_equal(plain["fb"], want["fb"]), "the merge changes nothing: the case is vacuous"
    assert not np.array_equal(bits(plain["shadow"]), bits(want["shadow"]))
    for q in (a, b, both):
        q.close()


@pytest.mark.gpu
@pytest.mark.parametrize("W,Hh", [(208, 40), (256, 32)], ids=["208x40", "256x32"])
@pytest.mark.parametrize("pipe", TWO_PASS)
def test_headline_the_sequence_equals_a_scene_of_the_concatenated_mesh(synthetic_pair, pipe, W, Hh):
    """Shadow passes, merge both ways, colour passes, composite with winner_base = n_tri(A): colour, z, winner and shadow
    bits of one scene of A ++ B, in every byte."""
    _headline(synthetic_pair, pipe, W, Hh)


@pytest.mark.gpu
@pytest.mark.parametrize("pipe", TWO_PASS)
def test_headline_at_800x800_on_the_real_models(real_pair, pipe):
    _headline(real_pair, pipe, 800, 800, oracle=False)


@pytest.mark.gpu
def test_downstream_a_render_without_clear_on_the_merged_frame(synthetic_pair):
    """After the sequence a render of dst without a clear depth-tests against the merged z and shades against the merged
    shadow buffer: the oracle of A ++ B rendered, then A ... which no oracle draws; so the expectation is the depth rule
    (tests/test_composite.py) applied to the merged frame and to A's next frame alone, shaded under the merged buffer."""
    A, B, texs = synthetic_pair
    W, Hh, pipe = 208, 40, "shadow"
    n_a = n_tri(A)
    a, b, top = (scene(W, Hh, (m, texs), pipe, tap=True) for m in (A, B, A))
    _sequence(a, b, n_a)
    merged = snap(a)
    # A alone under the next camera, its shadow buffer the merged one
    top.clear(), aim(top, cam=-0.6)
    top.render_shadow_pass(), top.shadow_merge(b), top.render_colour_pass()
    f2 = snap(top)
    assert np.array_equal(bits(f2["shadow"]), bits(merged["shadow"]))
    covered = bits(f2["z"]) != F32_MIN_BITS
    with np.errstate(invalid="ignore"):
        wins = covered & ~(f2["z"] <= merged["z"])
    assert wins.any() and (covered & ~wins).any()
    want = {"fb": np.where(wins[::-1, :, None], f2["fb"], merged["fb"]), "z": np.where(wins, f2["z"], merged["z"]),
            "win": np.where(wins, f2["win"], merged["win"]), "shadow": merged["shadow"]}
    drive(a, cam=-0.6, clear=False)
    same(snap(a), want)
    for q in (a, b, top):
        q.close()


@pytest.mark.gpu
def test_errors_change_nothing(small_synthetic, other_synthetic):
    import tiny_renderer_amd as T
    from tiny_renderer_amd import _lib
    L = T.load_library()
    W, Hh = 256, 32
    d = scene(W, Hh, small_synthetic, "shadow", A_AT, tap=True)
    drive(d)
    before = snap(d)
    cases = {
        "width": scene(W + 16, Hh, other_synthetic, "shadow", B_AT),
        "height": scene(W, Hh + 8, other_synthetic, "shadow", B_AT),
        "one pass": scene(W, Hh, other_synthetic, "phong", B_AT),
        "matrices": scene(W, Hh, other_synthetic, "occlusion", B_AT),
    }
    for word, s in cases.items():
        drive(s, light=0.2 if word == "matrices" else LIGHT)
        kept = snap(s)
        for dst, src in ((d, s), (s, d)):
            assert L.tr_scene_shadow_merge(dst._h, src._h) == _lib.TR_E_INVALID, word
            assert word.encode() in L.tr_last_error().lower(), L.tr_last_error()
        same(snap(s), kept, what=word)
    assert L.tr_scene_shadow_merge(d._h, d._h) == _lib.TR_E_INVALID and b"same scene" in L.tr_last_error()
    assert L.tr_scene_shadow_merge(d._h, None) == _lib.TR_E_INVALID and L.tr_scene_shadow_merge(None, d._h) == _lib.TR_E_INVALID
    # a one-pass scene in each of the split calls
    one = cases["one pass"]
    kept = snap(one)
    assert L.tr_scene_render_shadow_pass(one._h) == _lib.TR_E_INVALID and b"one pass" in L.tr_last_error()
    assert L.tr_scene_render_colour_pass(one._h) == _lib.TR_E_INVALID and b"one pass" in L.tr_last_error()
    same(snap(one), kept)
    assert d.sync() == 0
    same(snap(d), before)
    # the same light again: the buffers merge
    drive(cases["matrices"])
    d.shadow_merge(cases["matrices"])
    assert d.sync() == 0
    for s in list(cases.values()) + [d]:
        s.close()


@pytest.mark.gpu
def test_ordering_src_rendered_again_right_after_the_merge(small_synthetic, other_synthetic):
    """No sync between the merge and src's next render under a new light: the merge must have read src's OLD buffer, and
    src's new frame must be complete afterwards."""
    W, Hh = 512, 256
    ref_d, ref_s = _pair(W, Hh, small_synthetic, other_synthetic)
    drive(ref_d), drive(ref_s)
    fd, fs = snap(ref_d), snap(ref_s)
    want = dict(fd, shadow=rule(fd["shadow"], fs["shadow"]))
    drive(ref_s, cam=1.2, light=0.1)
    new_src = snap(ref_s)
    assert not np.array_equal(bits(new_src["shadow"]), bits(fs["shadow"]))
    d, s = _pair(W, Hh, small_synthetic, other_synthetic)
    drive(d), drive(s)
    d.shadow_merge(s)
    drive(s, cam=1.2, light=0.1)      # overwrites what the merge reads: must run behind it
    s.flush()
    same(snap(d), want, what="dst:")
    same(snap(s), new_src, what="src:")
    for q in (ref_d, ref_s, d, s):
        q.close()


@pytest.mark.gpu
@pytest.mark.parametrize("pipe", TWO_PASS)
def test_ordering_renders_held_back_come_out_ahead_of_a_split_pass(small_synthetic, pipe):
    """tr_scene_render calls that auto-grouping holds back are submitted by a split call: the passes that follow without
    a clear land on top of the last of them, as the oracle's second render without a clear does."""
    import tiny_renderer_amd as T
    W, Hh = 208, 40
    at = np.array([[0.1, 0.0, 0.0, 0.9]], np.float32)
    s = scene(W, Hh, small_synthetic, pipe, at)
    assert s.frames_per_launch > 1, "nothing would be held back"
    drive(s, cam=0.9, light=0.2), drive(s, cam=0.1)     # two cleared frames, held back on the library's own stream
    split(s, cam=-0.5, clear=False)
    cpu = oracle_frame(W, Hh, T.apply_instances(small_synthetic[0], at), small_synthetic[1], pipe, cam=0.1, again=(-0.5, LIGHT))
    got = snap(s)
    got["win"] = None
    same(got, cpu)
    s.close()


@pytest.mark.gpu
def test_overflow_in_a_split_pass_is_reported_and_the_calls_again_succeed(small_synthetic):
    """bin_capacity=64 records: both passes want more.  They count as handed on, so the sync reports TR_E_BIN_OVERFLOW with
    the pools grown instead of replaying the scene's last render; the same calls again match the oracle."""
    import tiny_renderer_amd as T
    from tiny_renderer_amd import _lib
    L = T.load_library()
    W, Hh, pipe = 320, 256, "shadow"
    s = scene(W, Hh, small_synthetic, pipe, bin_capacity=64)
    split(s)
    assert L.tr_scene_sync(s._h) == _lib.TR_E_BIN_OVERFLOW
    assert b"handed on" in L.tr_last_error(), L.tr_last_error()
    split(s)
    assert L.tr_scene_sync(s._h) == 0, L.tr_last_error()
    got = snap(s)
    got["win"] = None
    same(got, oracle_frame(W, Hh, small_synthetic[0], small_synthetic[1], pipe))
    s.close()


@pytest.mark.gpu
def test_cli_shared_shadows_writes_the_python_sequence(african_head, diablo, tmp_path):
    import tiny_renderer_amd as T
    from tiny_renderer_amd import cli
    head_dir, diablo_dir = H.asset_dir("african_head"), H.asset_dir("diablo")
    W, Hh = 256, 128
    off = [float(v) for v in _toward_light(0.9, 1.0)[0, :3]]
    common = ["-p", head_dir, "--width", str(W), "--height", str(Hh), "--camera-angle", str(CAM), "--light-angle", str(LIGHT),
              "--with", diablo_dir, "--with-offset", ",".join(repr(v) for v in off)]
    paths = [str(tmp_path / n) for n in ("shared.ppm", "plain.ppm")]
    assert cli.main(common + ["-s", "shadow", "--with-shader", "occlusion", "--shared-shadows", "--out", paths[0]]) == 0
    assert cli.main(common + ["-s", "shadow", "--with-shader", "occlusion", "--out", paths[1]]) == 0
    hd = b"P6\n%d %d\n255\n" % (W, Hh)
    shared, plain = (np.frombuffer(open(p, "rb").read()[len(hd):], np.uint8).reshape(Hh, W, 3) for p in paths)
    a = T.Scene(W, Hh, *T.load_assets(head_dir), "shadow")
    b = T.Scene(W, Hh, *T.load_assets(diablo_dir), "occlusion", store_depth=True, instances=np.array([off + [1.0]], np.float32))
    _sequence(a, b, 0)
    assert np.array_equal(shared, a.get_frame_buffer())
    assert not np.array_equal(shared, plain), "the second model throws no shadow on the first"
    a.close(), b.close()
    # refused unless both sides have a shadow buffer, and without --with
    for bad in (["-s", "shadow", "--with-shader", "phong"], ["-s", "phong", "--with-shader", "shadow"], ["-s", "phong"]):
        with pytest.raises(SystemExit):
            cli.main(common + bad + ["--shared-shadows"])
    with pytest.raises(SystemExit):
        cli.main(["-p", head_dir, "-s", "shadow", "--shared-shadows"])
