"""What tests/test_warp_consumers_host.py (CPU) and tests/test_warp_consumers.py (GPU) share: the sizes, placements, grids
and kernels of the stages that replace a frame's colour and colour flags in place (warp, convolve), the consumers that
follow them, and the chains of host rules that are the expectation.

An in-place warp leaves a frame's two sets of per-tile fast-clear flags disagreeing in both directions:
  state A: colour flag UP over drawn depth (the colour moved out of a tile the model was drawn in; k_warp stored zeros
           and raised the flag, z memory still holds the drawn depth and its flag is down);
  state B: colour flag DOWN and colour in a tile nothing was drawn in (the z flag is up).
The rules themselves are not restated here: every expectation is a chain of the library's host rules, each of which its
own file pins against numpy.  What this file adds is the footprint bound of k_warp restated in numpy from the text of
tr_warp.h / k_warp ([min >> 8, (max >> 8) + 1] per axis over a tile's nodes), so that the CPU file can show that the
`shift` grid reaches state A, and the masks of the render-without-a-clear case."""
import numpy as np

from tests import convolve_cases as CC
from tests import dense_cases as DC
from tests import test_composite as TC
from tests import test_depth_of_field as TD
from tests import test_stage_entry_points as TS
from tests import warp_cases as WC

bits, tiles_any = TC.bits, TC.tiles_any
F32_MIN_BITS = TC.F32_MIN_BITS
CAM, LIGHT, PIPE = 0.3, 0.7, "phong"
AO = dict(radius=8, rings=2)
MIDDLE, NARROW, POSED = (384, 48), (200, 40), (208, 64)
# 384 x 48 is 3 x 3 whole tiles: tests/test_composite.py's DST_AT draws in the left and the middle tile column, over all
# three tile rows, and leaves the right column alone, so that a shift by two tile columns moves the colour out of the
# left column (state A) and into the right one (state B).  200 x 40: tests/test_depth_of_field.py's place for 208 x 40,
# over the corner of the partial tile column and the partial top tile row.  208 x 64: DST_AT, for the posed scenes.
# A whole-tile shift of one model moves ALL its colour off its own depth, and k_ao and a k_dof whose background stays
# sharp would then have nothing to do.  So each of the two sizes has a second, small instance (LANDING) where the
# shifted colour lands: inside one tile (the right one of the middle tile row at 384 x 48, the left one of the middle
# tile row at 200 x 40), so that colour lies over drawn depth there and a tile next to it stays undrawn and receives
# colour (state B: the top right tile at 384 x 48, into which rotate7 turns the instance's own colour as well).
LANDING = {MIDDLE: (1.05, 0.2, 0.0, 0.25), NARROW: (-0.95, 0.0, 0.0, 0.2)}
PLACE = {MIDDLE: np.concatenate([TC.DST_AT, np.array([LANDING[MIDDLE]], np.float32)]),
         NARROW: np.concatenate([TD.PLACE[(208, 40)], np.array([LANDING[NARROW]], np.float32)]), POSED: TC.DST_AT}
# the other scene of the composite cases: over the left tile columns, in front of and behind parts of the model
OTHER_AT = {MIDDLE: np.array([[-0.55, 0.1, 0.2, 0.5]], np.float32), NARROW: TC.SRC_AT}
# `shift`: the picture moves by (kx tile columns to the right, ky tile rows up): output (X, Y) shows source
# (X - 128 kx, Y + 16 ky), in buffer rows (row 0 = top).  200 x 40: the model stands in the upper right corner and moves
# left and down, part of it out of the frame.
DENSE = (256, 48)                                   # of DC.SIZES: the caller's buffer filled with noise
SHIFT = {MIDDLE: (2, 1), NARROW: (-1, -1), POSED: (1, 1), DENSE: (1, 1)}
OTHER_LIGHT = 0.2
ORDER_PAIRS = (("shift", "gaussian31"), ("rotate7", "emboss"))      # (warp, convolve), in place in either order
# the camera of the render without a clear on top: chosen with the oracle so that it wins many pixels and loses many
TOP_CAM = {MIDDLE: -1.0, NARROW: 2.0}
ON_TOP_STAGES = ("shift", "gaussian31", "unsharp")
# the posed group: rotate7 keeps the colour over the model's depth, so that another pose's depth would show in the blur
POSED_KIND, POSED_BACK, POSED_STAGE = "skin", 2, "rotate7"
assert DENSE in DC.SIZES


def shift_grid(W, Hh):
    kx, ky = SHIFT[(W, Hh)]
    return WC.nodes(lambda X, Y: (X - 128.0 * kx, Y + 16.0 * ky), W, Hh)


def grid(name, W, Hh):
    return shift_grid(W, Hh) if name.startswith("shift") else WC.grids(W, Hh, W, Hh)[name]


# name: (kind, grid or kernel, edge, border)
STAGES = {
    "shift": ("warp", "shift", "border", (0, 0, 0)),
    "rotate7": ("warp", "rotate7", "border", (0, 0, 0)),
    "shift_paper": ("warp", "shift", "border", WC.PAPER),
    "gaussian31": ("convolve", "gaussian31", "border", (0, 0, 0)),
    "emboss": ("convolve", "emboss", "border", CC.PAPER),
    "unsharp": ("convolve", "unsharp", "clamp", (0, 0, 0)),
}
_KERNELS = {}


def kernel(name):
    if not _KERNELS:
        _KERNELS.update(CC.everything())
    return _KERNELS[name]


def stage_params(name, W, Hh):
    import tiny_renderer_amd as T
    kind, what, edge, border = STAGES[name]
    if kind == "warp":
        return T.warp_params(edge, border)
    return CC.params(kernel(what), edge, border)


def stage_host(name, fb):
    """The stage's host rule over a frame's colour (row 0 = top)."""
    import tiny_renderer_amd as T
    Hh, W = fb.shape[:2]
    kind, what, edge, border = STAGES[name]
    if kind == "warp":
        return T.warp_host(fb, grid(what, W, Hh), W, Hh, stage_params(name, W, Hh))
    return T.convolve_host(fb, stage_params(name, W, Hh))


def stage_run(s, name):
    """The stage in place on the device."""
    kind, what, edge, border = STAGES[name]
    p = stage_params(name, s.width, s.height)
    if kind == "warp":
        s.set_warp(grid(what, s.width, s.height), s.width, s.height)
        assert s.warp(p) is None
    else:
        assert s.convolve(p) is None


def drawn(f):
    return bits(f["z"]) != F32_MIN_BITS


def lit(fb):
    """[tiles_y, tiles_x], y up: does the tile hold a non-zero colour byte (fb row 0 = top)?"""
    return tiles_any(fb[::-1].any(-1))


# ----------------------------------------------------------------------------------------------------------------------
# The two states, on a snapshot {"fb", "z"} from before the stage and the colour after it
# ----------------------------------------------------------------------------------------------------------------------

def state_a(f, staged, flags=None):
    """Tiles with a drawn pixel whose colour is all zeros afterwards (and, with the device's flags, whose flag is up)."""
    t = tiles_any(drawn(f)) & ~lit(staged)
    return t if flags is None else t & flags


def state_b(f, staged, flags=None):
    """Tiles without a drawn pixel that hold colour afterwards (and, with the device's flags, whose flag is down)."""
    t = ~tiles_any(drawn(f)) & lit(staged)
    return t if flags is None else t & ~flags


def tile_pixels(t, Hh, W, y_up=True):
    """[Hh, W] bool of the pixels of the tiles set in t ([tiles_y, tiles_x], row 0 = bottom); y_up False: row 0 = top."""
    m = np.zeros((Hh, W), bool)
    for ty, tx in zip(*np.nonzero(t)):
        m[ty * 16:ty * 16 + 16, tx * 128:tx * 128 + 128] = True
    return m if y_up else m[::-1]


def footprint_tiles(g, W, Hh, ty, tx):
    """k_warp's footprint of output tile (ty, tx) (y up; the height a multiple of 16) from the words of tr_warp.h: the
    tile's texels lie in [min >> 8, (max >> 8) + 1] per axis over the tile's nodes.  Returns (outside, [tiles_y, tiles_x]
    bool of the source tiles under the footprint clamped to the image)."""
    assert Hh % 16 == 0
    nty, ntx = Hh // 16, (W + 127) // 128
    by = nty - 1 - ty                                   # the workgroup's row: buffer rows 16 by onwards
    n_cx = (min(128, W - 128 * tx) + 15) // 16
    n = np.asarray(g, np.int64)[by:by + 2, 8 * tx:8 * tx + n_cx + 1]
    fx0, fx1, fy0, fy1 = int(n[..., 0].min()) >> 8, (int(n[..., 0].max()) >> 8) + 1, int(n[..., 1].min()) >> 8, (int(n[..., 1].max()) >> 8) + 1
    outside = fx1 < 0 or fx0 >= W or fy1 < 0 or fy0 >= Hh
    cx0, cx1, cy0, cy1 = (min(max(v, 0), m - 1) for v, m in ((fx0, W), (fx1, W), (fy0, Hh), (fy1, Hh)))
    under = np.zeros((nty, ntx), bool)
    under[(Hh - 1 - cy1) // 16:(Hh - 1 - cy0) // 16 + 1, cx0 // 128:cx1 // 128 + 1] = True
    return outside, under


def state_a_by_the_footprint(f, staged, name="shift"):
    """The state-A tiles k_warp must flag by its own rule: drawn z, output all zeros, and the footprint outside the image
    (under the black border) or on undrawn source tiles only.  (Undrawn by the oracle's pixels: a tile the scene flags
    clean has none.)"""
    Hh, W = f["z"].shape
    drawn_tiles = tiles_any(drawn(f))
    out = np.zeros_like(drawn_tiles)
    g = grid(STAGES[name][1], W, Hh)
    for ty, tx in zip(*np.nonzero(state_a(f, staged))):
        outside, under = footprint_tiles(g, W, Hh, ty, tx)
        out[ty, tx] = outside or not (under & drawn_tiles).any()
    return out


# ----------------------------------------------------------------------------------------------------------------------
# Consumers: name -> (the host rule over {"fb": the staged colour, "z": the z of before the stage}, the call on a scene)
# ----------------------------------------------------------------------------------------------------------------------

def outline_kw(only):
    sets = DC.outline_sets()
    kw = [k for k in sets if k["radius"] == 3 and bool(k.get("only")) == only and "crease" not in k][0]
    assert not only or tuple(kw["paper"]) != (0, 0, 0)
    return kw


def luts(W):
    """A table whose entry 0 is black and one whose entry 0 is not."""
    return {"grade_black": TS.random_lut(17, 17 + W, c0=(0, 0, 0)), "grade_tint": TS.random_lut(17, 18 + W, c0=(9, 0, 200))}


def zrange(f):
    z = f["z"][drawn(f)]
    return dict(z_lo=float(z.min()), z_scale=float(np.float32(200.0) / (z.max() - z.min())))


DEPTH_CONSUMERS = ("ao", "ao_grey", "dof0", "dof2", "outline", "outline_only", "stats_depth")
COLOUR_CONSUMERS = ("bloom", "grade_black", "grade_tint", "aa", "stats", "yuv")
# TR_OUTLINE_ONLY draws ink over paper from z alone: by its rule it reads no colour, so its expectation cannot tell the
# staged frame from the unstaged one.  It is here for what k_outline does with the colour FLAG (store_all = clean).
COLOUR_BLIND = ("outline_only",)


def consumer(name, f0):
    """(host(f) -> the expected frame or record, run(s) -> None or the getter's result) of consumer `name`; f0: the
    snapshot of before the stage, from which parameters that depend on the scene's depth are taken."""
    import tiny_renderer_amd as T
    from tests import test_bloom as TB
    W = f0["fb"].shape[1]
    if name in ("ao", "ao_grey"):
        kw = dict(AO, grey=name == "ao_grey")
        return (lambda f: T.ambient_occlusion_host(f["z"], f["fb"], **kw)), (lambda s: s.ambient_occlusion(**kw))
    if name in ("dof0", "dof2"):
        p = TD.params_for(f0, 3, bg=int(name[3]))
        return (lambda f: T.depth_of_field_host(f["z"], f["fb"], p)), (lambda s: s.depth_of_field(p))
    if name in ("outline", "outline_only"):
        p = T.outline_params(**outline_kw(name == "outline_only"))
        return (lambda f: T.outline_host(f["z"], f["fb"], p)), (lambda s: s.outline(p))
    if name == "stats_depth":
        zkw = zrange(f0)
        return (lambda f: T.frame_stats_host(f["fb"], f["z"], depth=True, **zkw)), (lambda s: s.get_frame_stats(depth=True, **zkw))
    if name == "stats":
        return (lambda f: T.frame_stats_host(f["fb"])), (lambda s: s.get_frame_stats())
    if name == "bloom":
        p = TB.P(15, 0, 256, 0)
        return (lambda f: T.bloom_host(f["fb"], p)), (lambda s: s.bloom(p))
    if name in ("grade_black", "grade_tint"):
        lut = luts(W)[name]
        return (lambda f: T.grade_host(f["fb"], lut)), (lambda s: (s.set_lut(lut), s.grade())[0])
    if name == "aa":
        p = T.aa_params()
        return (lambda f: T.aa_host(f["fb"], p)), (lambda s: s.antialias(p))
    if name == "yuv":
        return (lambda f: T.yuv_host(f["fb"], "i420")), (lambda s: s.to_yuv("i420"))
    raise ValueError(name)


def is_getter(name):
    """Consumers that return their result and leave the frame."""
    return name in ("stats_depth", "stats", "yuv")


# ----------------------------------------------------------------------------------------------------------------------
# A render without a clear on top of a staged frame
# ----------------------------------------------------------------------------------------------------------------------

def on_top(first, second, staged):
    """The frame after a second render without a clear on a frame whose colour a stage replaced: `first` and `second`
    are a twin's snapshots after its first render and after its second (no stage between them).  A pixel whose z bits
    changed was won by the second render and has the twin's colour; every other pixel keeps the staged colour."""
    won = bits(second["z"]) != bits(first["z"])
    return np.ascontiguousarray(np.where(won[::-1, :, None], second["fb"], staged)), won
