"""What tests/test_frame_extremes_host.py (CPU) and tests/test_frame_extremes.py (GPU) share: the frame sizes at the two
ends of what tr_scene_create accepts (1 x 1 .. 32768 x 32768) with the reason for each, the models that draw on them, and
the parameter sets of every frame stage there.

Every frame is dense as in tests/dense_cases.py: a backdrop of noise in a caller's guarded buffer, drawn into without a
clear.  The rules are not restated: the suite's numpy restatements are the second opinion (one addition: the resize rule
evaluated tap by tap from resize_cases.tables_np, because the dense weight matrix of a 32768-wide axis is gigabytes; the
CPU test pins it to resize_cases.resize_np on the small frames)."""
import numpy as np

from tests import dense_cases as DC
from tests import outline_cases as OC
from tests import resize_cases as RC
from tests import warp_cases as WC
from tests import yuv_cases as YC

bits, F32_MIN_BITS = DC.bits, DC.F32_MIN_BITS
KIND = "noise"
PIPE = DC.PIPE
CAM, LIGHT = DC.CAM, DC.LIGHT

# (W, H): why the size is here
REASON = {
    (1, 1): "smaller than every radius in both directions: one pixel",
    (3, 2): "smaller than every radius in both directions: no 4-pixel unit, an odd width",
    (7, 5): "smaller than every radius in both directions: one whole unit and a partial one",
    (4, 16): "one 4-pixel unit a row: the wide store forms on a frame that is all border, one whole tile row",
    (8, 8): "one 8-pixel unit a row: the wide store forms on a frame that is all border",
    (5, 40): "narrower than every halo, three tile rows",
    (40, 3): "lower than every radius",
    (127, 15): "one short of a tile on both sides",
    (300, 1): "one row: three tile columns of one pixel row",
    (1, 70): "one column: five tile rows",
    (32768, 17): "256 tile columns, a 1-row tile row, x up to 32767 in every 16-bit field",
    (20, 32768): "2048 tile rows",
    (8200, 16): "the first width past the stages' own 8192",
}
SMALL = ((1, 1), (3, 2), (7, 5), (4, 16), (8, 8), (5, 40), (40, 3), (127, 15), (300, 1), (1, 70))
LONG = ((32768, 17), (20, 32768), (8200, 16))
SIZES = SMALL + LONG
assert set(SIZES) == set(REASON)
# resolve needs sides its factor divides: 32768 x 17 has none, so 32768 x 16 stands in for it there
RESOLVE_LONG = (32768, 16)
STAGE_MAX = 8192                                          # warp grids, resize outputs and YUV planes: 1..8192

# The model.  OC.table's spheres draw nothing on the small frames; these two overlap at different depths.
TWO = np.array([[-0.3, 0.0, 0.0, 1.1], [0.35, 0.1, 0.4, 0.8]], np.float32)
# The sizes at which the model could not be made to draw: no sphere and no flat mesh over the whole view leaves a
# pixel there (a frame one pixel wide or high has no pixel centre inside any polygon's box), so the depth stages run on
# an all-undrawn depth, which the CPU test asserts.
DRAWS_NOTHING = ((1, 1), (300, 1), (1, 70))
# 3 x 2 takes no pixel of any sphere either, but it does of a flat mesh: half a tilted square, so that one column stays
FLAT_AT = ((3, 2),)
# the sizes at which the depth stages are asserted to change the frame (outline at radius 3, AO and DOF at radius 8)
DEPTH_CHANGES = ((5, 40), (40, 3), (127, 15)) + LONG + (RESOLVE_LONG,)


def is_long(W, Hh):
    return max(W, Hh) > 4096


def flat_mesh():
    """A square in the plane z = 0.2 x that covers the left part of the view and faces the camera."""
    pos = np.array([[-4.0, -4.0, -0.8], [0.1, -4.0, 0.02], [0.1, 4.0, 0.02], [-4.0, 4.0, -0.8]], np.float32)
    tex = np.array([[0.1, 0.1, 0], [0.9, 0.1, 0], [0.9, 0.9, 0], [0.1, 0.9, 0]], np.float32)   # (1.0 is past the image's last texel)
    nrm = np.array([[0, 0, 1]], np.float32)
    idx = np.array([[a, a, 0, b, b, 0, c, c, 0] for a, b, c in ((0, 1, 2), (0, 2, 3))], np.uint32)
    return {"pos": pos, "tex": tex, "nrm": nrm, "idx": idx}


def model(ms, W, Hh):
    """(mesh, textures) of the scene at this size."""
    return (flat_mesh(), ms[1]) if (W, Hh) in FLAT_AT else ms


def table(W, Hh):
    """Scene(instances=...) at this size."""
    if (W, Hh) in FLAT_AT:
        return None
    return OC.AT_SMALL if is_long(W, Hh) else TWO


# two scenes (composite, shadow_merge): dst and src pass through each other
PAIR_SIZES = ((7, 5), (40, 3), (127, 15), (32768, 17))
ACCUMULATE_SIZES = ((7, 5), (32768, 17))
PAIR_LONG_SRC = np.array([[-0.35, -0.05, 0.1, 0.4]], np.float32)


def pair_tables(W, Hh):
    """(dst's table, src's table): src is another mesh, tests/test_composite.py's other_synthetic."""
    if is_long(W, Hh):
        return OC.AT_SMALL[:2], PAIR_LONG_SRC
    return TWO[:1], TWO[1:2]


def parity_light(W, Hh, pipe):
    """The light of the render-parity cases.  At 20 x 32768 the reference's second pass indexes its shadow buffer out of
    range under LIGHT (the oracle reports TRO_E_SHADOW_OOB, where the reference panics), so there is nothing to be equal
    to: 0.5 keeps every lookup inside."""
    return 0.5 if (W, Hh, pipe) == (20, 32768, "shadow") else LIGHT


def draws(W, Hh):
    return (W, Hh) not in DRAWS_NOTHING


def backdrop(W, Hh):
    return DC.backdrop(KIND, W, Hh)


# ----------------------------------------------------------------------------------------------------------------------
# Parameter sets: the lists of tests/dense_cases.py on the small frames, one set a stage on the long ones
# ----------------------------------------------------------------------------------------------------------------------

IN_STAGES = ("ao", "dof", "bloom", "grade", "outline", "aa", "convolve", "warp")
# the one set of a stage that runs in place, at odd addresses and on the long frames (an index into the small list)
ONE = {"aa": 0, "bloom": 0, "dof": 3, "grade": 1, "outline": 3, "ao": 0, "convolve": 0, "warp": 0}


def pick(stage, W, Hh, full):
    return [full[ONE[stage]]] if is_long(W, Hh) else list(full)


def aa_sets(W, Hh):
    return pick("aa", W, Hh, DC.aa_sets())


def bloom_sets(W, Hh):
    return pick("bloom", W, Hh, DC.BLOOM_SETS)


def ao_sets(W, Hh):
    return pick("ao", W, Hh, DC.AO_SETS)


def outline_sets(W, Hh):
    return pick("outline", W, Hh, DC.outline_sets())


def grade_luts(W, Hh):
    return pick("grade", W, Hh, DC.grade_luts(W))


def dof_sets(f, W, Hh):
    """tests/test_depth_of_field.py's params_for wants more than 50 drawn pixels, which the tiny frames do not have: here the
    focus is the farthest drawn depth and the scale takes the nearest one past max_radius 8, whatever the frame holds
    (an undrawn frame: focus 0, scale 1); the backdrop at circles 0, 3 and 8, and the largest background with six times
    the scale as in DC.dof_sets."""
    from tests import test_depth_of_field as TD
    z = f["z"][bits(f["z"]) != F32_MIN_BITS]
    lo, span = (float(z.min()), float(z.max() - z.min())) if z.size else (0.0, 0.0)
    scale = 9.5 / span if span > 0.0 else 1.0
    full = [TD.P(lo, scale, R=8, bg=bg) for bg in (0, 3, 8)] + [TD.P(lo, scale * 6.0, R=8, bg=8)]
    return pick("dof", W, Hh, full)


# (kernel of tests/convolve_cases.py, edge, border): the 31-tap gaussian first -- wider and higher than every small frame
CONVOLVE_SETS = (("gaussian31", "border", (250, 240, 200)), ("gaussian31", "clamp", (0, 0, 0)), ("box3", "border", (0, 0, 0)),
                 ("sobel_x_abs", "clamp", (0, 0, 0)), ("9x9_alternating", "border", (250, 240, 200)), ("3x7", "clamp", (0, 0, 0)),
                 ("31x1", "border", (250, 240, 200)), ("1x31", "clamp", (0, 0, 0)), ("unsharp", "border", (0, 0, 0)))


def convolve_sets(W, Hh):
    return pick("convolve", W, Hh, CONVOLVE_SETS)


def cap(v):
    return min(v, STAGE_MAX)


WARP_FLAG_TILES = 1024                                    # k_warp scans the flags of a footprint of at most so many tiles


def whole_grids(W, Hh):
    """Two grids of a 17 x 33 output whose first cell row spans the source from its first row and column on: "whole" from
    (0, 0), "whole-3" from (-3, -3).  Nodes end at 16384 source pixels, so on 20 x 32768 the first footprint is rows 0 to
    16385 or 0 to 16382: 1025 and 1024 tile rows of one tile column -- one past what a workgroup of k_warp scans the
    flags of, and exactly that (warp_footprints; the CPU test asserts both)."""
    return {"whole": WC.nodes(lambda X, Y: (X * (W / 16.0), Y * (Hh / 32.0)), 17, 33),
            "whole-3": WC.nodes(lambda X, Y: (X * (W / 16.0) - 3.0, Y * (Hh / 32.0) - 3.0), 17, 33)}


def warp_footprints(g, W, Hh, w, h):
    """The number of source tiles under the footprint of every workgroup of k_warp, by its description (a workgroup is
    128 x 16 output pixels; its nodes are two grid rows and up to nine columns; the footprint is the nodes' box in whole
    source pixels plus one, clamped to the image; tile rows count from the bottom): [rows, columns] of int."""
    g = np.asarray(g, np.int64)
    assert g.ndim == 3
    out = np.zeros(((h + 15) // 16, (w + 127) // 128), np.int64)
    for by in range(out.shape[0]):
        for bx in range(out.shape[1]):
            n_cx = (min(128, w - 128 * bx) + 15) // 16
            n = g[by:by + 2, 8 * bx:8 * bx + n_cx + 1]
            fx0, fx1, fy0, fy1 = n[..., 0].min() >> 8, (n[..., 0].max() >> 8) + 1, n[..., 1].min() >> 8, (n[..., 1].max() >> 8) + 1
            cx0, cx1, cy0, cy1 = (int(np.clip(v, 0, m - 1)) for v, m in ((fx0, W), (fx1, W), (fy0, Hh), (fy1, Hh)))
            out[by, bx] = (cx1 // 128 - cx0 // 128 + 1) * ((Hh - 1 - cy0) // 16 - (Hh - 1 - cy1) // 16 + 1)
    return out


def stretch_grid(W, Hh, w, h):
    """Four source pixels an output pixel along the long side: the builders clip the nodes at the coordinate limit."""
    return WC.nodes((lambda X, Y: (4.0 * X, Y)) if W >= Hh else (lambda X, Y: (X, 4.0 * Y)), w, h)


def warp_sets(W, Hh):
    """[(grid name, grid, w, h, edge, border)].  Small frames: every grid of tests/warp_cases.py at the frame's own size
    (the first one is the in-place case) under the three edges, and the rotation at 17 x 33.  Long frames: the rotation
    at the largest output a grid may have, and whole_grids.  On a source wider or higher than 16384 the nodes are
    clipped to the coordinate limit."""
    edges = (("border", WC.PAPER), ("clamp", (0, 0, 0)), ("border", (0, 0, 0)))
    if is_long(W, Hh):
        w, h = cap(W), cap(Hh)
        whole = whole_grids(W, Hh)
        return [("rotate7", WC.grids(W, Hh, w, h)["rotate7"], w, h) + edges[0], ("whole", whole["whole"], 17, 33) + edges[1],
                ("whole", whole["whole"], 17, 33) + edges[0], ("whole-3", whole["whole-3"], 17, 33) + edges[1]]
    out = []
    names = ("rotate7", "identity", "flip", "lens", "chromatic", "far")
    g = WC.grids(W, Hh, W, Hh)
    for name in names:
        for e in edges:
            out.append((name, g[name], W, Hh) + e)
    out.append(("rotate7", WC.grids(W, Hh, 17, 33)["rotate7"], 17, 33) + edges[0])
    return out


def td_params(stage, f, W, Hh):
    """The parameter sets of a stage that tests/test_dense_frames.py's `sets` knows, for its `params`."""
    return {"aa": aa_sets, "bloom": bloom_sets, "outline": outline_sets, "grade": grade_luts, "ao": ao_sets, "resolve": resolve_factors,
            "dof": lambda W, Hh: dof_sets(f, W, Hh)}[stage](W, Hh)


def resize_outputs(W, Hh):
    """ceil(N / 8); the same size (where a resize output may be that large: the largest it may be otherwise); + 1 and - 1."""
    up8 = RC.up8
    out = [(up8(W), up8(Hh)), (cap(W), cap(Hh)), (cap(W + 1), cap(Hh + 1)), (max(cap(W - 1), up8(W), 1), max(cap(Hh - 1), up8(Hh), 1))]
    seen = []
    for o in out:
        assert RC.allowed(W, o[0]) and RC.allowed(Hh, o[1])
        if o not in seen:
            seen.append(o)
    return seen


def resize_sets(W, Hh):
    return [(w, h, filt) for w, h in resize_outputs(W, Hh) for filt in RC.FILTERS]


def yuv_ok(W, Hh):
    return W <= STAGE_MAX and Hh <= STAGE_MAX


def yuv_sets(W, Hh):
    return [(layout, m, r) for layout in YC.LAYOUTS for m, r in YC.TABLES]


def resolve_factors(W, Hh):
    return [k for k in (2, 4, 8) if W % k == 0 and Hh % k == 0]


def window(W, Hh):
    """A window of the statistics that is not the frame (the frame itself where it has one pixel a side)."""
    return (W // 3, Hh // 4, max(W // 2, 1), max(Hh // 2, 1))


def z_range(f):
    z = f["z"][bits(f["z"]) != F32_MIN_BITS]
    if z.size == 0 or z.max() == z.min():
        return dict(z_lo=0.0, z_scale=1.0)
    return dict(z_lo=float(z.min()), z_scale=float(np.float32(200.0) / (z.max() - z.min())))


def must_change(stage, W, Hh):
    """Must at least one parameter set of the stage change the frame?  The colour stages everywhere but at 1 x 1 (where
    aa's single pixel has no neighbour to differ from and a rotation about the centre maps the one pixel to itself;
    bloom, grade and convolve change even that); the depth stages where the model leaves enough of both drawn and
    undrawn pixels."""
    if stage in ("outline", "ao", "dof"):
        return (W, Hh) in DEPTH_CHANGES
    return (W, Hh) != (1, 1) or stage in ("bloom", "grade", "convolve")


# ----------------------------------------------------------------------------------------------------------------------
# The resize rule tap by tap
# ----------------------------------------------------------------------------------------------------------------------

def _axis(a, filt, n, m, axis):
    """a [.., n, ..] int64 along `axis` -> [.., m, ..]: sum over the taps of RC.tables_np."""
    first, count, w = (v.astype(np.int64) for v in RC.tables_np(filt, n, m))
    a = np.moveaxis(a, axis, 0)
    out = np.zeros((m,) + a.shape[1:], np.int64)
    for k in range(RC.MAX_TAPS):
        live = k < count
        if not live.any():
            break
        src = a[np.minimum(first + k, n - 1)]
        out += np.where(live, w[:, k], 0).reshape((m,) + (1,) * (a.ndim - 1)) * src
    return np.moveaxis(out, 0, axis)


def resize_np(rgb, width, height, filt):
    f = RC.filter_id(filt) if isinstance(filt, str) else filt
    Hh, W, _ = rgb.shape
    inner = _axis(rgb.astype(np.int64), f, W, width, 1)
    assert inner.max() <= 255 * RC.ONE
    acc = _axis(inner, f, Hh, height, 0) + (1 << 23)
    assert acc.max() < 1 << 32
    return (acc >> 24).astype(np.uint8)
