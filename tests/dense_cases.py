"""What tests/test_dense_frames_host.py (CPU) and tests/test_dense_frames.py (GPU) share: the backdrops, the sizes, the
models' placement and the parameter sets of the frame stages on DENSE frames -- a caller's buffer filled with a backdrop
and drawn into without a clear, so that every pixel holds colour, the frame's borders are lit and the model's rim lies
against colour on both sides.

The rules themselves are not restated here: the numpy restatements of the suite (aa_cases.rule_np, outline_cases.rule_np,
test_bloom.rule, test_depth_of_field.rule, test_ambient_occlusion.rule, test_grade.rule, box) are the second opinion.
What this file adds beside the cases is the few sums the CPU test needs to show that a case reaches what it is for
(the horizontal tent sums of bloom, the weight sums of depth of field split by who contributes)."""
import numpy as np

from tests import aa_cases as AC
from tests import outline_cases as OC
from tests import test_composite as TC

F32_MIN_BITS = OC.F32_MIN_BITS
bits = OC.bits
BACKDROPS = ("noise", "white", "planted")
# OC.SIZES: the smallest frames that have both tile borders, a 4-pixel tile column, a 1-row tile row and an odd width
SIZES = OC.SIZES
# 3 x 3 tiles: a tile with all eight neighbours, for the stages that stage a halo of colour (bloom, depth of field)
MIDDLE = (384, 48)
SIZES_HALO = SIZES + (MIDDLE,)
CAM, LIGHT = OC.CAM, OC.LIGHT
PIPE = "phong"
GUARD = 64                                                # bytes of 0xAA on either side of a caller's buffer
GLOW = 1


def backdrop(kind, W, Hh):
    """uint8 [Hh, W, 3], row 0 = top."""
    if kind == "noise":
        return np.random.default_rng(W).integers(0, 256, (Hh, W, 3), dtype=np.uint8)
    if kind == "white":
        return np.full((Hh, W, 3), 255, np.uint8)
    if kind == "planted":
        from tests.test_aa_host import planted_image
        return planted_image(W, Hh, W * Hh)
    raise ValueError(kind)


def table(W, Hh):
    """Where the model stands (Scene(instances=...)): part of the backdrop stays, so that drawn and undrawn pixels lie
    beside each other."""
    return TC.DST_AT if (W, Hh) == MIDDLE else OC.table(W, Hh)


def paste(back, fb, z):
    """The dense frame the device produces, built on the host: the drawn pixels of a frame rendered on a cleared buffer
    (fb row 0 = top, z row 0 = bottom) over the backdrop."""
    drawn = (bits(z) != F32_MIN_BITS)[::-1]
    return np.ascontiguousarray(np.where(drawn[..., None], fb, back))


def distinct(fb):
    return len(np.unique(fb.reshape(-1, 3), axis=0))


# ----------------------------------------------------------------------------------------------------------------------
# Parameter sets, a short fixed list per stage
# ----------------------------------------------------------------------------------------------------------------------

def aa_sets():
    return AC.gpu_params() + [dict(contrast_min=0, contrast_rel=0)]


# (radius, threshold, strength, flags): the largest sums at radius 15; a mid threshold; the smallest radius at the top key
BLOOM_SETS = ((15, 0, 256, 0), (15, 0, 1024, GLOW), (8, 128, 256, 0), (1, 254, 1024, 0))
AO_SETS = (dict(radius=8, rings=2), dict(radius=8, rings=2, grey=True))
RESOLVE_FACTORS = (2, 4)


def dof_sets(f):
    """max_radius 8 with the focus on the model (test_depth_of_field.params_for) and the backdrop sharp, at 3 and at the
    largest circle; then the largest background with a scale that takes nearly all of the model to the largest circle
    too, so that model and backdrop spread over each other."""
    from tests import test_depth_of_field as TD
    out = [TD.params_for(f, 8, bg) for bg in (0, 3, 8)]
    p = out[-1]
    out.append(TD.P(float(p.focus), float(p.scale) * 6.0, R=8, bg=8))
    return out


def outline_sets():
    """OC.gpu_params() at radius 0 and 3: opacity 256 and 100, creases off and on, ONLY over PAPER."""
    out = [kw for kw in OC.gpu_params() if kw["radius"] in (0, 3)]
    assert len(out) == 5 and {kw.get("opacity", 256) for kw in out} == {256, 100}
    assert any(kw.get("only") and kw["paper"] == OC.PAPER for kw in out)
    return out


def grade_luts(W):
    from tests import test_grade as TG
    return [TG.random_lut(17, 17 + W), TG.random_lut(33, 33 + W)]


def resolve_factors(W, Hh):
    return [f for f in RESOLVE_FACTORS if W % f == 0 and Hh % f == 0]


# ----------------------------------------------------------------------------------------------------------------------
# Sums behind the rules, for the conditions of the CPU test
# ----------------------------------------------------------------------------------------------------------------------

def whole_tiles(W, Hh):
    """(x0, y0) in buffer coordinates (row 0 = top) of every whole 128 x 16 tile; tile rows count from the BOTTOM."""
    return [(128 * i, Hh - 16 * (j + 1)) for j in range(Hh // 16) for i in range(W // 128)]


def aa_survivors(rgb):
    """Pixels that pass step 1 of the anti-aliasing rule at the defaults, in every whole 128 x 16 tile: k_aa's list of
    them holds 2048 and is dealt out 256 at a time."""
    Hh, W, _ = rgb.shape
    passed = AC.rule_np(rgb)["passed"]
    return [int(passed[y0:y0 + 16, x0:x0 + 128].sum()) for x0, y0 in whole_tiles(W, Hh)]


def bloom_row_sums(rgb, R, thr):
    """The horizontal pass of the rule alone: [H, W, 3] int64, the tent sum over dx of the keyed frame."""
    F = np.asarray(rgb).astype(np.int64)
    Hh, W, _ = F.shape
    B = np.where((F.max(-1) > thr)[..., None], F, 0)
    pb = np.zeros((Hh, W + 2 * R, 3), np.int64)
    pb[:, R:R + W] = B
    out = np.zeros((Hh, W, 3), np.int64)
    for dx in range(-R, R + 1):
        out += (R + 1 - abs(dx)) * pb[:, R + dx:R + dx + W]
    return out


def dof_sums(z, rgb, p, who=None):
    """sw [H, W], sc [H, W, 3] and the number of taps [H, W] of the depth-of-field rule in z's orientation, int64; `who`
    ([H, W] bool, z's orientation) keeps the taps q with who[q] only."""
    from tests import test_depth_of_field as TD
    z = np.ascontiguousarray(z, np.float32)
    Hh, W = z.shape
    R = int(p.max_radius)
    coc = TD.coc_np(z, p.focus, p.scale, R, int(p.background_radius), p.range)
    w = np.array(TD.WT, np.int64)[coc]
    if who is not None:
        coc = np.where(who, coc, -1)
    pc = np.full((Hh + 2 * R, W + 2 * R), -1, np.int64)
    pc[R:R + Hh, R:R + W] = coc
    pw = np.zeros((Hh + 2 * R, W + 2 * R), np.int64)
    pw[R:R + Hh, R:R + W] = w
    pf = np.zeros((Hh + 2 * R, W + 2 * R, 3), np.int64)
    pf[R:R + Hh, R:R + W] = np.asarray(rgb)[::-1]
    sw, sc, taps = np.zeros((Hh, W), np.int64), np.zeros((Hh, W, 3), np.int64), np.zeros((Hh, W), np.int64)
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            sl = (slice(R + dy, R + dy + Hh), slice(R + dx, R + dx + W))
            ok = pc[sl] >= max(abs(dx), abs(dy))
            ww = np.where(ok, pw[sl], 0)
            sw += ww
            sc += ww[..., None] * pf[sl]
            taps += ok
    return sw, sc, taps
