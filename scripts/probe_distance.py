"""What a distance field costs: python scripts/probe_distance.py W H [-p DIR] [-s pipeline] [--reps N]
A scene (default model: the procedural scene) renders one frame; then, at R = 8, 64 and 255, under DRAWN seeds and under
KEY seeds (threshold 1: every pixel that is not black), median [min, max] over the repetitions of
  * the field alone -- k_dist_mask, k_dist_row and k_dist, which the profile times under the one name "k_dist" --, written
    into device memory;
  * the ramp (a glow table, KEEP_SEEDS, ADD) out of place and in place: the same three kernels, k_dist_apply, and their
    sum -- the whole call on the device (HIP events on the scene's stream through tr_scene_profile_*; the frame is
    rendered again before every repetition, so that every in-place call finds the same frame, depth and flags);
  * beside it, in the same run: a device-to-device copy of the frame, k_tile, k_ramp (a fog table), k_rank's 15 x 15
    dilate and k_outline at radius 3;
  * the waves of k_dist by path -- a wave is 64 pixels of a row: its mask word constant on a raised flag (k_dist_mask
    loaded nothing), FAR without a search (no summary byte within reach), searched -- and the mean taps per searched
    pixel.  A MODEL computed on the host from the frame, its flags and the field by the kernels' own rule, not a counter:
    a searched pixel with field value d2 reads its own byte and two bytes a row for ceil(sqrt(d2)) - 1 rows, R rows
    where it ends FAR (rows outside the frame are not subtracted)."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tiny_renderer_amd as T  # noqa: E402
from probe_bloom import HIP, drive, colour_flags, time_copy  # noqa: E402
from probe_convolve import stats  # noqa: E402

FIELD = ("k_dist",)   # (the profile's one name for k_dist_mask, k_dist_row and k_dist: three launches a call, their summed time)


def timed(s, call, kernels, reps, warmup):
    """Median [min, max] microseconds of each of `kernels`, of their sum and of k_tile over reps calls of call()."""
    us = {k: [] for k in kernels + ("sum", "k_tile")}
    for i in range(warmup + reps):
        s.profile_enable(True)
        drive(s)
        s.sync()
        call()
        s.sync()
        prof = s.profile_read()
        s.profile_enable(False)
        if i >= warmup:
            for k in kernels:
                us[k].append(prof[k]["total_ms"] * 1e3)
            us["sum"].append(sum(prof[k]["total_ms"] for k in kernels) * 1e3)
            us["k_tile"].append(prof["k_tile"]["total_ms"] * 1e3)
    return {k: stats(v) for k, v in us.items()}


def census(field, mask, flagged_rows, R):
    """Waves by path and the taps of the searched pixels: field and mask [H, W] row 0 = top, flagged_rows [H, words] bool."""
    Hh, W = field.shape
    wpr = (W + 63) // 64
    pad = np.full((Hh, wpr * 64), 256, np.int64)
    # the row distance of every pixel, by two running scans (the model needs the summary bytes only)
    idx = np.arange(W)
    for r in range(Hh):
        xs = np.flatnonzero(mask[r])
        if xs.size:
            k = np.searchsorted(xs, idx)
            left = np.where(k > 0, idx - xs[np.maximum(k - 1, 0)], 256)
            right = np.where(k < xs.size, xs[np.minimum(k, xs.size - 1)] - idx, 256)
            pad[r, :W] = np.minimum(np.minimum(left, right), 256)
    summary = pad.reshape(Hh, wpr, 64).min(axis=2)
    summary = np.where(summary == 256, 255, np.minimum(summary, 254))
    reach = np.zeros((Hh, wpr), bool)
    hit = summary <= min(R, 254)
    for r in range(Hh):
        reach[r] = hit[max(r - R, 0):r + R + 1].any(axis=0)
    searched_px = np.repeat(reach, 64, axis=1)[:, :W]
    d2 = field.astype(np.int64)
    rows = np.where(field == 0xFFFF, R, np.maximum(np.ceil(np.sqrt(d2)) - 1, 0))
    taps = 1 + 2 * rows[searched_px]
    return {"waves": int(Hh * wpr), "waves_constant_on_a_flag": int(flagged_rows.sum()), "waves_far_without_a_search": int((~reach).sum()),
            "waves_searched": int(reach.sum()), "mean_taps_per_searched_pixel": round(float(taps.mean()), 1) if taps.size else 0.0}


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("width", type=int)
    ap.add_argument("height", type=int)
    ap.add_argument("-p", dest="path", default=None)
    ap.add_argument("-s", dest="pipeline", default="phong")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    W, Hh = a.width, a.height
    mesh, texs = T.load_assets(a.path) if a.path else T.synthetic_scene()
    s = T.Scene(W, Hh, mesh, texs, a.pipeline, store_depth=True)
    drive(s)
    cflags = colour_flags(s)
    fb, z = s.get_frame_buffer(), s.read_z_f32()
    drawn = (z.view(np.uint32) != 0xFF7FFFFF)[::-1]
    zflag_tiles = np.array([[not drawn[::-1][16 * j:16 * j + 16, 128 * i:128 * i + 128].any() for i in range(cflags.shape[1])] for j in range(cflags.shape[0])])
    wpr = (W + 63) // 64

    def flagged_rows(tiles):
        rows = np.repeat(tiles, 16, axis=0)[:Hh][::-1]              # [H, tiles_x], row 0 = top
        return np.repeat(rows, 2, axis=1)[:, :wpr]

    dev_field, dev_frame = C.c_void_p(), C.c_void_p()
    assert HIP.hipMalloc(C.byref(dev_field), W * Hh * 2) == 0 and HIP.hipMalloc(C.byref(dev_frame), W * Hh * 3) == 0
    out = {"width": W, "height": Hh, "pipeline": a.pipeline, "reps": a.reps, "drawn_share": round(float(drawn.mean()), 4),
           "frame_copy_d2d": time_copy(W * Hh * 3, a.reps, a.warmup), "cases": []}
    for seed, thr, mask, tiles in (("drawn", 0, drawn, zflag_tiles), ("key", 1, fb.max(axis=2) >= 1, cflags)):
        for R in (8, 64, 255):
            case = {"seed": seed, "radius": R}
            field = s.get_distance(R, seed, thr)
            case.update(census(field, mask, flagged_rows(tiles), R))
            case["field"] = timed(s, lambda: s.distance(dev_field.value, R, seed, thr), FIELD, a.reps, a.warmup)
            table, step = T.ramp_glow((255, 200, 40), R)
            s.set_ramp(table)
            for mode in ("out_of_place", "in_place"):
                target = None if mode == "in_place" else dev_frame.value
                case["ramp_" + mode] = timed(s, lambda: s.distance_ramp(R, step, seed, thr, mode="add", keep_seeds=True, out=target),
                                             FIELD + ("k_dist_apply",), a.reps, a.warmup)
            out["cases"].append(case)
    # beside it
    s.set_ramp(T.ramp_fog((200, 210, 230), 256))
    zz = z[z.view(np.uint32) != 0xFF7FFFFF]
    z0, scale = T.ramp_span(float(zz.max()), float(zz.min()) if zz.min() != zz.max() else float(zz.max()) - 1.0, 256) if zz.size else T.ramp_span(1.0, 0.0, 256)
    beside = {}
    beside["k_ramp_in_place"] = timed(s, lambda: s.ramp(z0, scale), ("k_ramp",), a.reps, a.warmup)["k_ramp"]
    beside["k_rank_dilate_15x15"] = timed(s, lambda: s.rank(T.rank_params(T.footprint_rect(15, 15), "max"), out=dev_frame.value), ("k_rank",), a.reps, a.warmup)["k_rank"]
    beside["k_outline_radius_3"] = timed(s, lambda: s.outline(T.outline_params(radius=3), out=dev_frame.value), ("k_outline",), a.reps, a.warmup)
    out["k_tile"] = beside["k_outline_radius_3"]["k_tile"]
    beside["k_outline_radius_3"] = beside["k_outline_radius_3"]["k_outline"]
    out["beside"] = beside
    s.close()
    HIP.hipFree(dev_field), HIP.hipFree(dev_frame)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
