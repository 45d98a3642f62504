"""What a rank filter costs: python scripts/probe_rank.py W H [-p DIR] [-s pipeline] [--reps N]
A scene (default model: the procedural scene) renders one frame and filters it, out of place into device memory and in
place, through a 3 x 3 erode, median and despeckle, a 5 x 5 median, a disc-3 median and a 15 x 15 erode and median, all
clamped at the edge:
  * k_rank alone and k_tile for scale (HIP events on the scene's stream through tr_scene_profile_*: median, minimum and
    maximum over the repetitions; the frame is rendered again before every repetition, so that every in-place call finds
    the same frame and flags), with the form the launcher takes: extremes (no selection) or general (the bit search);
  * a device-to-device copy of the frame (hipMemcpyAsync between two device buffers, HIP events) in the same run;
  * the yardstick: k_convolve through a general 3 x 3 and a general 9 x 9 kernel on the same frame, and the ratios of
    k_rank to the copy and to k_convolve on the same window (3 x 3 against 3 x 3; the larger ones against 9 x 9);
  * the tiles by path -- the constant without a load, staged -- a MODEL computed on the host from the frame's flags by
    the kernel's own rule, not a counter."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tiny_renderer_amd as T  # noqa: E402
from probe_bloom import HIP, drive, colour_flags, time_copy  # noqa: E402
from probe_convolve import census, timed  # noqa: E402


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
    s = T.Scene(W, Hh, mesh, texs, a.pipeline)
    drive(s)
    cflags = colour_flags(s)
    dev = C.c_void_p()
    assert HIP.hipMalloc(C.byref(dev), W * Hh * 3) == 0
    copy = time_copy(W * Hh * 3, a.reps, a.warmup)
    out = {"width": W, "height": Hh, "pipeline": a.pipeline, "reps": a.reps, "frame_copy_d2d": copy, "k_convolve": [], "cases": []}
    rng = np.random.default_rng(0)
    conv = {}
    for label, p, r in (("general 3x3", T.convolve_params(T.kernel_emboss()[0], bias=128, edge="clamp"), 1),
                        ("general 9x9", T.convolve_params(rng.integers(-300, 301, (9, 9)).astype(np.int32), shift=11, bias=128, edge="clamp"), 4)):
        k, tile = timed(s, lambda: s.convolve(p, dev.value), "k_convolve", a.reps, a.warmup)
        conv[r] = k["us"]
        out["k_convolve"].append({"kernel": label, "out_of_place": {"k_convolve": k, "k_tile": tile}})
    sq3, sq5, d3, sq15 = T.footprint_rect(3, 3), T.footprint_rect(5, 5), T.footprint_disc(3), T.footprint_rect(15, 15)
    filters = [("3x3 erode", T.rank_params(sq3, "min", edge="clamp"), 1, "extremes"),
               ("3x3 median", T.rank_params(sq3, "median", edge="clamp"), 1, "general"),
               ("3x3 despeckle", T.rank_params(sq3, 1, 7, op="clamp_centre", edge="clamp"), 1, "general, two searches"),
               ("5x5 median", T.rank_params(sq5, "median", edge="clamp"), 2, "general"),
               ("disc-3 median", T.rank_params(d3, "median", edge="clamp"), 3, "general"),
               ("15x15 erode", T.rank_params(sq15, "min", edge="clamp"), 7, "extremes"),
               ("15x15 median", T.rank_params(sq15, "median", edge="clamp"), 7, "general")]
    for label, p, r, form in filters:
        case = {"filter": label, "form": form, "taps": int(sum(bin(v).count("1") for v in p.rows))}
        case.update(census(cflags, W, Hh, r, r, True))
        for mode in ("out_of_place", "in_place"):
            k, tile = timed(s, lambda: s.rank(p, None if mode == "in_place" else dev.value), "k_rank", a.reps, a.warmup)
            case[mode] = {"k_rank": k, "k_tile": tile}
        us = case["out_of_place"]["k_rank"]["us"]
        case["ratio_to_copy"] = round(us / copy["us"], 2)
        case["ratio_to_k_convolve"] = {"window": "3x3" if r == 1 else "9x9", "ratio": round(us / conv[1 if r == 1 else 4], 2)}
        out["cases"].append(case)
    s.close()
    HIP.hipFree(dev)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
