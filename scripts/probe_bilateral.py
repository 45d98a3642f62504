"""What a bilateral filter costs: python scripts/probe_bilateral.py W H [-p DIR] [-s pipeline] [--reps N]
A scene (default model: the procedural scene) renders one frame and smooths it, out of place into device memory and in
place, through boxes of 3 x 3, 5 x 5, 9 x 9 and 15 x 15 under a step table (cutoff 16), guided by colour and by depth,
all clamped at the edge:
  * k_bilateral alone and k_tile for scale (HIP events on the scene's stream through tr_scene_profile_*: median, minimum
    and maximum over the repetitions; the frame is rendered again before every repetition, so that every in-place call
    finds the same frame and flags -- and every depth-guided call a depth left on the chip, which it makes real: that
    pass is k_tile_depth's time, not k_bilateral's);
  * a device-to-device copy of the frame (hipMemcpyAsync between two device buffers, HIP events) in the same run;
  * the yardsticks: k_convolve through a general 9 x 9 kernel and k_rank's median over the same four windows on the same
    frame, and the ratios of k_bilateral to the copy and to k_rank's median on the same window;
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
    ap.add_argument("--depth-scale", type=float, default=8.0)
    a = ap.parse_args()
    W, Hh = a.width, a.height
    mesh, texs = T.load_assets(a.path) if a.path else T.synthetic_scene()
    s = T.Scene(W, Hh, mesh, texs, a.pipeline)
    drive(s)
    cflags = colour_flags(s)
    dev = C.c_void_p()
    assert HIP.hipMalloc(C.byref(dev), W * Hh * 3) == 0
    copy = time_copy(W * Hh * 3, a.reps, a.warmup)
    out = {"width": W, "height": Hh, "pipeline": a.pipeline, "reps": a.reps, "frame_copy_d2d": copy, "k_rank_median": {}, "cases": []}
    rng = np.random.default_rng(0)
    p9 = T.convolve_params(rng.integers(-300, 301, (9, 9)).astype(np.int32), shift=11, bias=128, edge="clamp")
    k, tile = timed(s, lambda: s.convolve(p9, dev.value), "k_convolve", a.reps, a.warmup)
    out["k_convolve"] = {"kernel": "general 9x9", "out_of_place": {"k_convolve": k, "k_tile": tile}}
    sides = (3, 5, 9, 15)
    for n in sides:
        rp = T.rank_params(T.footprint_rect(n, n), "median", edge="clamp")
        k, tile = timed(s, lambda: s.rank(rp, dev.value), "k_rank", a.reps, a.warmup)
        out["k_rank_median"]["%dx%d" % (n, n)] = {"k_rank": k, "k_tile": tile}
    for n in sides:
        for guide in ("colour", "depth"):
            p = T.bilateral_params(T.spatial_box(n, n), T.range_step(16), guide=guide, depth_scale=a.depth_scale, edge="clamp")
            case = {"window": "%dx%d" % (n, n), "guide": guide, "taps": n * n}
            case.update(census(cflags, W, Hh, n // 2, n // 2, True))
            for mode in ("out_of_place", "in_place"):
                k, tile = timed(s, lambda: s.bilateral(p, None if mode == "in_place" else dev.value), "k_bilateral", a.reps, a.warmup)
                case[mode] = {"k_bilateral": k, "k_tile": tile}
            us = case["out_of_place"]["k_bilateral"]["us"]
            case["ratio_to_copy"] = round(us / copy["us"], 2)
            case["ratio_to_k_rank_median"] = round(us / out["k_rank_median"][case["window"]]["k_rank"]["us"], 2)
            case["ratio_to_k_convolve_9x9"] = round(us / out["k_convolve"]["out_of_place"]["k_convolve"]["us"], 2)
            out["cases"].append(case)
    s.close()
    HIP.hipFree(dev)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
