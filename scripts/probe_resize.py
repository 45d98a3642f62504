"""What the resize stage costs: python scripts/probe_resize.py W H [-p DIR] [-s pipeline] [--reps R]
A scene of W x H (default model: the procedural scene) renders one frame and resizes it, with both filters, to W/2 x H/2
(beside k_resolve by 2 of the same frame), 1920 x 1080, W/8 x H/8, W+1 x H-1; a scene of W/2 x H/2 resizes to W x H.
  * k_resize, k_resolve and k_tile from the same run (HIP events on the scene's stream through tr_scene_profile_*, median
    and range over the repetitions; the frame is rendered again before every repetition);
  * a device-to-device copy of the LARGER of the two images of a case (hipMemcpyAsync between two device buffers, HIP
    events) in the same run, and the case's time as a multiple of it;
  * the output tiles by path, a MODEL computed on the host from the frame's flags and the tables (tr_resize_taps), not a
    counter: stored as zeros on the flags (every source tile under the footprint flagged) or computed, and the shape
    of the kernel (output tile width x height, rows of horizontal sums)."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tiny_renderer_amd as T  # noqa: E402
from probe_outline import HIP, drive, time_copy, stat  # noqa: E402

SHAPES = ((64, 16, 24), (32, 8, 40), (32, 4, 48))   # kResizeShapes (csrc/tr_resize.h)


def flags_of(s):
    """The colour-clean flags of the current frame, [tiles_y, tiles_x], tile row 0 = bottom."""
    import torch
    s.sync()
    t = s.band_tiles()
    n = t.tiles_x * t.tiles_y

    class Flags:
        __cuda_array_interface__ = {"shape": (n,), "typestr": "<u4", "data": (int(t.clean_device), False), "version": 2}

    return torch.as_tensor(Flags(), device="cuda").cpu().numpy().reshape(t.tiles_y, t.tiles_x) != 0


def census(flags, W, Hh, w, h, filt):
    fx, cx, _ = T.resize_taps(filt, W, w)
    fy, cy, _ = T.resize_taps(filt, Hh, h)
    fx, cx, fy, cy = (v.astype(np.int64) for v in (fx, cx, fy, cy))
    for tw, th, rows in SHAPES:
        span = max(int(fy[min(a + th, h) - 1] + cy[min(a + th, h) - 1] - fy[a]) for a in range(0, h, th))
        if span <= rows:
            break
    zeros = total = 0
    for Y0 in range(0, h, th):
        Y1 = min(Y0 + th, h) - 1
        ty0, ty1 = (Hh - 1 - int(fy[Y1] + cy[Y1] - 1)) // 16, (Hh - 1 - int(fy[Y0])) // 16
        for X0 in range(0, w, tw):
            X1 = min(X0 + tw, w) - 1
            total += 1
            zeros += bool(flags[ty0:ty1 + 1, int(fx[X0]) // 128:int(fx[X1] + cx[X1] - 1) // 128 + 1].all())
    return {"shape": "%dx%d/%d" % (tw, th, rows), "tiles": total, "tiles_zeros_on_flags": zeros, "tiles_computed": total - zeros}


def run(s, W, Hh, sizes, reps, warmup, resolve_beside=None):
    drive(s)
    s.get_frame_buffer()
    flags = flags_of(s)
    cases, tile_us = [], []
    for w, h in sizes:
        nbytes = 3 * max(W * Hh, w * h)
        copy = time_copy(nbytes, reps, warmup)
        dev = C.c_void_p()
        assert HIP.hipMalloc(C.byref(dev), 3 * w * h) == 0
        case = {"from": [W, Hh], "to": [w, h], "copy_of_the_larger_image_d2d": copy}
        for filt in ("area", "bilinear"):
            us, res = [], []
            for i in range(warmup + reps):
                s.profile_enable(True)
                drive(s)
                s.resize_into(dev.value, w, h, filt)
                if resolve_beside == (w, h) and filt == "area":
                    s.resolve_into(2, dev.value)
                s.sync()
                prof = s.profile_read()
                s.profile_enable(False)
                if i >= warmup:
                    us.append(prof["k_resize"]["total_ms"] * 1e3)
                    tile_us.append(prof["k_tile"]["total_ms"] * 1e3)
                    if "k_resolve" in prof:
                        res.append(prof["k_resolve"]["total_ms"] * 1e3)
            case[filt] = dict(census(flags, W, Hh, w, h, filt), **stat(us))
            case[filt]["copies"] = round(case[filt]["us"] / copy["us"], 2)
            if res:
                case["k_resolve_by_2"] = stat(res)
        HIP.hipFree(dev)
        cases.append(case)
    return cases, stat(tile_us)


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
    out = {"width": W, "height": Hh, "pipeline": a.pipeline, "model": a.path or "procedural", "reps": a.reps}
    s = T.Scene(W, Hh, mesh, texs, a.pipeline)
    sizes = [(W // 2, Hh // 2), (min(1920, W), min(1080, Hh)), (W // 8, Hh // 8), (W + 1, Hh - 1)]
    out["cases"], out["k_tile"] = run(s, W, Hh, sizes, a.reps, a.warmup, resolve_beside=(W // 2, Hh // 2) if W % 2 == 0 and Hh % 2 == 0 else None)
    s.close()
    half = T.Scene(W // 2, Hh // 2, mesh, texs, a.pipeline)
    up, out["k_tile_half"] = run(half, W // 2, Hh // 2, [(W, Hh)], a.reps, a.warmup)
    half.close()
    out["cases"] += up
    print(json.dumps(out))


if __name__ == "__main__":
    main()
