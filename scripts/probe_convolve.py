"""What a convolve costs: python scripts/probe_convolve.py W H [-p DIR] [-s pipeline] [--reps N]
A scene (default model: the procedural scene) renders one frame and filters it, out of place into device memory and in
place, through a 3 x 3 and a 9 x 9 general kernel and separable Gaussians of 5, 17 and 31 taps:
  * k_convolve alone and k_tile for scale (HIP events on the scene's stream through tr_scene_profile_*, median and range
    over the repetitions; the frame is rendered again before every repetition, so that every in-place call finds the
    same frame and flags);
  * a device-to-device copy of the frame (hipMemcpyAsync between two device buffers, HIP events) in the same run;
  * the yardstick: k_bloom, glow only at threshold 0, at radius 2, 8 and 15 against k_convolve on the same tent (taps
    [1 .. R + 1 .. 1] on both axes under a border of 0: the same taps on the same tiles, another rounding only);
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


def census(cflags, W, Hh, rx, ry, clamp_or_black):
    """Tiles by path of one k_convolve launch over a W x Hh frame with colour-clean flags cflags (y up)."""
    ty, tx = cflags.shape
    constant = 0
    for j in range(ty):
        for i in range(tx):
            if not cflags[max(j - 1, 0):min(j + 2, ty), max(i - 1, 0):min(i + 2, tx)].all():
                continue
            inside = 128 * i - rx >= 0 and 128 * i + 128 + rx <= W and 16 * j - ry >= 0 and 16 * j + 16 + ry <= Hh
            constant += 1 if clamp_or_black or inside else 0
    return {"tiles": ty * tx, "tiles_constant": constant, "tiles_staged": ty * tx - constant}


def stats(us):
    return {"us": round(float(np.median(us)), 2), "us_min_max": [round(min(us), 2), round(max(us), 2)]}


def timed(s, call, kernel, reps, warmup):
    """Median [min, max] microseconds of `kernel` and of k_tile over reps calls of call(), the frame rendered before each."""
    k_us, tile_us = [], []
    for i in range(warmup + reps):
        s.profile_enable(True)
        drive(s)
        s.sync()
        call()
        s.sync()
        prof = s.profile_read()
        s.profile_enable(False)
        if i >= warmup:
            k_us.append(prof[kernel]["total_ms"] * 1e3)
            tile_us.append(prof["k_tile"]["total_ms"] * 1e3)
    return stats(k_us), stats(tile_us)


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
    out = {"width": W, "height": Hh, "pipeline": a.pipeline, "reps": a.reps, "frame_copy_d2d": time_copy(W * Hh * 3, a.reps, a.warmup),
           "cases": [], "yardstick": []}
    rng = np.random.default_rng(0)
    kernels = [("general 3x3", T.convolve_params(T.kernel_emboss()[0], bias=128, edge="clamp"), 1, 1),
               ("general 9x9", T.convolve_params(rng.integers(-300, 301, (9, 9)).astype(np.int32), shift=11, bias=128, edge="clamp"), 4, 4)]
    for r in (2, 8, 15):
        k, shift = T.kernel_gaussian(r / 3.0, r)
        kernels.append(("separable %d taps" % (2 * r + 1), T.convolve_params(k, shift=shift, edge="clamp"), r, r))
    for label, p, rx, ry in kernels:
        case = {"kernel": label}
        case.update(census(cflags, W, Hh, rx, ry, True))
        for mode in ("out_of_place", "in_place"):
            k, tile = timed(s, lambda: s.convolve(p, None if mode == "in_place" else dev.value), "k_convolve", a.reps, a.warmup)
            case[mode] = {"k_convolve": k, "k_tile": tile}
        out["cases"].append(case)
    for R in (2, 8, 15):
        tent, shift = T.kernel_tent(R)
        if (R + 1) & R:   # (the tent's own taps, not the normalised ones: the divisor is no power of two, so the bytes differ)
            t = (R + 1 - np.abs(np.arange(-R, R + 1))).astype(np.int32)
            tent, shift = (t, t.copy()), int(round(4 * np.log2(R + 1)))
        pc = T.convolve_params(tent, shift=shift)
        pb = T.bloom_params(R, 0, 256, T.scene.BLOOM_GLOW_ONLY)
        kc, _ = timed(s, lambda: s.convolve(pc, dev.value), "k_convolve", a.reps, a.warmup)
        kb, _ = timed(s, lambda: s.bloom(pb, dev.value), "k_bloom", a.reps, a.warmup)
        out["yardstick"].append({"radius": R, "k_convolve": kc, "k_bloom": kb, "ratio": round(kc["us"] / kb["us"], 2)})
    s.close()
    HIP.hipFree(dev)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
