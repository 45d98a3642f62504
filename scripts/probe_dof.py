"""What depth of field costs: python scripts/probe_dof.py W H [-p DIR] [-s pipeline] [-r RADIUS ...] [--reps N]
A scene that stores its depth (default model: the procedural scene) renders one frame and blurs it at every RADIUS
(default 2 4 8), out of place into device memory and in place; focus and scale come from the frame's z quantiles, so
that the model holds sharp pixels and pixels at max_radius:
  * k_dof alone and k_tile for scale (HIP events on the scene's stream, median and range over the repetitions; the
    frame is rendered again before every repetition, so that every in-place call finds the same frame and flags);
  * the whole call by a host clock around call + sync on a scene that is idle, both ways: their difference is what the
    two device-to-device copies of the in-place form cost;
  * the share of tiles leaving at each early exit and the bytes k_dof moves, computed on the host from the frame's flags
    and circles: read -- 4 bytes of z per staged pixel of a tile whose z flag is down, 3 of colour where the colour flag
    is down (16-byte pieces: the halo's columns round up to four); written -- the whole frame."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tiny_renderer_amd as T  # noqa: E402

HIP = C.CDLL("libamdhip64.so")
HIP.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
HIP.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
HIP.hipFree.argtypes = [C.c_void_p]
F32_MIN_BITS = np.uint32(0xFF7FFFFF)


def drive(s):
    s.clear()
    s.set_light_direction([0.5, 0.0, 0.8])
    s.set_camera([0.3, 0.0, 0.95], [0.0, 0.0, 0.0], [0.0, 1.0, 0.0])
    s.render()


def colour_flags(s):
    s.sync()
    t = s.band_tiles()
    m = t.tiles_x * t.tiles_y
    words = np.zeros(m, np.uint32)
    assert HIP.hipMemcpy(words.ctypes.data, t.clean_device, 4 * m, 2) == 0   # (2: device to host)
    return words.reshape(t.tiles_y, t.tiles_x) != 0


def census(z, cflags, p):
    """Exits and bytes of one k_dof launch over the frame z (y up) with colour-clean flags cflags, as the kernel decides
    them: the z flags of a frame rendered after a clear are up exactly where no pixel is drawn."""
    Hh, W = z.shape
    R = p.max_radius
    ty, tx = cflags.shape
    drawn = z.view(np.uint32) != F32_MIN_BITS
    coc = T.dof_coc(p, z)
    zflags = np.zeros((ty, tx), bool)
    for j in range(ty):
        for i in range(tx):
            zflags[j, i] = not drawn[16 * j:16 * j + 16, 128 * i:128 * i + 128].any()
    halo = -(-R // 4) * 4
    zeros = copies = 0
    read = 0
    for j in range(ty):
        for i in range(tx):
            j0, j1, i0, i1 = max(j - 1, 0), min(j + 2, ty), max(i - 1, 0), min(i + 2, tx)
            if cflags[j0:j1, i0:i1].all():
                zeros += 1
                continue
            ys = (max(16 * j - R, 0), min(16 * j + 16 + R, Hh))
            xs = (max(128 * i - halo, 0), min(128 * i + 128 + halo, W))
            if not coc[ys[0]:ys[1], xs[0]:xs[1]].any():
                copies += 1
            for jj in range(j0, j1):
                for ii in range(i0, i1):
                    h = min(ys[1], 16 * jj + 16) - max(ys[0], 16 * jj)
                    w = min(xs[1], 128 * ii + 128) - max(xs[0], 128 * ii)
                    read += max(h, 0) * max(w, 0) * ((0 if zflags[jj, ii] else 4) + (0 if cflags[jj, ii] else 3))
    return {"tiles": ty * tx, "tiles_zeros_exit": zeros, "tiles_copy_exit": copies, "bytes_read": read, "bytes_written": W * Hh * 3}


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("width", type=int)
    ap.add_argument("height", type=int)
    ap.add_argument("-p", dest="path", default=None)
    ap.add_argument("-s", dest="pipeline", default="phong")
    ap.add_argument("-r", dest="radii", type=int, nargs="+", default=[2, 4, 8])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    W, Hh = a.width, a.height
    mesh, texs = T.load_assets(a.path) if a.path else T.synthetic_scene()
    s = T.Scene(W, Hh, mesh, texs, a.pipeline, store_depth=True)
    drive(s)
    z = s.read_z_f32()
    drive(s)
    cflags = colour_flags(s)
    zd = z[z.view(np.uint32) != F32_MIN_BITS]
    lo, hi = float(np.quantile(zd, 0.15)), float(np.quantile(zd, 0.95))
    dev = C.c_void_p()
    assert HIP.hipMalloc(C.byref(dev), W * Hh * 3) == 0
    out = {"width": W, "height": Hh, "pipeline": a.pipeline, "reps": a.reps, "focus": lo, "cases": []}
    for R in a.radii:
        p = T.dof_params(lo, (R + 1.5) / (hi - lo), max_radius=R, range=(hi - lo) * 0.02)
        case = {"max_radius": R, "scale": p.scale}
        case.update(census(z, cflags, p))
        for mode in ("out_of_place", "in_place"):
            k_us, tile_us, call_us = [], [], []
            for i in range(a.warmup + a.reps):
                s.profile_enable(True)
                drive(s)
                s.sync()
                t0 = time.perf_counter()
                s.depth_of_field(p, None if mode == "in_place" else dev.value)
                s.sync()
                dt = (time.perf_counter() - t0) * 1e6
                prof = s.profile_read()
                s.profile_enable(False)
                if i >= a.warmup:
                    k_us.append(prof["k_dof"]["total_ms"] * 1e3)
                    tile_us.append(prof["k_tile"]["total_ms"] * 1e3)
                    call_us.append(dt)
            med = float(np.median(k_us))
            case[mode] = {"k_dof_us": round(med, 2), "k_dof_us_min_max": [round(min(k_us), 2), round(max(k_us), 2)],
                          "call_and_sync_us": round(float(np.median(call_us)), 2), "k_tile_us": round(float(np.median(tile_us)), 2),
                          "GBps": round((case["bytes_read"] + case["bytes_written"]) / (med * 1e-6) / 1e9, 1)}
        case["copies_us_by_difference"] = round(case["in_place"]["call_and_sync_us"] - case["out_of_place"]["call_and_sync_us"], 2)
        out["cases"].append(case)
    s.close()
    HIP.hipFree(dev)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
