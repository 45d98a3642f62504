"""What bloom costs: python scripts/probe_bloom.py W H [-p DIR] [-s pipeline] [-r RADIUS ...] [-t THRESHOLD] [--reps N]
A scene (default model: the procedural scene) renders one frame and blooms it at every RADIUS (default 2 8 15), out of
place into device memory and in place; the threshold defaults to the 60 % quantile of the drawn pixels' largest channel:
  * k_bloom alone and k_tile for scale (HIP events on the scene's stream through tr_scene_profile_*, median and range
    over the repetitions; the frame is rendered again before every repetition, so that every in-place call finds the
    same frame and flags);
  * the whole call by a host clock around call + sync on a scene that is idle, both ways: their difference is what the
    two device-to-device copies of the in-place form cost;
  * a device-to-device copy of the frame (hipMemcpyAsync between two device buffers, HIP events) in the same run;
  * the tiles by path -- zeros on the flags alone, a copy (no staged pixel passes the key), blurred -- and the bytes
    k_bloom moves, a MODEL computed on the host from the frame's flags and the snapshot, not a counter: read -- 3 bytes
    per staged pixel of a tile whose colour flag is down (pieces of four pixels: the halo's columns round up to four),
    and the tile's own 3 bytes per pixel a second time where it is not written as zeros or glow alone; written -- the
    whole frame."""
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
HIP.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
HIP.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
HIP.hipFree.argtypes = [C.c_void_p]
HIP.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
HIP.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
HIP.hipEventSynchronize.argtypes = [C.c_void_p]
HIP.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
HIP.hipEventDestroy.argtypes = [C.c_void_p]


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


def census(fb, cflags, R, thr, glow_only):
    """Paths and bytes of one k_bloom launch over the frame fb (row 0 = top) with colour-clean flags cflags (y up), as the
    kernel decides them."""
    Hh, W, _ = fb.shape
    ty, tx = cflags.shape
    keyed = (fb.max(-1) > thr)[::-1]                       # y up
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
            staged_key = False
            for jj in range(j0, j1):
                for ii in range(i0, i1):
                    if cflags[jj, ii]:
                        continue
                    y0, y1 = max(ys[0], 16 * jj), min(ys[1], 16 * jj + 16)
                    x0, x1 = max(xs[0], 128 * ii), min(xs[1], 128 * ii + 128)
                    if y1 > y0 and x1 > x0:
                        read += (y1 - y0) * (x1 - x0) * 3
                        staged_key = staged_key or bool(keyed[y0:y1, x0:x1].any())
            if not staged_key:
                copies += 1
            if not glow_only and not cflags[j, i]:
                read += (min(16 * j + 16, Hh) - 16 * j) * (min(128 * i + 128, W) - 128 * i) * 3
    return {"tiles": ty * tx, "tiles_zeros_on_flags": zeros, "tiles_copy": copies, "tiles_blurred": ty * tx - zeros - copies,
            "bytes_read": read, "bytes_written": W * Hh * 3}


def time_copy(nbytes, reps, warmup):
    """Median [min, max] microseconds of a device-to-device copy of nbytes bytes."""
    a, b, e0, e1 = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert HIP.hipMalloc(C.byref(a), nbytes) == 0 and HIP.hipMalloc(C.byref(b), nbytes) == 0
    assert HIP.hipEventCreate(C.byref(e0)) == 0 and HIP.hipEventCreate(C.byref(e1)) == 0
    us = []
    for i in range(warmup + reps):
        HIP.hipEventRecord(e0, None)
        assert HIP.hipMemcpyAsync(b, a, nbytes, 3, None) == 0   # (3: device to device)
        HIP.hipEventRecord(e1, None)
        HIP.hipEventSynchronize(e1)
        ms = C.c_float()
        HIP.hipEventElapsedTime(C.byref(ms), e0, e1)
        if i >= warmup:
            us.append(ms.value * 1e3)
    HIP.hipEventDestroy(e0), HIP.hipEventDestroy(e1), HIP.hipFree(a), HIP.hipFree(b)
    return {"us": round(float(np.median(us)), 2), "us_min_max": [round(min(us), 2), round(max(us), 2)]}


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("width", type=int)
    ap.add_argument("height", type=int)
    ap.add_argument("-p", dest="path", default=None)
    ap.add_argument("-s", dest="pipeline", default="phong")
    ap.add_argument("-r", dest="radii", type=int, nargs="+", default=[2, 8, 15])
    ap.add_argument("-t", dest="threshold", type=int, default=None)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    W, Hh = a.width, a.height
    mesh, texs = T.load_assets(a.path) if a.path else T.synthetic_scene()
    s = T.Scene(W, Hh, mesh, texs, a.pipeline)
    drive(s)
    fb = s.get_frame_buffer()
    drive(s)
    cflags = colour_flags(s)
    m = fb.max(-1)
    thr = a.threshold if a.threshold is not None else int(np.quantile(m[m > 0], 0.6))
    dev = C.c_void_p()
    assert HIP.hipMalloc(C.byref(dev), W * Hh * 3) == 0
    out = {"width": W, "height": Hh, "pipeline": a.pipeline, "reps": a.reps, "threshold": thr, "frame_max": int(m.max()),
           "pixels_keyed": int((m > thr).sum()), "frame_copy_d2d": time_copy(W * Hh * 3, a.reps, a.warmup), "cases": []}
    for R in a.radii:
        p = T.bloom_params(R, threshold=thr, strength=256)
        case = {"radius": R}
        case.update(census(fb, cflags, R, thr, False))
        for mode in ("out_of_place", "in_place"):
            k_us, tile_us, call_us = [], [], []
            for i in range(a.warmup + a.reps):
                s.profile_enable(True)
                drive(s)
                s.sync()
                t0 = time.perf_counter()
                s.bloom(p, None if mode == "in_place" else dev.value)
                s.sync()
                dt = (time.perf_counter() - t0) * 1e6
                prof = s.profile_read()
                s.profile_enable(False)
                if i >= a.warmup:
                    k_us.append(prof["k_bloom"]["total_ms"] * 1e3)
                    tile_us.append(prof["k_tile"]["total_ms"] * 1e3)
                    call_us.append(dt)
            med = float(np.median(k_us))
            case[mode] = {"k_bloom_us": round(med, 2), "k_bloom_us_min_max": [round(min(k_us), 2), round(max(k_us), 2)],
                          "call_and_sync_us": round(float(np.median(call_us)), 2), "k_tile_us": round(float(np.median(tile_us)), 2),
                          "k_tile_us_min_max": [round(min(tile_us), 2), round(max(tile_us), 2)],
                          "GBps": round((case["bytes_read"] + case["bytes_written"]) / (med * 1e-6) / 1e9, 1)}
        case["copies_us_by_difference"] = round(case["in_place"]["call_and_sync_us"] - case["out_of_place"]["call_and_sync_us"], 2)
        out["cases"].append(case)
    s.close()
    HIP.hipFree(dev)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
