"""What outlines cost: python scripts/probe_outline.py W H [-p DIR] [-s pipeline] [--reps R]
A scene (default model: the procedural scene) renders one frame and outlines it at radius 0 and 3, without and with
creases, out of place into device memory and in place:
  * k_outline alone, and k_tile and k_ao (radius 4, one ring) for scale, all timed in the same run (HIP events on the
    scene's stream through tr_scene_profile_*, median and range over the repetitions; the frame is rendered again before
    every repetition, so that every in-place call finds the same frame and flags);
  * a device-to-device copy of the frame (hipMemcpyAsync between two device buffers, HIP events) in the same run;
  * the tiles by path, a MODEL computed on the host from the frame's z, its flags and tr_outline_kinds, not a counter:
    left on flags (in place: no ink reaches them; all nine z flags of the neighbourhood up, or staged and found empty),
    copied (out of place, no ink: colour passed through or zeros stored) and inked."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tiny_renderer_amd as T  # noqa: E402

HIP = C.CDLL("libamdhip64.so")
HIP.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
HIP.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
HIP.hipFree.argtypes = [C.c_void_p]
HIP.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
HIP.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
HIP.hipEventSynchronize.argtypes = [C.c_void_p]
HIP.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
HIP.hipEventDestroy.argtypes = [C.c_void_p]
F32_MIN_BITS = np.uint32(0xFF7FFFFF)


def drive(s):
    s.clear()
    s.set_light_direction([0.5, 0.0, 0.8])
    s.set_camera([0.3, 0.0, 0.95], [0.0, 0.0, 0.0], [0.0, 1.0, 0.0])
    s.render()


def tiles_any(mask):
    Hh, W = mask.shape
    return np.array([[mask[j:j + 16, i:i + 128].any() for i in range(0, W, 128)] for j in range(0, Hh, 16)])


def census(z, params, radius):
    """Tiles by path for one launch over the depth z [H, W] (y up)."""
    drawn = z.view(np.uint32) != F32_MIN_BITS
    seed = T.outline_kinds(z, params) != 0
    Hh, W = z.shape
    pad = np.zeros((Hh + 2 * radius, W + 2 * radius), bool)
    pad[radius:radius + Hh, radius:radius + W] = seed
    inked = np.zeros((Hh, W), bool)
    for dy in range(2 * radius + 1):
        for dx in range(2 * radius + 1):
            inked |= pad[dy:dy + Hh, dx:dx + W]
    d, k = tiles_any(drawn), tiles_any(inked)
    near = np.zeros_like(d)   # a drawn tile in the 3 x 3 neighbourhood: the tile is staged
    p = np.pad(d, 1)
    for dy in range(3):
        for dx in range(3):
            near |= p[dy:dy + d.shape[0], dx:dx + d.shape[1]]
    return {"tiles": int(d.size), "tiles_inked": int(k.sum()), "tiles_staged_without_ink": int((near & ~k).sum()),
            "tiles_on_flags_alone": int((~near).sum()), "pixels_inked": int(inked.sum()), "pixels_seed": int(seed.sum())}


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


def stat(us):
    return {"us": round(float(np.median(us)), 2), "us_min_max": [round(min(us), 2), round(max(us), 2)]}


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("width", type=int)
    ap.add_argument("height", type=int)
    ap.add_argument("-p", dest="path", default=None)
    ap.add_argument("-s", dest="pipeline", default="phong")
    ap.add_argument("--depth", type=float, default=4.0)
    ap.add_argument("--crease", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    W, Hh = a.width, a.height
    mesh, texs = T.load_assets(a.path) if a.path else T.synthetic_scene()
    s = T.Scene(W, Hh, mesh, texs, a.pipeline, store_depth=True)
    drive(s)
    z = s.read_z_f32()
    dev = C.c_void_p()
    assert HIP.hipMalloc(C.byref(dev), W * Hh * 3) == 0
    out = {"width": W, "height": Hh, "pipeline": a.pipeline, "reps": a.reps, "depth_step": a.depth, "crease": a.crease,
           "frame_copy_d2d": time_copy(W * Hh * 3, a.reps, a.warmup), "cases": []}
    ao_us, tile_us = [], []
    for i in range(a.warmup + a.reps):
        s.profile_enable(True)
        drive(s)
        s.ambient_occlusion(radius=4, rings=1)
        s.sync()
        prof = s.profile_read()
        s.profile_enable(False)
        if i >= a.warmup:
            ao_us.append(prof["k_ao"]["total_ms"] * 1e3)
            tile_us.append(prof["k_tile"]["total_ms"] * 1e3)
    out["k_ao_radius4_ring1"], out["k_tile"] = stat(ao_us), stat(tile_us)
    for radius in (0, 3):
        for crease in (None, a.crease):
            p = T.outline_params(radius=radius, depth_step=a.depth, crease=crease)
            case = dict(census(z, p, radius), radius=radius, creases=crease is not None)
            for mode in ("out_of_place", "in_place"):
                us = []
                for i in range(a.warmup + a.reps):
                    s.profile_enable(True)
                    drive(s)
                    s.outline(p, None if mode == "in_place" else dev.value)
                    s.sync()
                    prof = s.profile_read()
                    s.profile_enable(False)
                    if i >= a.warmup:
                        us.append(prof["k_outline"]["total_ms"] * 1e3)
                case[mode] = stat(us)
            out["cases"].append(case)
    s.close()
    HIP.hipFree(dev)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
