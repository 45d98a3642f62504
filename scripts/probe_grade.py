"""What colour grading costs: python scripts/probe_grade.py W H [-p DIR] [-s pipeline] [-n N ...] [--reps R]
A scene (default model: the procedural scene) renders one frame and grades it through tables of edge N (default 17 25
33: two LDS forms and the global form), a seeded random table and an identity table each, out of place into device
memory and in place:
  * k_grade alone and k_tile for scale (HIP events on the scene's stream through tr_scene_profile_*, median and range
    over the repetitions; the frame is rendered again before every repetition, so that every in-place call finds the
    same frame and flags);
  * a device-to-device copy of the frame (hipMemcpyAsync between two device buffers, HIP events) in the same run;
  * the tiles by path -- flagged (not read: left alone in place, stored as zeros out of place; the tables here have
    c0 = 0, the random one by construction) and graded -- and the bytes k_grade moves, a MODEL computed on the host from
    the frame's flags, not a counter: read -- 3 bytes a pixel of every tile whose flag is down; written -- as many in
    place, the whole frame out of place;
  * the launch geometry the library derives (CUs, LDS per CU as the runtime reports it, workgroups)."""
import argparse
import ctypes as C
import json
import os
import sys

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
HIP.hipDeviceGetAttribute.argtypes = [C.POINTER(C.c_int), C.c_int, C.c_int]
ATTR_CUS, ATTR_LDS_PER_CU = 63, 10002   # hipDeviceAttributeMultiprocessorCount, ...MaxSharedMemoryPerMultiprocessor


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


def census(W, Hh, cflags, in_place):
    """Paths and bytes of one k_grade launch with c0 = 0 over a W x Hh frame with colour-clean flags cflags."""
    ty, tx = cflags.shape
    px = 0
    for j, i in zip(*np.nonzero(~cflags)):
        px += (min(16 * j + 16, Hh) - 16 * j) * (min(128 * i + 128, W) - 128 * i)
    return {"tiles": int(ty * tx), "tiles_flagged": int(cflags.sum()), "tiles_graded": int((~cflags).sum()),
            "bytes_read": int(3 * px), "bytes_written": int(3 * px if in_place else 3 * W * Hh)}


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


def geometry(n, n_tiles):
    """The grid launch_grade derives for a table of edge n (tr_kernels.hip)."""
    cus, lds = C.c_int(), C.c_int()
    assert HIP.hipDeviceGetAttribute(C.byref(cus), ATTR_CUS, 0) == 0
    if HIP.hipDeviceGetAttribute(C.byref(lds), ATTR_LDS_PER_CU, 0) != 0 or lds.value < 65536:
        lds.value = 65536
    lds_bytes = (n ** 3 + 3) // 4 * 16 if n <= 25 else 0
    per_cu = min(8, lds.value // lds_bytes) if lds_bytes else 8
    return {"cus": cus.value, "lds_per_cu": lds.value, "lds_bytes": lds_bytes, "workgroups_per_cu": per_cu,
            "workgroups": min(cus.value * per_cu, n_tiles)}


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("width", type=int)
    ap.add_argument("height", type=int)
    ap.add_argument("-p", dest="path", default=None)
    ap.add_argument("-s", dest="pipeline", default="phong")
    ap.add_argument("-n", dest="edges", type=int, nargs="+", default=[17, 25, 33])
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
    out = {"width": W, "height": Hh, "pipeline": a.pipeline, "reps": a.reps,
           "frame_copy_d2d": time_copy(W * Hh * 3, a.reps, a.warmup), "cases": []}
    for n in a.edges:
        for kind in ("random", "identity"):
            if kind == "random":
                lut = np.random.default_rng(n).integers(0, 256, (n, n, n, 3), dtype=np.uint8)
                lut[0, 0, 0] = 0
            else:
                lut = T.lut_identity(n)
            s.set_lut(lut)
            case = {"n": n, "table": kind, "form": "lds" if n <= 25 else "global"}
            case.update(geometry(n, int(cflags.size)))
            for mode in ("out_of_place", "in_place"):
                k_us, tile_us = [], []
                for i in range(a.warmup + a.reps):
                    s.profile_enable(True)
                    drive(s)
                    s.grade(None if mode == "in_place" else dev.value)
                    s.sync()
                    prof = s.profile_read()
                    s.profile_enable(False)
                    if i >= a.warmup:
                        k_us.append(prof["k_grade"]["total_ms"] * 1e3)
                        tile_us.append(prof["k_tile"]["total_ms"] * 1e3)
                med = float(np.median(k_us))
                c = census(W, Hh, cflags, mode == "in_place")
                case[mode] = dict(c, k_grade_us=round(med, 2), k_grade_us_min_max=[round(min(k_us), 2), round(max(k_us), 2)],
                                  k_tile_us=round(float(np.median(tile_us)), 2),
                                  k_tile_us_min_max=[round(min(tile_us), 2), round(max(tile_us), 2)],
                                  GBps=round((c["bytes_read"] + c["bytes_written"]) / (med * 1e-6) / 1e9, 1))
            out["cases"].append(case)
    s.close()
    HIP.hipFree(dev)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
