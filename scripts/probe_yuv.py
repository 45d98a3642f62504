"""What the YUV output stage costs: python scripts/probe_yuv.py W H [-p DIR] [-s pipeline] [--reps R]
A scene of W x H (default model: the procedural scene) renders one frame and converts it to I420, NV12 and I444
(bt709, limited range).
  * k_yuv per layout, k_grade out of place (a 17^3 identity table: the other pointwise stage over the same bytes) and
    k_tile from the same run (HIP events on the scene's stream through tr_scene_profile_*, median and range over the
    repetitions; the frame is rendered again before every repetition);
  * a device-to-device copy of the frame (hipMemcpyAsync between two device buffers, HIP events) in the same run, and
    each layout's time as a multiple of it -- the yardstick for 4:2:0, which moves 4.5 bytes a pixel where the copy
    moves 6;
  * the 128 x 16 tiles by path, a MODEL computed on the host from the frame's flags, not a counter: constant on the flag
    or converted, and the modelled bytes read (3 a pixel of an unflagged tile) and written (every plane byte);
  * wall clock: to_yuv_into a page-locked block plus sync against get_frame_buffer_async plus sync, the frame already
    rendered and waited for (time.perf_counter, median and range)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tiny_renderer_amd as T  # noqa: E402
from probe_outline import HIP, drive, time_copy, stat  # noqa: E402
from probe_resize import flags_of  # noqa: E402

LAYOUTS = ("i420", "nv12", "i444")


def census(flags, W, Hh):
    """Tiles by path and the modelled traffic of one conversion."""
    ty, tx = flags.shape
    read = 0
    for j in range(ty):
        rows = min(16, Hh - 16 * j)
        for i in range(tx):
            if not flags[j, i]:
                read += 3 * rows * min(128, W - 128 * i)
    return {"tiles": int(flags.size), "tiles_constant_on_flag": int(flags.sum()), "tiles_converted": int((~flags).sum()), "bytes_read": int(read)}


def wall(call, sync, reps, warmup):
    us = []
    for i in range(warmup + reps):
        t0 = time.perf_counter()
        call()
        sync()
        if i >= warmup:
            us.append((time.perf_counter() - t0) * 1e6)
    return stat(us)


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
    s.set_lut(T.lut_identity(17))
    drive(s)
    s.get_frame_buffer()
    flags = flags_of(s)
    out = {"width": W, "height": Hh, "pipeline": a.pipeline, "model": a.path or "procedural", "reps": a.reps}
    out["tiles"] = census(flags, W, Hh)
    out["copy_of_the_frame_d2d"] = copy = time_copy(3 * W * Hh, a.reps, a.warmup)
    dev = C.c_void_p()
    assert HIP.hipMalloc(C.byref(dev), 3 * W * Hh) == 0
    tile_us, grade_us = [], []
    for layout in LAYOUTS:
        us = []
        for i in range(a.warmup + a.reps):
            s.profile_enable(True)
            drive(s)
            s.to_yuv_into(dev.value, layout)
            if layout == "i420":
                s.grade(out=dev.value)
            s.sync()
            prof = s.profile_read()
            s.profile_enable(False)
            if i >= a.warmup:
                us.append(prof["k_yuv"]["total_ms"] * 1e3)
                tile_us.append(prof["k_tile"]["total_ms"] * 1e3)
                if "k_grade" in prof:
                    grade_us.append(prof["k_grade"]["total_ms"] * 1e3)
        out[layout] = dict(stat(us), bytes_written=T.yuv_bytes(W, Hh, layout))
        out[layout]["copies"] = round(out[layout]["us"] / copy["us"], 2)
    out["k_grade_out_of_place"], out["k_tile"] = stat(grade_us), stat(tile_us)
    HIP.hipFree(dev)
    # wall clock over the slow link, the frame rendered and waited for
    drive(s)
    s.sync()
    frame, planes = s.pinned_frame(), s.pinned_yuv("i420")
    out["wall_get_frame_buffer_async_plus_sync"] = wall(lambda: s.get_frame_buffer_async(frame), s.sync, a.reps, a.warmup)
    out["wall_to_yuv_i420_pinned_plus_sync"] = wall(lambda: s.to_yuv_into(planes, "i420"), s.sync, a.reps, a.warmup)
    out["wall_ratio"] = round(out["wall_to_yuv_i420_pinned_plus_sync"]["us"] / out["wall_get_frame_buffer_async_plus_sync"]["us"], 2)
    assert np.array_equal(planes, T.yuv_host(frame, "i420", flat=True)), "the planes are not the host rule's"
    s.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
