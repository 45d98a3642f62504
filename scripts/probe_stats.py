"""What frame statistics cost: python scripts/probe_stats.py W H [-p DIR] [-s pipeline] [--reps R]
A scene (default model: the procedural scene; stored depth) renders one frame and reduces it to a record in page-locked
host memory (Scene.frame_stats into pinned_stats), and from one run reports the median [min, max] over the repetitions of:
  * k_stats + k_stats_finish (HIP events on the scene's stream through tr_scene_profile_*, both launches in one
    bracket), colour only and with depth, over the whole frame and over a central window (the middle half of each
    axis), for the rendered frame and for the same frame graded in place to one flat colour that is not black -- every
    flag down, every pixel the same: the worst case for contention on the LDS histograms;
  * a device-to-device copy of the frame (hipMemcpyAsync between two device buffers, HIP events);
  * k_tile, for scale;
  * the streamed read-back the record is there to replace: get_frame_buffer_async into tr_host_alloc memory plus sync,
    and frame_stats into pinned memory plus sync, both wall clock around a frame that has already been rendered;
  * the tiles by path -- answered from the flag alone, skipped (outside the window), read -- computed on the host from the
    frame's colour flags, not a counter."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tiny_renderer_amd as T  # noqa: E402
from scripts.probe_grade import HIP, colour_flags, drive, time_copy  # noqa: E402


def med(us):
    return {"us": round(float(np.median(us)), 2), "us_min_max": [round(min(us), 2), round(max(us), 2)]}


def census(W, Hh, cflags, window):
    """Tiles of one k_stats launch by path."""
    ty, tx = cflags.shape
    x0, y0, w, h = window if window else (0, 0, W, Hh)
    iy0, iy1 = Hh - (y0 + h), Hh - y0                     # the kernel's rows count from the bottom
    out = {"tiles": int(ty * tx), "tiles_flag": 0, "tiles_skipped": 0, "tiles_read": 0}
    for j in range(ty):
        for i in range(tx):
            meets = max(x0, 128 * i) < min(x0 + w, 128 * i + 128) and max(iy0, 16 * j) < min(iy1, 16 * j + 16)
            out["tiles_skipped" if not meets else "tiles_flag" if cflags[j, i] else "tiles_read"] += 1
    return out


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
    first = s.get_frame_stats(depth=True)
    zkw = dict(z_lo=float(first.z_min), z_scale=float(np.float32(256.0) / max(np.float32(first.z_max) - np.float32(first.z_min), np.float32(1e-6))))
    record = s.pinned_stats()
    frame = s.pinned_frame()
    flat = np.empty((2, 2, 2, 3), np.uint8)
    flat[...] = (9, 200, 77)
    window = (W // 4, Hh // 4, max(1, W // 2), max(1, Hh // 2))
    out = {"width": W, "height": Hh, "pipeline": a.pipeline, "reps": a.reps, "record_bytes": int(record.nbytes),
           "frame_bytes": 3 * W * Hh, "workgroups": 0, "first_record": repr(first),
           "frame_copy_d2d": time_copy(W * Hh * 3, a.reps, a.warmup), "cases": []}
    for frame_kind in ("rendered", "flat"):
        s.set_lut(flat if frame_kind == "flat" else None)
        for win_name, win in (("whole", None), ("window", window)):
            for depth in (False, True):
                k_us, tile_us = [], []
                for i in range(a.warmup + a.reps):
                    s.profile_enable(True)
                    drive(s)
                    if frame_kind == "flat":
                        s.grade()
                    s.frame_stats(window=win, depth=depth, out=record, **(zkw if depth else {}))
                    s.sync()
                    prof = s.profile_read()
                    s.profile_enable(False)
                    if i >= a.warmup:
                        k_us.append(prof["k_stats"]["total_ms"] * 1e3)
                        tile_us.append(prof["k_tile"]["total_ms"] * 1e3)
                flags = cflags if frame_kind == "rendered" else np.zeros_like(cflags)
                got = T.FrameStats(record)
                case = {"frame": frame_kind, "window": win_name, "depth": depth, "k_stats_and_finish": med(k_us), "k_tile": med(tile_us),
                        "n_pixels": got.n_pixels, "n_drawn": got.n_drawn}
                case.update(census(W, Hh, flags, win))
                out["cases"].append(case)
    out["workgroups"] = s.debug_stats_grid(0)
    s.set_lut(None)
    # wall clock, the frame already rendered and waited for: what a caller pays to see the frame, and to see the record
    for name, call in (("read_back_async_plus_sync", lambda: s.get_frame_buffer_async(frame)),
                       ("stats_colour_pinned_plus_sync", lambda: s.frame_stats(out=record)),
                       ("stats_depth_pinned_plus_sync", lambda: s.frame_stats(depth=True, out=record, **zkw))):
        us = []
        for i in range(a.warmup + a.reps):
            drive(s)
            s.sync()
            if name.startswith("read_back"):
                s.host_buffer_written(frame)              # (every repetition streams the whole frame's drawn tiles)
            t0 = time.perf_counter()
            call()
            s.sync()
            if i >= a.warmup:
                us.append((time.perf_counter() - t0) * 1e6)
        out[name] = med(us)
    s.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
