"""What frame accumulation costs: python scripts/probe_accumulate.py W H [-p DIR] [-s pipeline] [-n FRAMES] [--reps N]
A scene with frames_per_launch = FRAMES (default 8; default model: the procedural scene) renders FRAMES frames of a
turning camera by one call and averages them under equal weights, out of place into device memory and in place:
  * k_accumulate alone (HIP events on the scene's stream, median and range over the repetitions; the frames are
    rendered again before every repetition, so that every in-place call finds the same frames and flags);
  * the bytes it really moves, from the frames' colour-clean flags: read -- every tile of every frame whose flag is
    down; written -- the whole frame out of place, the tiles some frame draws in place -- against the 6.29 TB/s copy
    rate of an MI355X (k_resolve reaches 0.88 of it).
Also the 96-frame render_frames step (--frames-step), for comparisons between builds (TR_LIBRARY)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tiny_renderer_amd as T  # noqa: E402

COPY_TBS = 6.29
HIP = C.CDLL("libamdhip64.so")
HIP.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
HIP.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
HIP.hipFree.argtypes = [C.c_void_p]


def orbit(n, of=96):
    p = np.zeros((n, 12), np.float32)
    for k in range(n):
        ang = 2.0 * np.pi * k / of
        p[k] = [0, 0, 1, np.sin(ang), 0, np.cos(ang), 0, 0, 0, 0, 1, 0]
    return p


def flags_of(s, n):
    """[n, tiles_y, tiles_x] bool: frame k's colour-clean flags (k = 0: the newest), and the tiles' pixel counts."""
    out = []
    for k in range(n):
        s.select_frame(k)
        s.sync()
        t = s.band_tiles()
        m = t.tiles_x * t.tiles_y
        words = np.zeros(m, np.uint32)
        assert HIP.hipMemcpy(words.ctypes.data, t.clean_device, 4 * m, 2) == 0   # (2: device to host)
        out.append(words.reshape(t.tiles_y, t.tiles_x) != 0)
    s.select_frame(0)
    ys = np.minimum(16, s.height - 16 * np.arange(t.tiles_y)).clip(0)
    xs = np.minimum(128, s.width - 128 * np.arange(t.tiles_x)).clip(0)
    return np.array(out), np.outer(ys, xs)


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("width", type=int)
    ap.add_argument("height", type=int)
    ap.add_argument("-p", dest="path", default=None)
    ap.add_argument("-s", dest="pipeline", default="phong")
    ap.add_argument("-n", dest="frames", type=int, default=8)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames-step", action="store_true", help="only the 96-frame render_frames step")
    a = ap.parse_args()
    W, Hh, pipe, n = a.width, a.height, a.pipeline, a.frames
    mesh, texs = T.load_assets(a.path) if a.path else T.synthetic_scene()
    if a.frames_step:
        s = T.Scene(W, Hh, mesh, texs, pipe)
        p = orbit(96)
        ts = []
        for i in range(2 + max(a.reps // 4, 5)):
            t0 = time.perf_counter()
            s.render_frames(p)
            s.sync()
            if i >= 2:
                ts.append((time.perf_counter() - t0) * 1e6)
        print(json.dumps({"width": W, "height": Hh, "pipeline": pipe, "library": T.library_path(),
                          "render_frames_96_us_med_min_max": [round(float(np.median(ts)), 1), round(min(ts), 1), round(max(ts), 1)],
                          "per_frame_us": round(float(np.median(ts)) / 96, 2)}))
        s.close()
        return
    s = T.Scene(W, Hh, mesh, texs, pipe, frames_per_launch=n)
    p = orbit(n)
    s.render_frames(p)
    clean, area = flags_of(s, n)
    read = int(((~clean) * area).sum()) * 3
    drawn_somewhere = int(((~clean).any(0) * area).sum()) * 3
    dev = C.c_void_p()
    assert HIP.hipMalloc(C.byref(dev), W * Hh * 3) == 0
    out = {"width": W, "height": Hh, "pipeline": pipe, "frames": n, "reps": a.reps, "tiles": int(area.size),
           "tiles_clean_per_frame": [int(c.sum()) for c in clean], "tiles_clean_in_every_frame": int(clean.all(0).sum()),
           "cases": []}
    for mode in ("out_of_place", "in_place"):
        k_us, tile_us = [], []
        for i in range(a.warmup + a.reps):
            s.profile_enable(True)
            s.render_frames(p)
            if mode == "in_place":
                s.accumulate_in_place(n)
            else:
                s.accumulate_into(n, dev.value)
            prof = s.profile_read()
            s.profile_enable(False)
            if i >= a.warmup:
                k_us.append(prof["k_accumulate"]["total_ms"] * 1e3)
                tile_us.append(prof["k_tile"]["total_ms"] * 1e3 / n)
        med = float(np.median(k_us))
        written = W * Hh * 3 if mode == "out_of_place" else drawn_somewhere
        b = read + written
        out["cases"].append({
            "mode": mode, "k_accumulate_us": round(med, 2), "k_accumulate_us_min_max": [round(min(k_us), 2), round(max(k_us), 2)],
            "k_tile_us_per_frame": round(float(np.median(tile_us)), 2), "bytes_read": read, "bytes_written": written,
            "GBps": round(b / (med * 1e-6) / 1e9, 1), "share_of_copy_rate": round(b / (med * 1e-6) / 1e12 / COPY_TBS, 4)})
    s.close()
    HIP.hipFree(dev)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
