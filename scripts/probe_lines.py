"""What lines cost: python scripts/probe_lines.py W H [-p DIR] [-s pipeline] [--reps N]
A scene (default model: the procedural scene) renders one frame and draws tables of segments into it, out of place into
device memory and in place:
  * the mesh's wireframe (wireframe_lines) at width 1 and 3, depth-tested and x-ray; a 12-segment box of frame-long lines;
    2^20 random short segments -- k_lines alone and k_tile for scale (HIP events on the scene's stream through
    tr_scene_profile_*, median and range over the repetitions; the frame is rendered again before every repetition, so
    that every in-place call finds the same frame, depth and flags);
  * beside it, in the same run: a device-to-device copy of the frame (hipMemcpyAsync between two device buffers, HIP
    events) and k_layer with a full-frame opaque rgb8 layer;
  * the host time of set_lines for each table (validation, binning and the upload), the bins (non-empty tiles, entries),
    and the tiles by path for one in-place call -- skipped (no list), visited, lowered (flagged, visited and with a
    winner) -- from the colour flags before and after the call;
  * how many wireframe pixels the depth test shows for a sweep of depth_bias against the x-ray count: the means to choose
    the CLI's default --wire-bias."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tiny_renderer_amd as T  # noqa: E402
from probe_bloom import HIP, drive, colour_flags, time_copy  # noqa: E402
from probe_convolve import timed  # noqa: E402


def box_table(W, Hh):
    """Twelve frame-long segments: the frame's edges, both diagonals, and six lines across it."""
    w, h = W - 1, Hh - 1
    ends = [(0, 0, w, 0), (0, h, w, h), (0, 0, 0, h), (w, 0, w, h), (0, 0, w, h), (0, h, w, 0), (0, h // 3, w, 2 * h // 3), (0, 2 * h // 3, w, h // 3),
            (w // 3, 0, 2 * w // 3, h), (2 * w // 3, 0, w // 3, h), (0, h // 2, w, h // 2), (w // 2, 0, w // 2, h)]
    e = np.array(ends, np.int64)
    return T.lines_table(e[:, :2], np.full(12, 1000.0), e[:, 2:], np.full(12, 1000.0), (255, 200, 0, 255))


def short_table(W, Hh, n=1 << 20):
    rng = np.random.default_rng(1)
    a = np.stack([rng.integers(0, W, n), rng.integers(0, Hh, n)], 1)
    b = a + rng.integers(-12, 13, (n, 2))
    return T.lines_table(a, rng.random(n) * 100.0, b, rng.random(n) * 100.0, rng.integers(0, 256, (n, 4)))


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
    dev = C.c_void_p()
    assert HIP.hipMalloc(C.byref(dev), W * Hh * 3) == 0
    out = {"width": W, "height": Hh, "pipeline": a.pipeline, "reps": a.reps, "frame_copy_d2d": time_copy(W * Hh * 3, a.reps, a.warmup), "cases": []}
    wire = T.wireframe_lines(s, mesh, (255, 255, 255, 255))
    tables = (("wireframe", wire, ((1, True), (3, True), (1, False), (3, False))), ("box of 12 frame-long lines", box_table(W, Hh), ((1, True), (3, False))),
              ("2^20 random short segments", short_table(W, Hh), ((1, True), (1, False))))
    for label, tab, combos in tables:
        t0 = time.perf_counter()
        s.set_lines(tab)
        set_ms = (time.perf_counter() - t0) * 1e3
        tiles, entries = s.debug_line_bins()
        for width, test in combos:
            case = {"table": label, "segments": int(tab.shape[0]), "set_lines_host_ms": round(set_ms, 2), "listed_tiles": tiles, "entries": entries,
                    "width": width, "depth_test": test}
            drive(s)
            before = colour_flags(s)
            s.lines(width, depth_test=test)
            after = colour_flags(s)
            case.update(tiles=int(before.size), tiles_skipped=int(before.size) - tiles, tiles_visited=tiles, tiles_lowered=int((before & ~after).sum()))
            for mode in ("out_of_place", "in_place"):
                k, tile = timed(s, lambda: s.lines(width, depth_test=test, out=None if mode == "in_place" else dev.value), "k_lines", a.reps, a.warmup)
                case[mode] = {"k_lines": k, "k_tile": tile}
            out["cases"].append(case)
    # the bias sweep on the wireframe: pixels shown under the test against the x-ray count
    s.set_lines(wire)
    drive(s)
    plain = s.get_frame_buffer()
    xray = int((s.get_lined(1, depth_test=False) != plain).any(-1).sum())
    out["bias_sweep"] = {"xray_pixels": xray, "shown": {str(b): int((s.get_lined(1, depth_bias=b) != plain).any(-1).sum()) for b in (0.0, 0.25, 0.5, 1.0, 2.0, 4.0, 8.0)}}
    # beside it: k_layer with a full-frame opaque layer in device memory
    out["beside"] = {}
    if W <= 8192 and Hh <= 8192:
        img = T.layer_gradient(W, Hh, (20, 40, 200), (240, 230, 220))
        back = C.c_void_p()
        assert HIP.hipMalloc(C.byref(back), img.nbytes) == 0
        assert HIP.hipMemcpy(back, img.ctypes.data_as(C.c_void_p), img.nbytes, 1) == 0
        for mode in ("out_of_place", "in_place"):
            k, _ = timed(s, lambda: s.layer(back.value, out=None if mode == "in_place" else dev.value, width=W, height=Hh), "k_layer", a.reps, a.warmup)
            out["beside"][mode] = {"k_layer_full_frame": k}
        HIP.hipFree(back)
    s.close()
    HIP.hipFree(dev)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
