"""What the warp stage costs: python scripts/probe_warp.py W H [-p DIR] [-s pipeline] [--reps R]
A scene of W x H (default model: the procedural scene) renders one frame and warps it at its own size through five
grids -- identity, a 7 degree rotation, a lens, a grid a channel (chromatic) and a flip --, each out of place and in place:
  * k_warp, k_resize (bilinear, to the same size) and k_tile from the same run (HIP events on the scene's stream through
    tr_scene_profile_*, median and range over the repetitions; the frame is rendered again before every repetition);
  * a device-to-device copy of the frame (hipMemcpyAsync between two device buffers, HIP events) in the same run, and
    every case's time as a multiple of it.  In place adds two such copies (frame and flags) that k_warp's time does not hold;
  * the output tiles by path, a MODEL computed on the host from the frame's flags and the grid by the kernel's own rule,
    not a counter: the border colour (footprint wholly outside), zeros on the flags, or gathered."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tiny_renderer_amd as T  # noqa: E402
from probe_outline import HIP, drive, time_copy, stat  # noqa: E402
from probe_resize import flags_of  # noqa: E402

FLAG_TILES = 1024   # WARP_FLAG_TILES (csrc/tr_kernels.hip)


def census(flags, W, Hh, grid, w, h, clamp, border_black):
    """k_warp's three paths over its 128 x 16 output tiles."""
    g = np.asarray(grid, np.int64)
    g = g[None] if g.ndim == 3 else g
    out = {"tiles": 0, "tiles_border": 0, "tiles_zeros_on_flags": 0, "tiles_gathered": 0}
    for by in range((h + 15) // 16):
        for bx in range((w + 127) // 128):
            ncx = (min(128, w - 128 * bx) + 15) // 16
            n = g[:, by:by + 2, 8 * bx:8 * bx + ncx + 1]
            fx0, fx1, fy0, fy1 = int(n[..., 0].min()) >> 8, (int(n[..., 0].max()) >> 8) + 1, int(n[..., 1].min()) >> 8, (int(n[..., 1].max()) >> 8) + 1
            out["tiles"] += 1
            outside = fx1 < 0 or fx0 >= W or fy1 < 0 or fy0 >= Hh
            inside = fx0 >= 0 and fx1 < W and fy0 >= 0 and fy1 < Hh
            if outside and not clamp:
                out["tiles_border"] += 1
                continue
            cx0, cx1, cy0, cy1 = (min(max(v, 0), m - 1) for v, m in ((fx0, W), (fx1, W), (fy0, Hh), (fy1, Hh)))
            f = flags[(Hh - 1 - cy1) // 16:(Hh - 1 - cy0) // 16 + 1, cx0 // 128:cx1 // 128 + 1]
            if f.size <= FLAG_TILES and f.all() and (clamp or border_black or inside):
                out["tiles_zeros_on_flags"] += 1
            else:
                out["tiles_gathered"] += 1
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
    out = {"width": W, "height": Hh, "pipeline": a.pipeline, "model": a.path or "procedural", "reps": a.reps}
    s = T.Scene(W, Hh, mesh, texs, a.pipeline)
    drive(s)
    s.get_frame_buffer()
    flags = flags_of(s)
    out["tiles_flagged"] = int(flags.sum())
    out["tiles_of_the_frame"] = int(flags.size)
    copy = time_copy(3 * W * Hh, a.reps, a.warmup)
    out["copy_of_the_frame_d2d"] = copy
    dev = C.c_void_p()
    assert HIP.hipMalloc(C.byref(dev), 3 * W * Hh) == 0
    grids = (("identity", T.warp_grid_identity(W, Hh), False), ("rotate 7", T.warp_grid_rotate(7, W, Hh), False),
             ("lens -0.2, 0.05", T.warp_grid_lens(-0.2, 0.05, W, Hh), False), ("chromatic 3 px (a grid a channel)", T.warp_grid_chromatic(3, W, Hh), True),
             ("flip", T.warp_grid_from_function(lambda X, Y: (W - 1 - X, Y), W, Hh), False))
    cases, tile_us, resize_us = [], [], []
    for name, g, pc in grids:
        p = T.warp_params("border", (0, 0, 0), per_channel=pc)
        case = dict(census(flags, W, Hh, g, W, Hh, False, True), grid=name)
        s.set_warp(g, W, Hh)
        for where in ("out_of_place", "in_place"):
            us = []
            for i in range(a.warmup + a.reps):
                s.profile_enable(True)
                drive(s)
                if where == "out_of_place":
                    s.warp(p, dev.value)
                    if name == "identity":
                        s.resize_into(dev.value, W, Hh, "bilinear")
                else:
                    s.warp(p)
                s.sync()
                prof = s.profile_read()
                s.profile_enable(False)
                if i >= a.warmup:
                    us.append(prof["k_warp"]["total_ms"] * 1e3)
                    tile_us.append(prof["k_tile"]["total_ms"] * 1e3)
                    if "k_resize" in prof:
                        resize_us.append(prof["k_resize"]["total_ms"] * 1e3)
            case[where] = dict(stat(us))
            case[where]["copies"] = round(case[where]["us"] / copy["us"], 2)
        cases.append(case)
    HIP.hipFree(dev)
    out["cases"], out["k_tile"], out["k_resize_bilinear_same_size"] = cases, stat(tile_us), stat(resize_us)
    s.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
