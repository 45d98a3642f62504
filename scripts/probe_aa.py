"""What edge anti-aliasing costs: python scripts/probe_aa.py W H [-p DIR] [-s pipeline] [--reps R]
A scene (default model: the procedural scene) renders one frame and filters it at search 4 and 8, out of place into
device memory and in place (k_aa into the scratch frame; the copy back is the frame copy timed beside it):
  * k_aa alone, and k_tile and k_outline (radius 1) for scale, all timed in the same run (HIP events on the scene's
    stream through tr_scene_profile_*, median and range over the repetitions; the frame is rendered again before every
    repetition, so that every in-place call finds the same frame and flags);
  * a device-to-device copy of the frame (hipMemcpyAsync between two device buffers, HIP events) in the same run;
  * the route the stage replaces: the same picture rendered at twice the edge (k_tile at 2 W x 2 H) plus k_resolve by 2;
  * the tiles by path, a MODEL computed on the host from the frame and its flags, not a counter: zeros on the flags
    alone (all nine colour flags of the neighbourhood up), copied (staged, no pixel passes the contrast test) and
    filtered, and the share of the pixels that pass."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tiny_renderer_amd as T  # noqa: E402
from probe_outline import HIP, F32_MIN_BITS, drive, tiles_any, time_copy, stat  # noqa: E402


def census(fb, z, p):
    """Tiles by path for one launch over the frame fb [H, W, 3] (row 0 = top) and its depth z [H, W] (y up)."""
    c = fb.astype(np.int32)
    lum = (54 * c[..., 0] + 183 * c[..., 1] + 19 * c[..., 2] + 128) >> 8
    pad = np.pad(lum, 1, mode="edge")
    five = np.stack([pad[1:-1, 1:-1], pad[:-2, 1:-1], pad[2:, 1:-1], pad[1:-1, :-2], pad[1:-1, 2:]])
    hi, lo = five.max(0), five.min(0)
    rng = hi - lo
    passed = (rng != 0) & (rng >= np.maximum(p.contrast_min, (hi * p.contrast_rel + 128) >> 8))
    d, k = tiles_any(z.view(np.uint32) != F32_MIN_BITS), tiles_any(passed[::-1])
    near = np.zeros_like(d)   # a drawn tile in the 3 x 3 neighbourhood: the tile is staged
    q = np.pad(d, 1)
    for dy in range(3):
        for dx in range(3):
            near |= q[dy:dy + d.shape[0], dx:dx + d.shape[1]]
    return {"tiles": int(d.size), "tiles_filtered": int(k.sum()), "tiles_copied": int((near & ~k).sum()),
            "tiles_zeros_on_flags": int((~near).sum()), "pixels_passed_share": round(float(passed.mean()), 4)}


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
    fb, z = s.get_frame_buffer(), s.read_z_f32()
    dev = C.c_void_p()
    assert HIP.hipMalloc(C.byref(dev), W * Hh * 3) == 0
    out = {"width": W, "height": Hh, "pipeline": a.pipeline, "model": a.path or "procedural", "reps": a.reps,
           "frame_copy_d2d": time_copy(W * Hh * 3, a.reps, a.warmup), "cases": []}
    ink_us, tile_us = [], []
    ink = T.outline_params(radius=1, depth_step=4.0)
    for i in range(a.warmup + a.reps):
        s.profile_enable(True)
        drive(s)
        s.outline(ink, dev.value)
        s.sync()
        prof = s.profile_read()
        s.profile_enable(False)
        if i >= a.warmup:   # (k_tile is not taken here: the outline fetches the depth by a depth-only repeat of the pass)
            ink_us.append(prof["k_outline"]["total_ms"] * 1e3)
    out["k_outline_radius1"] = stat(ink_us)
    for search in (4, 8):
        p = T.aa_params(search=search)
        case = dict(census(fb, z, p), search=search)
        for mode in ("out_of_place", "in_place"):
            us = []
            for i in range(a.warmup + a.reps):
                s.profile_enable(True)
                drive(s)
                s.antialias(p, None if mode == "in_place" else dev.value)
                s.sync()
                prof = s.profile_read()
                s.profile_enable(False)
                if i >= a.warmup:
                    us.append(prof["k_aa"]["total_ms"] * 1e3)
                    tile_us.append(prof["k_tile"]["total_ms"] * 1e3)
            case[mode] = stat(us)
        out["cases"].append(case)
    out["k_tile"] = stat(tile_us)
    s.close()
    HIP.hipFree(dev)
    # the route this stage replaces: the picture at twice the edge, box-filtered by k_resolve
    big = T.Scene(2 * W, 2 * Hh, mesh, texs, a.pipeline)
    big_tile, big_resolve = [], []
    for i in range(a.warmup + a.reps):
        big.profile_enable(True)
        drive(big)
        big.resolve(2)
        prof = big.profile_read()
        big.profile_enable(False)
        if i >= a.warmup:
            big_tile.append(prof["k_tile"]["total_ms"] * 1e3)
            big_resolve.append(prof["k_resolve"]["total_ms"] * 1e3)
    big.close()
    out["ssaa2"] = {"k_tile": stat(big_tile), "k_resolve": stat(big_resolve)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
