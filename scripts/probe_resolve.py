"""What the supersampling resolve costs: python scripts/probe_resolve.py W H pipeline f [--reps N] [--synthetic]
k_resolve and k_tile of the same frame (HIP events on the scene's stream, median per frame), the tiles k_resolve reads,
the bytes it moves against the 6.29 TB/s copy rate of an MI355X, and render -> resolve into page-locked memory -> sync
against render -> get_frame_buffer_async of a frame rendered directly at the OUTPUT size."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tiny_renderer_amd as T  # noqa: E402

COPY_TBS = 6.29


def frame(s, angle=0.0):
    s.clear()
    s.set_light_direction([float(np.sin(angle)), 0.0, float(np.cos(angle))])
    s.set_camera([float(np.sin(angle)), 0.0, float(np.cos(angle))], [0, 0, 0], [0, 1, 0])
    s.render()


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("width", type=int)
    ap.add_argument("height", type=int)
    ap.add_argument("pipeline")
    ap.add_argument("factor", type=int)
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("-p", dest="asset_path", default=None, help="asset folder; default: the procedural scene")
    a = ap.parse_args()
    import torch
    mesh, texs = T.load_assets(a.asset_path) if a.asset_path else T.synthetic_scene()
    W, Hh, f = a.width, a.height, a.factor
    s = T.Scene(W, Hh, mesh, texs, a.pipeline, auto_group=False)
    out_bytes = 3 * (W // f) * (Hh // f)
    dev = torch.empty(out_bytes, dtype=torch.uint8, device="cuda")
    pinned = s.pinned_resolved(f)

    # tiles the kernel reads
    frame(s)
    s.sync()
    t = s.band_tiles()
    n = t.tiles_x * t.tiles_y

    class Flags:
        __cuda_array_interface__ = {"shape": (n,), "typestr": "<u4", "data": (int(t.clean_device), False), "version": 2}

    read = int((torch.as_tensor(Flags(), device="cuda").cpu().numpy() == 0).sum())

    # per-kernel device times, one profiled frame at a time
    k_res, k_tile = [], []
    for i in range(a.warmup + a.reps):
        s.profile_enable(True)
        frame(s)
        s.resolve_into(f, dev.data_ptr())
        prof = s.profile_read()
        if i >= a.warmup:
            k_res.append(prof["k_resolve"]["total_ms"] * 1e3)
            k_tile.append(prof["k_tile"]["total_ms"] * 1e3)
    s.profile_enable(False)
    res_us, tile_us = float(np.median(k_res)), float(np.median(k_tile))
    bytes_read = read * 128 * 16 * 3   # (whole tiles: an upper bound at the frame's partial edges)
    gbs = (bytes_read + out_bytes) / (res_us * 1e-6) / 1e9

    # end to end on the host clock: supersampled and resolved into page-locked memory ...
    def wall(fn, reps):
        ts = []
        for i in range(a.warmup + reps):
            t0 = time.perf_counter()
            fn()
            if i >= a.warmup:
                ts.append((time.perf_counter() - t0) * 1e6)
        return float(np.median(ts))

    def ssaa():
        frame(s)
        s.resolve_into(f, pinned)
        s.sync()

    ssaa_us = wall(ssaa, a.reps)
    s.close()
    # ... against the frame rendered at the output size and read back
    d = T.Scene(W // f, Hh // f, mesh, texs, a.pipeline, auto_group=False)
    direct_pinned = d.pinned_frame()

    def direct():
        frame(d)
        d.get_frame_buffer_async(direct_pinned)
        d.sync()

    direct_us = wall(direct, a.reps)
    d.close()
    print(json.dumps({"width": W, "height": Hh, "pipeline": a.pipeline, "factor": f, "reps": a.reps,
                      "k_resolve_us": round(res_us, 2), "k_tile_us": round(tile_us, 2),
                      "k_resolve_us_min_max": [round(min(k_res), 2), round(max(k_res), 2)],
                      "tiles_read": read, "tiles_total": n, "bytes_read": bytes_read, "bytes_written": out_bytes,
                      "GBps": round(gbs, 1), "share_of_copy_rate": round(gbs / (COPY_TBS * 1e3), 3),
                      "render_resolve_pinned_sync_us": round(ssaa_us, 1),
                      "render_at_output_size_readback_sync_us": round(direct_us, 1)}))


if __name__ == "__main__":
    main()
