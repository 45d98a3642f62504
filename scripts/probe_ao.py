"""What ambient occlusion costs: python scripts/probe_ao.py W H [-p DIR] [-s pipeline] [--reps N]
A scene with TR_OPT_STORE_DEPTH (default: the procedural scene), default camera and light, shaded by
Scene.ambient_occlusion at radius 4, 8 and 16 with 1 and 4 rings:
  * k_ao alone (HIP events on the scene's stream, median and range over the repetitions) beside the same frame's k_tile;
  * the tiles it enters (tiles with a drawn pixel; the others leave after one word) and its bytes -- per entered tile the
    z of the tile and of the halo pieces that are not behind a raised flag, and colour read and written for the
    16-pixel shares in which a pixel changes -- against the 6.29 TB/s copy rate of an MI355X;
  * LDS reads per drawn pixel: 16 * rings samples and the pixel's own depth.
Also the 96-frame render_frames step (--frames-step), for comparisons between builds (TR_LIBRARY)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tiny_renderer_amd as T  # noqa: E402

COPY_TBS = 6.29
F32_MIN_BITS = np.uint32(0xFF7FFFFF)


def frame(s):
    s.clear()
    s.set_light_direction([0.0, 0.0, 1.0])
    s.set_camera([0.0, 0.0, 1.0], [0, 0, 0], [0, 1, 0])
    s.render()


def tiles(mask):
    """[ty, tx] bool of a [H, W] mask: does the 128 x 16 tile hold a set pixel?"""
    Hh, W = mask.shape
    ty, tx = (Hh + 15) // 16, (W + 127) // 128
    pad = np.zeros((ty * 16, tx * 128), bool)
    pad[:Hh, :W] = mask
    return pad.reshape(ty, 16, tx, 128).any((1, 3))


def z_bytes(entered, radius):
    """Bytes of z the kernel loads: per entered tile its own 128 x 16 floats and, for each of the eight tiles around it
    that exists and is entered too (flag down), the halo pieces inside it (16-byte pieces: columns rounded up to 4)."""
    ty, tx = entered.shape
    cols = -(-radius // 4) * 4
    pad = np.zeros((ty + 2, tx + 2), bool)
    pad[1:-1, 1:-1] = entered
    n = lambda dy, dx: int((entered & pad[1 + dy:1 + dy + ty, 1 + dx:1 + dx + tx]).sum())
    side = (n(0, -1) + n(0, 1)) * 16 * cols
    above = (n(-1, 0) + n(1, 0)) * radius * 128
    corner = (n(-1, -1) + n(-1, 1) + n(1, -1) + n(1, 1)) * radius * cols
    return 4 * (int(entered.sum()) * 128 * 16 + side + above + corner)


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("width", type=int)
    ap.add_argument("height", type=int)
    ap.add_argument("-p", dest="path", default=None)
    ap.add_argument("-s", dest="pipeline", default="phong")
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames-step", action="store_true", help="only the 96-frame render_frames step")
    a = ap.parse_args()
    W, Hh, pipe = a.width, a.height, a.pipeline
    mesh, texs = T.load_assets(a.path) if a.path else T.synthetic_scene()
    if a.frames_step:
        s = T.Scene(W, Hh, mesh, texs, pipe)
        p = np.zeros((96, 12), np.float32)
        for k in range(96):
            ang = 2.0 * np.pi * k / 96
            p[k] = [0, 0, 1, np.sin(ang), 0, np.cos(ang), 0, 0, 0, 0, 1, 0]
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
    s = T.Scene(W, Hh, mesh, texs, pipe, store_depth=True, auto_group=False)
    frame(s)
    fb, z = s.get_frame_buffer(), s.read_z_f32()
    drawn = z.view(np.uint32) != F32_MIN_BITS
    entered = tiles(drawn)
    out = {"width": W, "height": Hh, "pipeline": pipe, "reps": a.reps, "tiles_total": int(entered.size),
           "tiles_entered": int(entered.sum()), "pixels_drawn": int(drawn.sum()), "cases": []}
    for radius, rings in ((4, 1), (8, 1), (16, 1), (4, 4), (8, 4), (16, 4)):
        shaded = T.ambient_occlusion_host(z, fb, radius=radius, rings=rings)
        px = (shaded != fb).any(-1)[::-1]
        ty, tx = entered.shape
        pad = np.zeros((ty * 16, tx * 128), bool)
        pad[:Hh, :W] = px
        shares = int(pad.reshape(ty * 16, tx * 8, 16).any(2).sum())      # 16-pixel shares with a changed pixel
        k_us, tile_us = [], []
        for i in range(a.warmup + a.reps):
            s.profile_enable(True)
            frame(s)
            s.ambient_occlusion(radius=radius, rings=rings)
            prof = s.profile_read()
            s.profile_enable(False)
            if i >= a.warmup:
                k_us.append(prof["k_ao"]["total_ms"] * 1e3)
                tile_us.append(prof["k_tile"]["total_ms"] * 1e3)
        med = float(np.median(k_us))
        b = z_bytes(entered, radius) + shares * 48 * 2
        out["cases"].append({
            "radius": radius, "rings": rings, "k_ao_us": round(med, 2), "k_ao_us_min_max": [round(min(k_us), 2), round(max(k_us), 2)],
            "k_tile_us": round(float(np.median(tile_us)), 2), "pixels_changed": int(px.sum()), "shares_rewritten": shares,
            "bytes": b, "GBps": round(b / (med * 1e-6) / 1e9, 1), "share_of_copy_rate": round(b / (med * 1e-6) / 1e12 / COPY_TBS, 4),
            "lds_reads_per_drawn_pixel": 16 * rings + 1,
            "lds_sample_reads_per_us": round(int(drawn.sum()) * (16 * rings + 1) / med, 1)})
    s.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
