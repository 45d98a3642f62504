"""What depth compositing costs: python scripts/probe_composite.py W H [-p DIR_A] [--with DIR_B] [-s pipeline] [--reps N]
Scene B (default: a second procedural sphere) merged into scene A (default: the procedural scene), both with A's images,
default camera and light:
  * k_composite alone (HIP events on dst's stream, median and range over the repetitions), the tiles it reads (src's
    tiles with a covered pixel) and its bytes -- per pixel of such a tile 4 + 4 + 3 read and up to 7 written -- against
    the 6.29 TB/s copy rate of an MI355X;
  * the step `render A; render B; composite; sync` (both scenes store their depth) against what a caller could do
    before: one scene of the concatenated mesh A ++ B, and the host merge -- both frames and both z buffers read back,
    the rule in numpy.
Also the 96-frame render_frames step of scene A (--frames-step), for comparisons between builds (TR_LIBRARY)."""
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


def frame(s, angle=0.0):
    s.clear()
    s.set_light_direction([float(np.sin(angle)), 0.0, float(np.cos(angle))])
    s.set_camera([float(np.sin(angle)), 0.0, float(np.cos(angle))], [0, 0, 0], [0, 1, 0])
    s.render()


def concat(a, b):
    ib = np.asarray(b["idx"], np.uint32).reshape(-1, 9).copy()
    n = [np.asarray(a[k]).reshape(-1, 3).shape[0] for k in ("pos", "tex", "nrm")]
    for col in range(9):
        ib[:, col] += np.uint32(n[col % 3])
    out = {k: np.concatenate([np.asarray(a[k], np.float32).reshape(-1, 3), np.asarray(b[k], np.float32).reshape(-1, 3)])
           for k in ("pos", "tex", "nrm")}
    out["idx"] = np.concatenate([np.asarray(a["idx"], np.uint32).reshape(-1, 9), ib])
    return out


def wall(fn, warmup, reps):
    ts = []
    for i in range(warmup + reps):
        t0 = time.perf_counter()
        fn()
        if i >= warmup:
            ts.append((time.perf_counter() - t0) * 1e6)
    return [round(float(np.median(ts)), 1), round(float(min(ts)), 1), round(float(max(ts)), 1)]


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("width", type=int)
    ap.add_argument("height", type=int)
    ap.add_argument("-p", dest="path_a", default=None)
    ap.add_argument("--with", dest="path_b", default=None)
    ap.add_argument("-s", dest="pipeline", default="phong")
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--frames-step", action="store_true", help="only the 96-frame render_frames step of scene A")
    a = ap.parse_args()
    W, Hh, pipe = a.width, a.height, a.pipeline
    A, texs = T.load_assets(a.path_a) if a.path_a else T.synthetic_scene()
    if a.frames_step:
        s = T.Scene(W, Hh, A, texs, pipe)
        p = np.zeros((96, 12), np.float32)
        for k in range(96):
            ang = 2.0 * np.pi * k / 96
            p[k] = [0, 0, 1, np.sin(ang), 0, np.cos(ang), 0, 0, 0, 0, 1, 0]

        def step():
            s.render_frames(p)
            s.sync()

        med = wall(step, 2, max(a.reps // 4, 5))
        print(json.dumps({"width": W, "height": Hh, "pipeline": pipe, "library": T.library_path(),
                          "render_frames_96_us_med_min_max": med, "per_frame_us": round(med[0] / 96, 2)}))
        s.close()
        return
    B = T.load_assets(a.path_b)[0] if a.path_b else T.synthetic_scene(n_lat=25, n_lon=60, radius=0.55)[0]
    d = T.Scene(W, Hh, A, texs, pipe, store_depth=True, auto_group=False)
    s = T.Scene(W, Hh, B, texs, pipe, store_depth=True, auto_group=False)

    # the tiles k_composite reads, and the pixels that win
    frame(d), frame(s)
    zs, zd = s.read_z_f32(), d.read_z_f32()
    covered = zs.view(np.uint32) != F32_MIN_BITS
    ty, tx = (Hh + 15) // 16, (W + 127) // 128
    pad = np.zeros((ty * 16, tx * 128), bool)
    pad[:Hh, :W] = covered
    read = int(pad.reshape(ty, 16, tx, 128).any((1, 3)).sum())
    won = int((covered & ~(zs <= zd)).sum())

    k_us = []
    for i in range(a.warmup + a.reps):
        frame(d), frame(s)
        d.sync(), s.sync()
        d.profile_enable(True)
        d.composite(s)
        prof = d.profile_read()
        d.profile_enable(False)
        if i >= a.warmup:
            k_us.append(prof["k_composite"]["total_ms"] * 1e3)
    med = float(np.median(k_us))
    px = read * 128 * 16      # (whole tiles: an upper bound at the frame's partial edges)
    b_read, b_written_max = px * 11, px * 7
    b_actual = px * 8 + won * (3 + 3 + 4 + 3)   # z of both; colour of both, z and colour stored where a pixel won (per pixel; pieces are coarser)

    def merged_step():
        frame(d), frame(s)
        d.composite(s)
        d.sync()

    t_merge = wall(merged_step, a.warmup, a.reps)
    both = T.Scene(W, Hh, concat(A, B), texs, pipe, auto_group=False)

    def one_scene():
        frame(both)
        both.sync()

    t_one = wall(one_scene, a.warmup, a.reps)
    both.close()
    pa, pb = T.Scene(W, Hh, A, texs, pipe, auto_group=False), T.Scene(W, Hh, B, texs, pipe, auto_group=False)

    def host_merge():
        frame(pa), frame(pb)
        fa, fb = pa.get_frame_buffer(), pb.get_frame_buffer()
        za, zb = pa.read_z_f32(), pb.read_z_f32()
        wins = (zb.view(np.uint32) != F32_MIN_BITS) & ~(zb <= za)
        np.copyto(fa[::-1], fb[::-1], where=wins[..., None])
        np.copyto(za, zb, where=wins)

    t_host = wall(host_merge, 2, max(a.reps // 8, 3))
    for q in (d, s, pa, pb):
        q.close()
    print(json.dumps({
        "width": W, "height": Hh, "pipeline": pipe, "reps": a.reps,
        "k_composite_us": round(med, 2), "k_composite_us_min_max": [round(min(k_us), 2), round(max(k_us), 2)],
        "tiles_read": read, "tiles_total": ty * tx, "pixels_won": won,
        "bytes_read": b_read, "bytes_written_at_most": b_written_max, "bytes_per_pixel_estimate": b_actual,
        "GBps_read_plus_at_most_written": round((b_read + b_written_max) / (med * 1e-6) / 1e9, 1),
        "GBps_estimate": round(b_actual / (med * 1e-6) / 1e9, 1),
        "share_of_copy_rate_estimate": round(b_actual / (med * 1e-6) / 1e12 / COPY_TBS, 3),
        "render_render_composite_sync_us_med_min_max": t_merge,
        "one_scene_of_concatenated_mesh_sync_us_med_min_max": t_one,
        "host_merge_us_med_min_max": t_host}))


if __name__ == "__main__":
    main()
