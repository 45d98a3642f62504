"""What shared shadows cost: python scripts/probe_shadow_merge.py W H [-p DIR_A] [--with DIR_B] [-s shadow|occlusion] [--reps N]
Scene B (default: a second procedural sphere) beside scene A (default: the procedural scene), both with A's images and
stored depth, default camera and light, B moved by --with-offset:
  * k_shadow_merge alone (HIP events on dst's stream, median and range over the repetitions) beside k_composite on the
    same two frames; the tiles of each of its three cases -- src's flag up (left after one word), dst's flag up (src's
    values taken, 4 bytes read and 4 written per pixel), both down (8 read, 4 written per 16-byte piece that changed) --
    and its bytes against the 6.29 TB/s copy rate of an MI355X.  The bytes are a MODEL, not a counter: the cases are
    taken from the two buffers read back beforehand (a tile without a drawn pixel counts as behind its flag) and tiles
    at the frame's partial edges count as whole tiles, so they are an upper bound;
  * the full sequence `shadow passes; merge both ways; colour passes; composite; sync` against one scene of the
    concatenated mesh A ++ B, in time and in every byte of colour, z and shadow buffer."""
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


def aim(s, angle=0.0, light=0.5):
    s.set_light_direction([float(np.sin(light)), 0.0, float(np.cos(light))])
    s.set_camera([float(np.sin(angle)), 0.0, float(np.cos(angle))], [0, 0, 0], [0, 1, 0])


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


def tiles(mask):
    Hh, W = mask.shape
    ty, tx = (Hh + 15) // 16, (W + 127) // 128
    pad = np.zeros((ty * 16, tx * 128), bool)
    pad[:Hh, :W] = mask
    return pad.reshape(ty, 16, tx, 128).any((1, 3))


def sequence(a, b, n_a):
    for q in (a, b):
        q.clear(), aim(q)
    a.render_shadow_pass(), b.render_shadow_pass()
    a.shadow_merge(b), b.shadow_merge(a)
    a.render_colour_pass(), b.render_colour_pass()
    a.composite(b, winner_base=n_a)


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("width", type=int)
    ap.add_argument("height", type=int)
    ap.add_argument("-p", dest="path_a", default=None)
    ap.add_argument("--with", dest="path_b", default=None)
    ap.add_argument("--with-offset", default="0.35,0.0,0.45", metavar="X,Y,Z")
    ap.add_argument("-s", dest="pipeline", default="shadow", choices=("shadow", "occlusion"))
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    W, Hh, pipe = a.width, a.height, a.pipeline
    A, texs = T.load_assets(a.path_a) if a.path_a else T.synthetic_scene()
    B = T.load_assets(a.path_b)[0] if a.path_b else T.synthetic_scene(n_lat=25, n_lon=60, radius=0.55)[0]
    B = T.apply_instances(B, np.array([[float(v) for v in a.with_offset.split(",")] + [1.0]], np.float32))
    n_a = np.asarray(A["idx"]).reshape(-1, 9).shape[0]
    d = T.Scene(W, Hh, A, texs, pipe, store_depth=True, auto_group=False)
    s = T.Scene(W, Hh, B, texs, pipe, store_depth=True, auto_group=False)

    def passes():
        for q in (d, s):
            q.clear(), aim(q)
            q.render_shadow_pass(), q.render_colour_pass()

    # the tiles of the three cases, from the buffers themselves (a tile without a drawn pixel counts as behind its flag)
    passes()
    zd, zs = d.read_shadow_f32(), s.read_shadow_f32()
    td, ts = tiles(zd.view(np.uint32) != F32_MIN_BITS), tiles(zs.view(np.uint32) != F32_MIN_BITS)
    n_tiles = int(td.size)
    left, taken, both_down = int((~ts).sum()), int((ts & ~td).sum()), int((ts & td).sum())
    with np.errstate(invalid="ignore"):
        merged = np.where(zs >= zd, zs.view(np.uint32), zd.view(np.uint32))
    changed = merged != zd.view(np.uint32)
    elementwise = np.repeat(np.repeat(ts & td, 16, 0), 128, 1)[:Hh, :W]
    w4 = W - W % 4
    pieces = int((changed & elementwise)[:, :w4].reshape(Hh, w4 // 4, 4).any(2).sum())
    tile_px = 128 * 16      # (whole tiles: an upper bound at the frame's partial edges)
    b_read = taken * tile_px * 4 + both_down * tile_px * 8
    b_written = taken * tile_px * 4 + pieces * 16

    k_merge, k_comp = [], []
    for i in range(a.warmup + a.reps):
        passes()
        d.sync(), s.sync()
        d.profile_enable(True)
        d.shadow_merge(s)
        d.composite(s, winner_base=n_a)
        prof = d.profile_read()
        d.profile_enable(False)
        if i >= a.warmup:
            k_merge.append(prof["k_shadow_merge"]["total_ms"] * 1e3)
            k_comp.append(prof["k_composite"]["total_ms"] * 1e3)
    med = float(np.median(k_merge))

    def full():
        sequence(d, s, n_a)
        d.sync()

    t_full = wall(full, a.warmup, a.reps)
    both = T.Scene(W, Hh, concat(A, B), texs, pipe, store_depth=True, auto_group=False)

    def one_scene():
        both.clear(), aim(both)
        both.render()
        both.sync()

    t_one = wall(one_scene, a.warmup, a.reps)
    full(), one_scene()
    equal = {"colour": bool(np.array_equal(d.get_frame_buffer(), both.get_frame_buffer())),
             "z": bool(np.array_equal(d.read_z_f32().view(np.uint32), both.read_z_f32().view(np.uint32))),
             "shadow": bool(np.array_equal(d.read_shadow_f32().view(np.uint32), both.read_shadow_f32().view(np.uint32)))}
    for q in (d, s, both):
        q.close()
    print(json.dumps({
        "width": W, "height": Hh, "pipeline": pipe, "reps": a.reps,
        "k_shadow_merge_us": round(med, 2), "k_shadow_merge_us_min_max": [round(min(k_merge), 2), round(max(k_merge), 2)],
        "k_composite_us": round(float(np.median(k_comp)), 2), "k_composite_us_min_max": [round(min(k_comp), 2), round(max(k_comp), 2)],
        "tiles_total": n_tiles, "tiles_left_on_src_flag": left, "tiles_taken_behind_dst_flag": taken, "tiles_elementwise": both_down,
        "share_of_tiles_left_on_a_flag": round(left / max(n_tiles, 1), 3), "pieces_changed": pieces,
        "bytes_read": b_read, "bytes_written": b_written,
        "GBps": round((b_read + b_written) / (med * 1e-6) / 1e9, 1),
        "share_of_copy_rate": round((b_read + b_written) / (med * 1e-6) / 1e12 / COPY_TBS, 3),
        "full_sequence_sync_us_med_min_max": t_full, "one_scene_of_concatenated_mesh_sync_us_med_min_max": t_one,
        "sequence_equals_concatenated_scene": equal}))


if __name__ == "__main__":
    main()
