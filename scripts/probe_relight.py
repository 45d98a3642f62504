"""What relighting costs: python scripts/probe_relight.py W H [-p DIR] [-s pipeline] [--reps N]
A scene (default model: the procedural scene) renders one frame, and 1, 4 and 8 lights of mixed kinds are laid on it, with
and without a highlight, out of place into device memory and in place:
  * k_relight alone and k_tile for scale, median and range over the repetitions; the frame is rendered again before
    every repetition, so that every in-place call finds the same frame, depth and flags; the scene stores its depth, so
    no call repeats a pass.  k_relight has no entry in tr_scene_profile_* (its table of names is full), so the scene runs
    on a stream of the probe's and the call is bracketed by two HIP events of the probe's on that stream, behind a 1 GB
    memset that keeps the stream busy while the host issues the three: the events then time the kernel, not the host;
  * beside it, in the same run: a device-to-device copy of the frame (hipMemcpyAsync between two device buffers, HIP
    events), k_projector plain with a 1024 x 1024 image (the same events), and k_outline at radius 0 through the profile;
  * the tiles by path -- nothing drawn (untouched in place, copied out of place), colour flag up, staged and lit -- and
    the share of drawn pixels that have a normal on a strip of the frame: a MODEL computed on the host from the frame's
    depth (tr_relight_normals_host over the strip read back), not a counter."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tiny_renderer_amd as T  # noqa: E402
from probe_bloom import HIP, drive, colour_flags, time_copy  # noqa: E402
from probe_convolve import timed  # noqa: E402
from probe_projector import timed_events, device_copy, BUSY, LIGHT, CAM, SIDE  # noqa: E402


def lights(n, specular):
    s = 0.5 if specular else 0.0
    base = [T.light_point([1.5, 1.0, 2.0], (255, 120, 40), 1.5, 0.3, s, 4), T.light_spot([-1.5, 1.5, 2.5], [0.0, 0.0, 0.0], 8.0, 25.0, (60, 140, 255), 2.5, 0.1, s, 6),
            T.light_directional([0.3, 1.0, 0.4], (200, 255, 200), 0.5, s, 5), T.light_point([0.0, -1.0, 1.5], (255, 0, 255), 0.8, 1.0, s, 3),
            T.light_spot([0.5, 0.2, 3.0], [0.3, 0.0, 0.0], 2.0, 6.0, (255, 255, 255), 6.0, 0.0, s, 10), T.light_directional([-1.0, 0.2, 0.6], (30, 30, 120), 1.0, s, 2),
            T.light_point([2.0, 2.0, 2.0], (90, 200, 90), 20.0, 2.0, s, 7), T.light_spot([0.0, 2.5, 0.5], [0.0, 0.0, 0.2], 20.0, 60.0, (255, 220, 160), 1.0, 0.05, s, 1)]
    return base[:n]


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("width", type=int)
    ap.add_argument("height", type=int)
    ap.add_argument("-p", dest="path", default=None)
    ap.add_argument("-s", dest="pipeline", default="phong")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    W, Hh, N = a.width, a.height, 1024
    mesh, texs = T.load_assets(a.path) if a.path else T.synthetic_scene()
    stream, busy = C.c_void_p(), C.c_void_p()
    assert HIP.hipStreamCreateWithFlags(C.byref(stream), 1) == 0 and HIP.hipMalloc(C.byref(busy), BUSY) == 0   # (1: non-blocking)
    s = T.Scene(W, Hh, mesh, texs, a.pipeline, store_depth=True, stream=stream.value)
    drive(s)
    cflags = colour_flags(s)
    z = s.read_z_f32()
    drawn = z.view(np.uint32) != 0xFF7FFFFF
    ty, tx = cflags.shape
    drawn_tiles = np.array([[drawn[16 * j:16 * j + 16, 128 * i:128 * i + 128].any() for i in range(tx)] for j in range(ty)])
    st, view = T.prepare_uniforms(2, W, Hh, LIGHT, *CAM)
    assert st == 0
    eye = [CAM[0][i] + 5.0 * float(view.camera_direction[i]) for i in range(3)]
    # the share of the drawn pixels with a normal, on a strip of the frame (its row 0 is frame row y = rows.start)
    rows = slice(Hh // 2 - min(Hh // 2, 32), Hh // 2 + min(Hh - Hh // 2, 32))
    uu = np.array(list(view.i_vpmv), np.float64).reshape(4, 4).T.copy()
    uu[:, 3] += uu[:, 1] * rows.start
    valid = T.relight_normals_host(z[rows], T.relight_params(uu, eye))[1]
    dev = C.c_void_p()
    assert HIP.hipMalloc(C.byref(dev), W * Hh * 3) == 0
    out = {"width": W, "height": Hh, "pipeline": a.pipeline, "reps": a.reps, "drawn_share": round(float(drawn.mean()), 4),
           "normal_share_of_drawn_in_the_middle_strip": round(float(valid.sum()) / max(int(drawn[rows].sum()), 1), 4),
           "tiles": int(cflags.size), "tiles_nothing_drawn": int((~drawn_tiles).sum()), "tiles_colour_flag_up": int(cflags.sum()),
           "tiles_staged_and_lit": int(drawn_tiles.sum()), "frame_copy_d2d": time_copy(W * Hh * 3, a.reps, a.warmup), "cases": []}
    for n in (1, 4, 8):
        for specular in (False, True):
            ls = lights(n, specular)
            p = T.relight_params(view, eye, (8, 8, 8), "add")
            case = {"lights": n, "highlight": specular}
            for mode in ("out_of_place", "in_place"):
                target = None if mode == "in_place" else dev.value
                k, tile = timed_events(s, stream, busy, lambda: s.relight(p, ls, out=target), a.reps, a.warmup)
                case[mode] = {"k_relight": k, "k_tile": tile}
            out["cases"].append(case)
    # beside it: k_projector plain (the same events) and k_outline at radius 0 (the profile)
    out["beside"] = {}
    st2, proj = T.prepare_uniforms(0, N, N, LIGHT, *SIDE)
    assert st2 == 0
    img = T.layer_checker(N, N, N // 16, (255, 240, 200), (40, 40, 90))
    img = np.concatenate([img, np.full((N, N, 1), 255, np.uint8)], axis=2)
    image = device_copy(img)
    pp = T.projector_params(T.projector_matrix(view, proj), N, N, 4, "add", 256)
    op = T.outline_params(radius=0)
    for mode in ("out_of_place", "in_place"):
        target = None if mode == "in_place" else dev.value
        k, _ = timed_events(s, stream, busy, lambda: s.projector(pp, image.value, None, out=target, width=N, height=N, format="rgba8"), a.reps, a.warmup)
        out["beside"][mode] = {"k_projector_plain": k}
        k, _ = timed(s, lambda: s.outline(op, out=target), "k_outline", a.reps, a.warmup)
        out["beside"][mode]["k_outline_radius_0"] = k
    s.close()
    HIP.hipFree(dev), HIP.hipFree(image), HIP.hipFree(busy), HIP.hipStreamDestroy(stream)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
