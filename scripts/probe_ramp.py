"""What a depth ramp costs: python scripts/probe_ramp.py W H [-p DIR] [-s pipeline] [--reps N]
A scene (default model: the procedural scene) renders one frame and ramps it, out of place into device memory and in
place, through a fog table (n = 256), the largest table (n = 1024) and a fog table under REPEAT, each with an `undrawn`
alpha of 0 and of 255:
  * k_ramp alone and k_tile for scale (HIP events on the scene's stream through tr_scene_profile_*, median and range over
    the repetitions; the frame is rendered again before every repetition, so that every in-place call finds the same
    frame, depth and flags);
  * beside it, in the same run: a device-to-device copy of the frame (hipMemcpyAsync between two device buffers, HIP
    events), k_grade (a 17^3 table), and k_layer with a frame-sized WHERE_UNDRAWN backdrop -- the stage that moves nearly
    the same bytes: colour in and out and depth, and the layer's image on top;
  * the tiles by path -- nothing drawn (no depth loaded; untouched in place where undrawn's alpha is 0), colour flag up
    (no colour loaded), read whole -- a MODEL computed on the host from the frame's flags by the kernel's own rule, not a
    counter.  The z flags are taken from the depth read back: a tile counts as empty where no pixel of it is drawn."""
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


def census(cflags, drawn_tiles, undrawn_alpha):
    """Tiles by path of one in-place k_ramp launch under NORMAL: cflags and drawn_tiles [ty, tx], y up."""
    empty = ~drawn_tiles
    return {"tiles": int(cflags.size), "tiles_nothing_drawn": int(empty.sum()), "tiles_untouched_in_place": int(empty.sum()) if undrawn_alpha == 0 else 0,
            "tiles_colour_flag_up": int(cflags.sum()), "tiles_read_whole": int((~cflags).sum())}


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
    z = s.read_z_f32()
    drawn = z.view(np.uint32) != 0xFF7FFFFF
    ty, tx = cflags.shape
    drawn_tiles = np.array([[drawn[16 * j:16 * j + 16, 128 * i:128 * i + 128].any() for i in range(tx)] for j in range(ty)])
    near, far = (float(z[drawn].max()), float(z[drawn].min())) if drawn.any() else (1.0, 0.0)
    dev = C.c_void_p()
    assert HIP.hipMalloc(C.byref(dev), W * Hh * 3) == 0
    out = {"width": W, "height": Hh, "pipeline": a.pipeline, "reps": a.reps, "drawn_share": round(float(drawn.mean()), 4),
           "frame_copy_d2d": time_copy(W * Hh * 3, a.reps, a.warmup), "cases": []}
    fog = T.ramp_fog((200, 210, 230), 256, "exp", 3.0)
    big = T.ramp_fog((200, 210, 230), 1024)
    for label, tab, repeat in (("fog n=256", fog, False), ("largest n=1024", big, False), ("fog n=256 REPEAT", fog, True)):
        n = tab.shape[0]
        z0, scale = T.ramp_span(near, far if far != near else near - 1.0, n)
        if repeat:
            scale = np.float32(scale * 4)      # four periods over the span
        s.set_ramp(tab)
        for alpha in (0, 255):
            case = {"table": label, "undrawn_alpha": alpha}
            case.update(census(cflags, drawn_tiles, alpha))
            p = T.ramp_params(z0, scale, undrawn=(200, 210, 230, alpha), repeat=repeat)
            for mode in ("out_of_place", "in_place"):
                k, tile = timed(s, lambda: s.ramp(None, None, params=p, out=None if mode == "in_place" else dev.value), "k_ramp", a.reps, a.warmup)
                case[mode] = {"k_ramp": k, "k_tile": tile}
            out["cases"].append(case)
    # beside it: k_grade and k_layer with a frame-sized WHERE_UNDRAWN backdrop in device memory
    s.set_lut(T.lut_identity(17))
    out["beside"] = {}
    back = None
    if W <= 8192 and Hh <= 8192:
        img = T.layer_gradient(W, Hh, (20, 40, 200), (240, 230, 220))
        back = C.c_void_p()
        assert HIP.hipMalloc(C.byref(back), img.nbytes) == 0
        assert HIP.hipMemcpy(back, img.ctypes.data_as(C.c_void_p), img.nbytes, 1) == 0
    for mode in ("out_of_place", "in_place"):
        target = None if mode == "in_place" else dev.value
        k, _ = timed(s, lambda: s.grade(target), "k_grade", a.reps, a.warmup)
        out["beside"][mode] = {"k_grade": k}
        if back is not None:
            k, _ = timed(s, lambda: s.layer(back.value, where="undrawn", out=target, width=W, height=Hh), "k_layer", a.reps, a.warmup)
            out["beside"][mode]["k_layer_where_undrawn"] = k
    if back is not None:
        HIP.hipFree(back)
    s.close()
    HIP.hipFree(dev)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
