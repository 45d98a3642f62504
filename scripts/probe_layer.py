"""What the layer stage costs: python scripts/probe_layer.py W H [-p DIR] [-s pipeline] [--reps R]
A scene of W x H (default model: the procedural scene) renders one frame and blends layers into it.
  * k_layer per case, out of place and in place (HIP events on the scene's stream through tr_scene_profile_*, median and
    range over the repetitions; the frame is rendered again before every repetition): a full-frame opaque rgb8 layer,
    NORMAL; a full-frame rgba8 layer with alpha; a full-frame MULTIPLY mask (layer_vignette); a full-frame backdrop,
    WHERE_UNDRAWN; a 480 x 270 inset at an odd offset; layer_from a second scene of the same size;
  * a device-to-device copy of the frame, k_grade out of place (a 17^3 identity table) and k_tile from the same run;
  * the 128 x 16 tiles by path for each case, a MODEL computed on the host from the frame's flags, not a counter:
    untouched (in place only), copied (out of place only), flagged base (zeros without a load), blended."""
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

HIP.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]


def census(flags, W, Hh, rect, in_place, dark=False):
    """Tiles by path for a layer on rect = (x, y, w, h), rows from the top; flags [tiles_y, tiles_x], rows from the bottom."""
    x, y, w, h = rect
    ty, tx = flags.shape
    hit = np.zeros_like(flags)
    x0, x1, r0, r1 = max(0, x), min(W, x + w), max(0, y), min(Hh, y + h)
    if x0 < x1 and r0 < r1:
        hit[(Hh - r1) // 16:(Hh - 1 - r0) // 16 + 1, x0 // 128:(x1 - 1) // 128 + 1] = True
    out = {"tiles": int(flags.size), "blended": int(hit.sum()), "blended_over_flagged_base": int((hit & flags).sum())}
    if in_place:
        out["untouched"] = int((~hit).sum()) + (int((hit & flags).sum()) if dark else 0)
    else:
        out["copied"] = int((~hit & ~flags).sum())
        out["zeros_on_flag"] = int((~hit & flags).sum())
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
    s = T.Scene(W, Hh, mesh, texs, a.pipeline)
    other = T.Scene(W, Hh, mesh, texs, a.pipeline)
    s.set_lut(T.lut_identity(17))
    drive(s), drive(other)
    fb = s.get_frame_buffer()
    other.get_frame_buffer()
    flags = flags_of(s)
    out = {"width": W, "height": Hh, "pipeline": a.pipeline, "model": a.path or "procedural", "reps": a.reps,
           "tiles_flagged": int(flags.sum()), "tiles": int(flags.size)}
    out["copy_of_the_frame_d2d"] = copy = time_copy(3 * W * Hh, a.reps, a.warmup)

    def device(img):
        p = C.c_void_p()
        assert HIP.hipMalloc(C.byref(p), img.nbytes) == 0
        assert HIP.hipMemcpy(p, img.ctypes.data_as(C.c_void_p), img.nbytes, 1) == 0
        return p.value, img.shape[1], img.shape[0], ("rgba8" if img.shape[2] == 4 else "rgb8")

    rng = np.random.default_rng(1)
    rgba = rng.integers(0, 256, (Hh, W, 4), dtype=np.uint8)
    iw, ih = min(480, W), min(270, Hh)
    cases = {
        "normal_rgb8_opaque": (device(rng.integers(0, 256, (Hh, W, 3), dtype=np.uint8)), (0, 0), dict()),
        "normal_rgba8_alpha": (device(rgba), (0, 0), dict()),
        "multiply_mask": (device(T.layer_vignette(W, Hh, 160)), (0, 0), dict(mode="multiply")),
        "backdrop_where_undrawn": (device(T.layer_gradient(W, Hh, (20, 40, 200), (240, 230, 220))), (0, 0), dict(where="undrawn")),
        "inset_480x270_odd_offset": (device(rng.integers(0, 256, (ih, iw, 3), dtype=np.uint8)), (min(37, W - 1), min(21, Hh - 1)), dict()),
        "layer_from_scene": (None, (0, 0), dict()),
    }
    target = C.c_void_p()
    assert HIP.hipMalloc(C.byref(target), 3 * W * Hh) == 0
    tile_us, grade_us = [], []
    for name, (img, (x, y), kw) in cases.items():
        for in_place in (False, True):
            us = []
            for i in range(a.warmup + a.reps):
                s.profile_enable(True)
                drive(s)
                dst = None if in_place else target.value
                if img is None:
                    s.layer_from(other, x, y, out=dst, **kw)
                else:
                    s.layer(img[0], x, y, out=dst, width=img[1], height=img[2], format=img[3], **kw)
                if name == "normal_rgb8_opaque" and not in_place:
                    s.grade(out=target.value)
                s.sync()
                prof = s.profile_read()
                s.profile_enable(False)
                if i >= a.warmup:
                    us.append(prof["k_layer"]["total_ms"] * 1e3)
                    tile_us.append(prof["k_tile"]["total_ms"] * 1e3)
                    if "k_grade" in prof:
                        grade_us.append(prof["k_grade"]["total_ms"] * 1e3)
            rect = (x, y, W, Hh) if img is None else (x, y, img[1], img[2])
            key = name + ("_in_place" if in_place else "_out_of_place")
            out[key] = dict(stat(us), copies=round(stat(us)["us"] / copy["us"], 2), tiles=census(flags, W, Hh, rect, in_place, kw.get("mode") == "multiply"))
    out["k_grade_out_of_place"], out["k_tile"] = stat(grade_us), stat(tile_us)
    # the last case ran in place: the frame is the layered one
    assert np.array_equal(s.get_frame_buffer(), T.layer_host(fb, other.get_frame_buffer())), "the layered frame is not the host rule's"
    s.close(), other.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
