"""What the projector costs: python scripts/probe_projector.py W H [--image N] [-p DIR] [-s pipeline] [--reps N]
A scene (default model: the procedural scene) renders one frame, and an N x N rgba8 image (default 1024) is cast on it
from a second camera to the side -- plain, with a second scene of N x N rendered from that camera as occluder (OCCLUDE),
and with the filtered shadow (OCCLUDE | SOFT) --, out of place into device memory and in place:
  * k_projector alone and k_tile for scale, median and range over the repetitions; the frame is rendered again before
    every repetition, so that every in-place call finds the same frame, depth and flags; both scenes store their depth, so
    no call repeats a pass.  k_projector has no entry in tr_scene_profile_* (its table of names is full), so the scene runs
    on a stream of the probe's and the call is bracketed by two HIP events of the probe's on that stream, behind a 1 GB
    memset that keeps the stream busy while the host issues the three: the events then time the kernel, not the host;
  * beside it, in the same run: a device-to-device copy of the frame (hipMemcpyAsync between two device buffers, HIP
    events), k_layer with a full-frame WHERE_DRAWN layer -- the same colour and depth traffic with a streamed image instead
    of a gathered one --, and k_ramp through a fog table;
  * the tiles by path -- nothing drawn (untouched in place, copied out of place), colour flag up, read whole -- and the
    share of drawn pixels the image reaches: a MODEL computed on the host from the frame's depth by the rule's own
    restatement in Python (tr_projector_host over the frame read back), not a counter."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tiny_renderer_amd as T  # noqa: E402
from probe_bloom import HIP, drive, colour_flags, time_copy  # noqa: E402
from probe_convolve import timed, stats  # noqa: E402

BUSY = 1 << 30
HIP.hipMemsetAsync.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]
HIP.hipStreamCreateWithFlags.argtypes = [C.POINTER(C.c_void_p), C.c_uint]
HIP.hipStreamDestroy.argtypes = [C.c_void_p]


def timed_events(s, stream, busy, call, reps, warmup):
    """Median [min, max] microseconds between two events around call() on the scene's stream, and of k_tile from the
    profile, over reps calls, the frame rendered before each."""
    e0, e1 = C.c_void_p(), C.c_void_p()
    assert HIP.hipEventCreate(C.byref(e0)) == 0 and HIP.hipEventCreate(C.byref(e1)) == 0
    k_us, tile_us = [], []
    for i in range(warmup + reps):
        s.profile_enable(True)
        drive(s)
        s.sync()
        assert HIP.hipMemsetAsync(busy, 0, BUSY, stream) == 0
        assert HIP.hipEventRecord(e0, stream) == 0
        call()
        assert HIP.hipEventRecord(e1, stream) == 0
        s.sync()
        assert HIP.hipEventSynchronize(e1) == 0
        ms = C.c_float()
        assert HIP.hipEventElapsedTime(C.byref(ms), e0, e1) == 0
        prof = s.profile_read()
        s.profile_enable(False)
        if i >= warmup:
            k_us.append(ms.value * 1e3)
            tile_us.append(prof["k_tile"]["total_ms"] * 1e3)
    HIP.hipEventDestroy(e0), HIP.hipEventDestroy(e1)
    return stats(k_us), stats(tile_us)


LIGHT, CAM, SIDE = [0.5, 0.0, 0.8], ([0.3, 0.0, 0.95], [0.0, 0.0, 0.0], [0.0, 1.0, 0.0]), ([0.95, 0.0, 0.3], [0.0, 0.0, 0.0], [0.0, 1.0, 0.0])


def device_copy(array):
    p = C.c_void_p()
    assert HIP.hipMalloc(C.byref(p), array.nbytes) == 0
    assert HIP.hipMemcpy(p, array.ctypes.data_as(C.c_void_p), array.nbytes, 1) == 0
    return p


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("width", type=int)
    ap.add_argument("height", type=int)
    ap.add_argument("--image", type=int, default=1024)
    ap.add_argument("-p", dest="path", default=None)
    ap.add_argument("-s", dest="pipeline", default="phong")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    W, Hh, N = a.width, a.height, a.image
    mesh, texs = T.load_assets(a.path) if a.path else T.synthetic_scene()
    stream, busy = C.c_void_p(), C.c_void_p()
    assert HIP.hipStreamCreateWithFlags(C.byref(stream), 1) == 0 and HIP.hipMalloc(C.byref(busy), BUSY) == 0   # (1: non-blocking)
    s = T.Scene(W, Hh, mesh, texs, a.pipeline, store_depth=True, stream=stream.value)
    occ = T.Scene(N, N, mesh, texs, a.pipeline, store_depth=True)
    drive(s)
    occ.clear(), occ.set_light_direction(LIGHT), occ.set_camera(*SIDE), occ.render()
    assert occ.sync() == 0
    cflags = colour_flags(s)
    z = s.read_z_f32()
    drawn = z.view(np.uint32) != 0xFF7FFFFF
    ty, tx = cflags.shape
    drawn_tiles = np.array([[drawn[16 * j:16 * j + 16, 128 * i:128 * i + 128].any() for i in range(tx)] for j in range(ty)])
    st, view = T.prepare_uniforms(2, W, Hh, LIGHT, *CAM)
    st2, proj = T.prepare_uniforms(0, N, N, LIGHT, *SIDE)
    assert st == 0 and st2 == 0
    m = T.projector_matrix(view, proj)
    img = T.layer_checker(N, N, max(N // 16, 1), (255, 240, 200), (40, 40, 90))
    img = np.concatenate([img, np.full((N, N, 1), 255, np.uint8)], axis=2)
    image = device_copy(img)
    # the share of the drawn pixels the image reaches, on a strip of the frame (the host rule over all of 4096^2 takes minutes)
    rows = slice(Hh // 2 - min(Hh // 2, 32), Hh // 2 + min(Hh - Hh // 2, 32))
    strip_fb = np.zeros((rows.stop - rows.start, W, 3), np.uint8)
    mm = m.reshape(4, 4).T.astype(np.float64).copy()
    mm[:, 3] += mm[:, 1] * rows.start       # (the strip's row 0 is frame row y = rows.start)
    lit = T.projector_host(strip_fb, z[rows], T.projector_params(mm, N, N, 4, "normal"), img)
    reached = (lit != 0).any(2)[::-1] & drawn[rows]
    dev = C.c_void_p()
    assert HIP.hipMalloc(C.byref(dev), W * Hh * 3) == 0
    out = {"width": W, "height": Hh, "image": N, "pipeline": a.pipeline, "reps": a.reps, "drawn_share": round(float(drawn.mean()), 4),
           "reached_share_of_drawn_in_the_middle_strip": round(float(reached.sum()) / max(int(drawn[rows].sum()), 1), 4),
           "tiles": int(cflags.size), "tiles_nothing_drawn": int((~drawn_tiles).sum()), "tiles_colour_flag_up": int(cflags.sum()),
           "tiles_read_whole": int((~cflags).sum()), "frame_copy_d2d": time_copy(W * Hh * 3, a.reps, a.warmup), "cases": []}
    for label, occlude, soft in (("plain", False, False), ("OCCLUDE", True, False), ("OCCLUDE | SOFT", True, True)):
        p = T.projector_params(m, N, N, 4, "add", 256, occlude, soft, 2.0)
        case = {"variant": label}
        for mode in ("out_of_place", "in_place"):
            target = None if mode == "in_place" else dev.value
            k, tile = timed_events(s, stream, busy, lambda: s.projector(p, image.value, occ if occlude else None, out=target, width=N, height=N, format="rgba8"),
                                   a.reps, a.warmup)
            case[mode] = {"k_projector": k, "k_tile": tile}
        out["cases"].append(case)
    # beside it: k_layer with a full-frame WHERE_DRAWN layer in device memory, and k_ramp through a fog table
    out["beside"] = {}
    near, far = (float(z[drawn].max()), float(z[drawn].min())) if drawn.any() else (1.0, 0.0)
    s.set_ramp(T.ramp_fog((200, 210, 230), 256, "exp", 3.0))
    rp = T.ramp_params(*T.ramp_span(near, far if far != near else near - 1.0, 256))
    back = device_copy(T.layer_gradient(W, Hh, (20, 40, 200), (240, 230, 220))) if W <= 8192 and Hh <= 8192 else None
    for mode in ("out_of_place", "in_place"):
        target = None if mode == "in_place" else dev.value
        k, _ = timed(s, lambda: s.ramp(None, None, params=rp, out=target), "k_ramp", a.reps, a.warmup)
        out["beside"][mode] = {"k_ramp": k}
        if back is not None:
            k, _ = timed(s, lambda: s.layer(back.value, where="drawn", mode="add", out=target, width=W, height=Hh), "k_layer", a.reps, a.warmup)
            out["beside"][mode]["k_layer_where_drawn"] = k
    if back is not None:
        HIP.hipFree(back)
    s.close(), occ.close()
    HIP.hipFree(dev), HIP.hipFree(image), HIP.hipFree(busy), HIP.hipStreamDestroy(stream)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
