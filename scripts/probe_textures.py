"""What replacing a texture costs: python scripts/probe_textures.py [--size 1024] [--reps 40]
k_pack_texels (HIP events on the scene's stream through tr_scene_profile_*, median [min, max] per call) for the colour
image (which = 0) and for the closure's normal map, on a one-word texel set (phong) and on a four-word set (specular),
from a size x size image in device memory -- beside a device-to-device copy of the same 3 * size * size bytes timed by
HIP events in the same run."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tiny_renderer_amd as T  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    import torch
    n = a.size
    mesh = T.synthetic_scene(n_lat=12, n_lon=24, tex_size=8)[0]
    rng = np.random.default_rng(1)
    texs = [rng.integers(0, 256, (n, n, 3), dtype=np.uint8) for _ in range(4)]
    src = torch.from_numpy(rng.integers(0, 256, 3 * n * n, dtype=np.uint8)).cuda()
    dst = torch.empty_like(src)
    torch.cuda.synchronize()
    out = {"size": n, "image_bytes": 3 * n * n}
    # the copy of the same bytes
    times = []
    for i in range(a.warmup + a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dst.copy_(src)
        e1.record()
        torch.cuda.synchronize()
        if i >= a.warmup:
            times.append(e0.elapsed_time(e1) * 1000.0)
    out["copy_us"] = [float(np.median(times)), float(min(times)), float(max(times))]
    for pipe, normal in (("phong", 1), ("specular", 1)):
        s = T.Scene(256, 256, mesh, texs, pipe, auto_group=False)
        for which in (0, normal):
            times = []
            for i in range(a.warmup + a.reps):
                s.profile_enable(True)
                s.set_texture_device(which, src.data_ptr(), n, n)
                s.sync()
                k = s.profile_read()["k_pack_texels"]
                s.profile_enable(False)
                if i >= a.warmup:
                    times.append(k["total_ms"] * 1000.0 / k["launches"])
            out["%s_which%d_us" % (pipe, which)] = [float(np.median(times)), float(min(times)), float(max(times))]
        out["%s_set_words" % pipe] = int(s.debug_texel_set().size)
        s.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
