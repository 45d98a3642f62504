"""Instanced vs replicated mesh at BASELINE.json configs[4] (diablo, 8 x 8 grid, -s specular, 8192^2):
python scripts/probe_instancing.py [SIZE GRID FRAMES]

The same frames rendered by a scene created from instanced_grid's replicated mesh (64 copies uploaded) and by a
scene of the mesh alone with grid_instances' table (tr_scene_set_instances).  Prints, per form: device memory
taken by the scene after create (and after the first frames), per-frame k_setup / k_bin / k_tile microseconds from
tr_scene_profile_read over one render_frames call, and the step time (wall clock of a timed render_frames call,
device idle on both sides).  The last frames are compared bit for bit (rgb, z)."""
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402

import tiny_renderer_amd as T  # noqa: E402
from tests import helpers as H  # noqa: E402

size = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
grid = int(sys.argv[2]) if len(sys.argv) > 2 else 8
frames = int(sys.argv[3]) if len(sys.argv) > 3 else 96
pipe = "specular"

loaded = H.load_assets_py("diablo")
if loaded is None:
    mesh, texs = T.synthetic_scene()
    model = "synthetic-sphere"
else:
    mesh, texs = loaded
    model = "diablo"
params = np.zeros((frames, 12), np.float32)
params[:, 0:3] = H.light(0.0)
params[:, 3:6], params[:, 6:9], params[:, 9:12] = H.camera(0.0)


def used_mib():
    free, total = torch.cuda.mem_get_info()
    return (total - free) / 2 ** 20


def run(form):
    torch.cuda.synchronize()
    base = used_mib()
    if form == "replicated":
        s = T.Scene(size, size, T.instanced_grid(mesh, grid), texs, pipe)
    else:
        s = T.Scene(size, size, mesh, texs, pipe, instances=T.grid_instances(grid))
    s.sync()
    at_create = used_mib() - base
    s.render_frames(params[:32])  # warm-up: frame slots, group sets
    s.sync()
    after_warm = used_mib() - base
    t0 = time.perf_counter()
    s.render_frames(params)
    s.sync()
    step_us = (time.perf_counter() - t0) / frames * 1e6
    s.profile_enable(True)
    s.render_frames(params)
    s.sync()
    prof = s.profile_read()
    s.profile_enable(False)
    per = {k: prof[k]["total_ms"] * 1e3 / max(prof[k]["frames"], 1) for k in ("k_setup", "k_bin", "k_tile") if k in prof}
    rgb, z = s.get_frame_buffer(), s.read_z_f32().view(np.uint32)
    s.close()
    print("%-10s %s x%d %s %d^2: memory after create %8.1f MiB, after warm-up %8.1f MiB | step %7.1f us | per frame "
          "(%d frames): %s" % (form, model, grid * grid, pipe, size, at_create, after_warm, step_us, frames,
                               "  ".join("%s %.1f us" % kv for kv in per.items())), flush=True)
    return rgb, z


rep = run("replicated")
ins = run("instanced")
print("bit-identical rgb: %s, z: %s" % (np.array_equal(rep[0], ins[0]), np.array_equal(rep[1], ins[1])), flush=True)
