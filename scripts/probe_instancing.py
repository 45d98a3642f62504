"""Instanced vs replicated mesh at BASELINE.json configs[4] (diablo, 8 x 8 grid, -s specular, 8192^2):
python scripts/probe_instancing.py [SIZE GRID FRAMES [FORMS [REPEATS]]]

The same frames rendered by a scene created from instanced_grid's replicated mesh (64 copies uploaded) and by a
scene of the mesh alone with grid_instances' table (tr_scene_set_instances).  Prints, per form: device memory
taken by the scene after create (and after the first frames), per-frame k_setup / k_bin / k_tile microseconds from
tr_scene_profile_read over one render_frames call, and the step time (wall clock of a timed render_frames call,
device idle on both sides; REPEATS such calls, default 1: their median and range).  The last frames are compared bit
for bit (rgb, z).  FORMS: a comma-separated choice of replicated, instanced, transformed (the same grid through a
transform table, tr_scene_set_instance_transforms: linear part identity / GRID, the grid's offsets -- bit-identical to
the other two) and yawed (cell k turned by k * 5 degrees about y: a different picture, timed only); default
replicated,instanced,transformed."""
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
forms = sys.argv[4].split(",") if len(sys.argv) > 4 else ["replicated", "instanced", "transformed"]
repeats = int(sys.argv[5]) if len(sys.argv) > 5 else 1
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
    elif form == "instanced":
        s = T.Scene(size, size, mesh, texs, pipe, instances=T.grid_instances(grid))
    else:
        g = T.grid_instances(grid)
        yaw = np.deg2rad(np.arange(grid * grid) * 5.0) if form == "yawed" else 0.0
        s = T.Scene(size, size, mesh, texs, pipe, instance_transforms=T.rotation_instances(yaw, 0.0, 0.0, g[:, 0:3], g[:, 3]))
    s.sync()
    at_create = used_mib() - base
    s.render_frames(params[:32])  # warm-up: frame slots, group sets
    s.sync()
    after_warm = used_mib() - base
    steps = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        s.render_frames(params)
        s.sync()
        steps.append((time.perf_counter() - t0) / frames * 1e6)
    step_us = float(np.median(steps))
    s.profile_enable(True)
    s.render_frames(params)
    s.sync()
    prof = s.profile_read()
    s.profile_enable(False)
    per = {k: prof[k]["total_ms"] * 1e3 / max(prof[k]["frames"], 1) for k in ("k_setup", "k_bin", "k_tile") if k in prof}
    rgb, z = s.get_frame_buffer(), s.read_z_f32().view(np.uint32)
    s.close()
    print("%-10s %s x%d %s %d^2: memory after create %8.1f MiB, after warm-up %8.1f MiB | step %7.1f us (%d calls: %.1f .. %.1f) | per "
          "frame (%d frames): %s" % (form, model, grid * grid, pipe, size, at_create, after_warm, step_us, repeats, min(steps),
                                     max(steps), frames,
                               "  ".join("%s %.1f us" % kv for kv in per.items())), flush=True)
    return rgb, z


out = {form: run(form) for form in forms}
same = [f for f in forms if f != "yawed"]
for f in same[1:]:
    print("%s against %s: bit-identical rgb: %s, z: %s" % (f, same[0], np.array_equal(out[same[0]][0], out[f][0]),
                                                         np.array_equal(out[same[0]][1], out[f][1])), flush=True)
