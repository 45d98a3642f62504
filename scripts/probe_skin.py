"""Skinning at the flagship configuration (diablo, phong, 4096^2, frame groups):
python scripts/probe_skin.py [SIZE FRAMES REPEATS]

Step time of tr_scene_render_frames without a skin, with a skin but no palette, and of tr_scene_render_frames_skinned
under palettes of 2 and of 64 bones (four non-zero influences per position index).  Per form: the median and range of
REPEATS medians -- each the median of five timed calls of FRAMES frames, device idle on both sides -- and, from
tr_scene_profile_read over one more call, k_skin / k_setup / k_tile microseconds per frame.  For the skinned forms also
the bytes k_skin moves per frame (the rows read and written, the influence rows read; the palette, a few KB per
workgroup, not counted) and the rate that makes of its time.

With TR_LIBRARY pointing at a build of the parent commit (no skin entry points) only the first line is measured: that is
the parent's figure for DESIGN.md 7d."""
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import tiny_renderer_amd as T  # noqa: E402
from tests import helpers as H  # noqa: E402

size = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
frames = int(sys.argv[2]) if len(sys.argv) > 2 else 96
repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 5
pipe = "phong"

loaded = H.load_assets_py("diablo")
if loaded is None:
    mesh, texs = T.synthetic_scene()
    model = "synthetic-sphere"
else:
    mesh, texs = loaded
    model = "diablo"
params = np.zeros((frames, 12), np.float32)
for i in range(frames):
    params[i, 0:3] = H.light(0.01 * i)
    params[i, 3:6], params[i, 6:9], params[i, 9:12] = H.camera(0.02 * i)

has_skin = hasattr(T.load_library(), "tr_scene_render_frames_skinned")
n_pos = np.asarray(mesh["pos"], np.float32).reshape(-1, 3).shape[0]
n_rows = len(mesh["idx"])


def rig(n_bones):
    """Four non-zero influences per position index on scattered bones, weights summing to one."""
    i = np.arange(n_pos, dtype=np.int64)[:, None]
    j = np.arange(4, dtype=np.int64)[None, :]
    bones = ((i * 37 + j * 11) % n_bones).astype(np.uint32)
    w = (1.0 + ((i * 7 + j * 3) % 9)).astype(np.float64)
    return bones, (w / w.sum(1, keepdims=True)).astype(np.float32)


def palettes(n_bones):
    """A palette per frame: every bone a small rotation about y that moves from frame to frame."""
    out = np.empty((frames, n_bones, 24), np.float32)
    for i in range(frames):
        yaw = 0.02 * np.sin(0.1 * i + np.arange(n_bones))
        out[i] = T.rotation_instances(yaw, 0.0, 0.0, np.zeros((n_bones, 3)), 1.0)
    return out


def run(name, n_bones, pals):
    s = T.Scene(size, size, mesh, texs, pipe)
    if n_bones:
        s.set_skin(*rig(n_bones), n_bones=n_bones)
    kw = {} if pals is None else {"bone_palettes": pals}
    warm = {k: v[:32] for k, v in kw.items()}
    s.render_frames(params[:32], **warm)  # warm-up: slots, group sets
    s.sync()
    medians = []
    for _ in range(repeats):
        steps = []
        for _ in range(5):
            t0 = time.perf_counter()
            s.render_frames(params, **kw)
            s.sync()
            steps.append((time.perf_counter() - t0) / frames * 1e6)
        medians.append(float(np.median(steps)))
    s.profile_enable(True)
    s.render_frames(params, **kw)
    s.sync()
    prof = s.profile_read()
    s.profile_enable(False)
    s.close()
    per = {k: prof[k]["total_ms"] * 1e3 / max(prof[k]["frames"], 1) for k in ("k_skin", "k_setup", "k_tile") if k in prof and prof[k]["launches"]}
    line = "%-22s %s %s %d^2, %d frames per call: step %6.2f us (median of %d medians of 5 calls: %.2f .. %.2f) | per frame: %s" % (
        name, model, pipe, size, frames, float(np.median(medians)), repeats, min(medians), max(medians),
        "  ".join("%s %.2f us" % kv for kv in per.items()))
    if "k_skin" in per:
        nbytes = n_rows * 96 * 3
        line += " | k_skin moves %.2f MB per frame (%d rows, %d bones): %.0f GB/s" % (
            nbytes / 1e6, n_rows, n_bones, nbytes / (per["k_skin"] * 1e-6) / 1e9)
    print(line, flush=True)


print("library: %s (%s skin entry points)" % (T.library_path(), "with" if has_skin else "without"), flush=True)
run("no skin", 0, None)
if has_skin:
    run("skin, no palette", 2, None)
    run("palette, 2 bones", 2, palettes(2))
    run("palette, 64 bones", 64, palettes(64))
