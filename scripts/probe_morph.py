"""Morph targets at the flagship configuration (diablo, phong, 4096^2, frame groups):
python scripts/probe_morph.py [SIZE FRAMES REPEATS [TARGETS]]

Step time of tr_scene_render_frames without a pose and of tr_scene_render_frames_morphed under two poses of TARGETS
(default 8) targets: 2 non-zero weights, and all non-zero.  Per form: the median and range of REPEATS medians -- each the
median of five timed calls of FRAMES frames, device idle on both sides -- and, from tr_scene_profile_read over one more
call, k_morph / k_setup / k_tile microseconds per frame.  For the posed forms also the bytes k_morph reads and writes per
frame (base rows + one set of delta rows per non-zero weight + posed rows) and the rate that makes of its time.

With TR_LIBRARY pointing at a build of the parent commit (no morph entry points) only the first line is measured: that is
the parent's figure for DESIGN.md 7c."""
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
n_targets = int(sys.argv[4]) if len(sys.argv) > 4 else 8
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

has_morph = hasattr(T.load_library(), "tr_scene_render_frames_morphed")
pos = np.asarray(mesh["pos"], np.float32).reshape(-1, 3)
nrm = np.asarray(mesh["nrm"], np.float32).reshape(-1, 3)
rs = np.random.RandomState(3)
dpos = (rs.standard_normal((n_targets,) + pos.shape) * 0.01).astype(np.float32)
dnrm = (rs.standard_normal((n_targets,) + nrm.shape) * 0.05).astype(np.float32)
n_rows = len(mesh["idx"])


def poses(nonzero):
    """A pose per frame with `nonzero` non-zero weights (the first ones), moving from frame to frame."""
    w = np.zeros((frames, n_targets), np.float32)
    for i in range(frames):
        w[i, :nonzero] = 0.25 + 0.5 * abs(((i + np.arange(nonzero)) % 16) / 8.0 - 1.0)
    return w


def run(name, weights):
    s = T.Scene(size, size, mesh, texs, pipe)
    if weights is not None:
        s.set_morph_targets(dpos, dnrm)
    kw = {} if weights is None else {"morph_weights": weights}
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
    per = {k: prof[k]["total_ms"] * 1e3 / max(prof[k]["frames"], 1) for k in ("k_morph", "k_setup", "k_tile") if k in prof and prof[k]["launches"]}
    line = "%-22s %s %s %d^2, %d frames per call: step %6.2f us (median of %d medians of 5 calls: %.2f .. %.2f) | per frame: %s" % (
        name, model, pipe, size, frames, float(np.median(medians)), repeats, min(medians), max(medians),
        "  ".join("%s %.2f us" % kv for kv in per.items()))
    if weights is not None and "k_morph" in per:
        nz = int((weights[0] != 0).sum())
        nbytes = n_rows * 96 * (2 + nz)
        line += " | k_morph moves %.2f MB per frame (%d rows, %d non-zero of %d): %.0f GB/s" % (
            nbytes / 1e6, n_rows, nz, n_targets, nbytes / (per["k_morph"] * 1e-6) / 1e9)
    print(line, flush=True)


print("library: %s (%s morph entry points)" % (T.library_path(), "with" if has_morph else "without"), flush=True)
run("no pose", None)
if has_morph:
    run("pose, 2 of %d non-zero" % n_targets, poses(2))
    run("pose, all %d non-zero" % n_targets, poses(n_targets))
