"""Generates tests/golden/oracle_hashes.json: sha256 fingerprints of the CPU oracle's outputs
(frame buffer, z bits, winner indices, shadow bits) for fixed scenes.

The reference ships no golden vectors and cannot be run here (Rust, no toolchain), so these are
regression pins of OUR restatement, not upstream data (PARITY UNPINNED, oracle/tr_oracle.h).
They let `-m "not gpu"` tests detect any drift of the oracle, and `-m gpu` tests check the GPU
against the same fingerprints without re-deriving them.

    python tests/golden/make_golden.py          # rewrites the json next to this script

Each model scene also has "fixture:" entries: the same scene with tests/golden/assets standing in for
the model's folder (its own OBJ, procedural maps; tests/helpers.py), which the tests use where the
model's assets are absent.
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)

PIPES = ("default", "phong", "normal_map", "specular", "darboux", "shadow", "occlusion")
# (scene, width, height, camera angle, light angle)
CASES = [("synthetic", 320, 240, 0.4, -0.7), ("synthetic", 257, 129, -1.2, 0.9),
         ("diablo", 800, 800, 0.0, 0.0), ("diablo", 640, 480, 0.7, -1.1), ("african_head", 800, 800, 0.0, 0.0)]


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:24]


def scene_inputs(name):
    import tiny_renderer_amd as T
    from tests import helpers as H
    if name == "synthetic":
        return T.synthetic_scene(n_lat=12, n_lon=24, tex_size=256)
    return H.load_assets_py(name)


def fingerprints(name, W, Hh, ca, la, pipe, inputs):
    from oracle import oracle as O
    from tests import helpers as H
    mesh, texs = inputs
    s = O.Scene(W, Hh, mesh, texs, pipe)
    s.clear()
    s.set_light_direction(H.light(la))
    s.set_camera(*H.camera(ca))
    err = s.render()
    out = {"err": err, "fb": sha(s.get_frame_buffer()), "z": sha(s.z_f32().view(np.uint32)),
           "winner": sha(s.winner_u32()), "accepts": s.stats()[-1 if pipe in ("shadow", "occlusion") else 0]["frag_accept"]}
    if pipe in ("shadow", "occlusion"):
        out["shadow"] = sha(s.shadow_f32().view(np.uint32))
    return out


def key(name, W, Hh, ca, la, pipe):
    return "%s/%dx%d/cam%+.2f/light%+.2f/%s" % (name, W, Hh, ca, la, pipe)


def fixture_key(name, W, Hh, ca, la, pipe):
    """The same scene with tests/golden/assets standing in for the model's folder (its OBJ, procedural maps)."""
    return "fixture:" + key(name, W, Hh, ca, la, pipe)


def gold_key(name, W, Hh, ca, la, pipe):
    """Key of what scene_inputs(name) renders here: the model's own assets, or the fixture standing in for them."""
    from tests import helpers as H
    k = fixture_key if name != "synthetic" and H.asset_source(name) == "fixture" else key
    return k(name, W, Hh, ca, la, pipe)


# the fingerprints that depend on the geometry alone: the fixture's equal the model's own
GEOMETRY_FIELDS = ("err", "z", "winner", "accepts", "shadow")


def fixture_inputs(name):
    from tests import helpers as H
    d = H._fixture_dir(name)
    return None if d is None else (H.load_obj_py(os.path.join(d, "model.obj")), H.fixture_maps())


def main():
    # (merged into what is there: a box without the models' own assets keeps their entries)
    path = os.path.join(HERE, "oracle_hashes.json")
    res = json.load(open(path)) if os.path.exists(path) else {}
    for name, W, Hh, ca, la in CASES:
        inputs = scene_inputs(name)
        if inputs is None:
            print("skipping %s: assets not available" % name)
            continue
        fixture = fixture_inputs(name) if name != "synthetic" else None
        for pipe in PIPES:
            res[gold_key(name, W, Hh, ca, la, pipe)] = fingerprints(name, W, Hh, ca, la, pipe, inputs)
            if fixture is not None:
                res[fixture_key(name, W, Hh, ca, la, pipe)] = fingerprints(name, W, Hh, ca, la, pipe, fixture)
    json.dump(res, open(path, "w"), indent=1, sort_keys=True)
    print("wrote %d fingerprints to %s" % (len(res), path))


if __name__ == "__main__":
    main()
