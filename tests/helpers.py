"""Test-side helpers: independent asset loaders (PIL for TGA, a small Python OBJ reader),
asset discovery and image dumps.  Independent of both the oracle and the product loaders so
that it can cross-check them."""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

TEX_FILES = ("texture.tga", "normal_map.tga", "normal_map_tangent.tga", "specular_map.tga")


FIXTURES = os.path.join(REPO, "tests", "golden", "assets")
_fixture_root = None


def asset_root():
    """Directory holding <model>/model.obj etc.: $TR_ASSETS or the git-ignored copy made by
    __graft_entry__.build() (assets/_ref), when present."""
    for p in (os.environ.get("TR_ASSETS"), os.path.join(REPO, "assets", "_ref")):
        if p and os.path.isdir(p):
            return p
    return None


def _real_asset_dir(name):
    root = asset_root()
    if root is None:
        return None
    d = os.path.join(root, name)
    return d if os.path.isfile(os.path.join(d, "model.obj")) else None


def fixture_maps():
    """The four maps of the committed fixtures: the procedural 1024^2 maps of synthetic_scene
    (diffuse, two normal maps, specular)."""
    import tiny_renderer_amd as T
    return T.synthetic_scene(n_lat=1, n_lon=1, tex_size=1024)[1]


def _fixture_dir(name):
    """tests/golden/assets/<name>.obj.xz (the model's own OBJ) with fixture_maps() written as
    RLE TGAs (by PIL), unpacked once per process into a temporary asset folder."""
    global _fixture_root
    import atexit
    import lzma
    import shutil
    import tempfile
    src = os.path.join(FIXTURES, name + ".obj.xz")
    if not os.path.isfile(src):
        return None
    if _fixture_root is None:
        _fixture_root = tempfile.mkdtemp(prefix="tr_assets_")
        atexit.register(shutil.rmtree, _fixture_root, True)
    d = os.path.join(_fixture_root, name)
    if not os.path.isfile(os.path.join(d, "model.obj")):
        from PIL import Image
        os.makedirs(d, exist_ok=True)
        for f, m in zip(TEX_FILES, fixture_maps()):
            Image.fromarray(m).save(os.path.join(d, f), compression="tga_rle")
        with lzma.open(src, "rb") as fi, open(os.path.join(d, "model.obj.part"), "wb") as fo:
            shutil.copyfileobj(fi, fo)
        os.replace(os.path.join(d, "model.obj.part"), os.path.join(d, "model.obj"))
    return d


def asset_source(name):
    """"assets" when the model's own folder is present, "fixture" when the committed fixture
    stands in for it (same OBJ, procedural maps), None when neither exists."""
    if _real_asset_dir(name):
        return "assets"
    return "fixture" if os.path.isfile(os.path.join(FIXTURES, name + ".obj.xz")) else None


def asset_dir(name):
    """<name>'s asset folder: the model's own (asset_root()) or else the fixture's."""
    return _real_asset_dir(name) or _fixture_dir(name)


def load_obj_py(path):
    """obj-rs `parse_obj` semantics for the subset the path uses: v / vt / vn / f with
    v/vt/vn triples; indices zero based; only the first three vertices of a face are used
    (scene.rs:224-226)."""
    pos, tex, nrm, idx = [], [], [], []
    with open(path, "r") as f:
        for line in f:
            parts = line.split()
            if not parts:
                continue
            if parts[0] == "v":
                pos.append([np.float32(x) for x in parts[1:4]])
            elif parts[0] == "vt":
                v = [np.float32(x) for x in parts[1:4]]
                while len(v) < 3:
                    v.append(np.float32(0.0))
                tex.append(v)
            elif parts[0] == "vn":
                nrm.append([np.float32(x) for x in parts[1:4]])
            elif parts[0] == "f":
                tri = []
                for tok in parts[1:4]:
                    a, b, c = tok.split("/")
                    tri += [int(a) - 1, int(b) - 1, int(c) - 1]
                idx.append(tri)
    return {"pos": np.array(pos, np.float32).reshape(-1, 3),
            "tex": np.array(tex, np.float32).reshape(-1, 3),
            "nrm": np.array(nrm, np.float32).reshape(-1, 3),
            "idx": np.array(idx, np.uint32).reshape(-1, 9)}


def load_tga_pil(path):
    """image::open(path)?.into_rgb8(): rgb8, row 0 = top."""
    from PIL import Image
    with Image.open(path) as im:
        return np.ascontiguousarray(np.array(im.convert("RGB"), dtype=np.uint8))


def load_assets_py(name):
    d = asset_dir(name)
    if d is None:
        return None
    mesh = load_obj_py(os.path.join(d, "model.obj"))
    texs = [load_tga_pil(os.path.join(d, f)) for f in TEX_FILES]
    return mesh, texs


def camera(angle):
    """app.rs:200-202"""
    a = np.float32(angle)
    return ([float(np.sin(a)), 0.0, float(np.cos(a))], [0.0, 0.0, 0.0], [0.0, 1.0, 0.0])


def light(angle):
    """app.rs:203-207"""
    a = np.float32(angle)
    return [float(np.sin(a)), 0.0, float(np.cos(a))]


TILE_W, TILE_H = 128, 16            # csrc/tr_types.h
LIT_PIXELS_PER_TEXEL = 16           # a scene takes the lit-texel path by itself from sixteen pixels per texel
INTERIOR_PIPES = ("default", "phong", "shadow")   # every pass has the interior form
LIT_PIPES = ("normal_map", "specular")            # ... only as FS_LIT, on the lit-texel path


def lit_path(W, Hh, texs, pipe):
    """Does a scene of `pipe` run the normal-map / specular closure once per texel (k_lit; the tile kernels then run
    FS_LIT)?  TR_LIT in the environment decides when it is set; else the frame has at least sixteen pixels per texel of
    the first image.  (The four images of every input here have one size, which the path needs.)"""
    if pipe not in LIT_PIPES:
        return False
    force = os.environ.get("TR_LIT")
    if force is not None:
        return int(force) != 0
    return W * Hh >= LIT_PIXELS_PER_TEXEL * texs[0].shape[0] * texs[0].shape[1]


SHARED_MAX_POLYGONS = 1 << 20      # the shared mode is honoured up to this many polygons per pass (mesh polygons x instances)


def expect_interior(W, Hh, pipe, waves, mode, band=None, lit=False, n_poly=None):
    """Must a fused launch of this scene have run the INTERIOR form of the tile kernels?  The documented rule
    (tr_scene_interior_tiles, include/tiny_renderer.h), restated -- not the launcher's code: the form exists
    for the four-wave column kernels (`waves`, `mode`: what the scene pins or is known to choose; anything else, 0
    included, says no) of the closures FS_DEFAULT, FS_PHONG, FS_LIT, FS_DEPTH and FS_SHADOW2, and runs when the width is
    a multiple of 128 and the band (output rows [row0, row1), row 0 = top; None: the whole frame) consists of whole
    16-row tile rows inside the frame -- tile rows count from the BOTTOM row of the frame.  The query says yes only when
    EVERY pass of the pipeline ran the form: occlusion's depth pass has it, its colour pass does not.
    lit: the scene is on the lit-texel path (lit_path above).
    n_poly: the polygons of a pass (mesh polygons x instances; None: few) -- beyond 2^20 of them a pinned or chosen shared
    mode (2) runs the column kernels, so it counts as mode 1 here."""
    if n_poly is not None and n_poly > SHARED_MAX_POLYGONS and mode == 2:
        mode = 1
    if waves != 4 or mode != 1 or W % TILE_W:
        return False
    r0, r1 = (0, Hh) if band is None else band
    if not (0 <= r0 < r1 <= Hh) or (Hh - r0) % TILE_H or (Hh - r1) % TILE_H:
        return False
    return pipe in INTERIOR_PIPES or (pipe in LIT_PIPES and bool(lit))


def save_png(path, rgb):
    from PIL import Image
    Image.fromarray(rgb).save(path)
