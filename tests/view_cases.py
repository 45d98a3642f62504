"""The view / light / texture-shape cases that tests/test_view_space_cpu.py (oracle against the numpy restatement and the
host emulation) and tests/test_view_space_parity.py (oracle against the GPU) share.  Pure numpy, deterministic, importable
without any of the libraries.

The reference's projection is fixed (coef = -1/5, shader.rs:204): with z_cam the coordinate of a point along the view axis
(new_z = normalize(look_from - look_at), measured from look_from) its homogeneous w is 1 - z_cam / 5.  The helpers of
tests/helpers.py keep every vertex at w in [1.0, 1.4]; the cameras below leave that corner on purpose."""
import numpy as np

F = np.float32

# name -> (look_from, look_at, up).  The models these are used with have a radius below 1 around the origin.
CAMERAS = {
    "elevated": ([0.5, 0.8, 0.9], [0.1, -0.1, 0.0], [0.0, 1.0, 0.0]),        # off-axis, look_at off the origin, distance 1.3
    "tilted_up": ([0.0, 0.2, 2.5], [0.0, 0.0, 0.0], [0.3, 0.9, 0.1]),        # up neither unit nor orthogonal to the view axis
    "inside": ([0.0, 0.0, 0.3], [0.0, 0.0, 0.0], [0.0, 1.0, 0.0]),           # distance 0.3: the camera is inside the mesh
    "distance3": ([1.2, 0.9, 2.6], [0.0, 0.0, 0.0], [0.0, 1.0, 0.0]),        # distance 3.0
    "distance10": ([3.0, 1.0, 9.0], [0.0, 0.0, 0.0], [0.0, 2.0, 0.0]),       # distance 9.5, up of length 2
    "off_origin": ([0.9, -0.4, 1.1], [0.35, 0.3, -0.25], [0.0, 1.0, 0.0]),   # look_at 0.52 from the origin, seen from below
    "rolled": ([-0.7, 0.3, -0.8], [0.0, 0.0, 0.0], [0.8, 0.1, -0.3]),        # from behind, the picture rolled by ~90 degrees
    "from_below": ([0.1, -1.6, 0.2], [0.0, 0.0, 0.0], [0.0, 0.0, -1.0]),     # view axis close to -y: up cannot be y
    "behind7": ([0.0, 0.0, -7.0], [0.0, 0.0, -8.0], [0.0, 1.0, 0.0]),        # looks AWAY from the mesh: w < 0 everywhere
    "straddle": ([0.0, 0.0, -4.6], [0.0, 0.0, -5.6], [0.0, 1.0, 0.0]),       # w = (0.4 - z) / 5 changes sign across the mesh
    "straddle_w0": ([0.0, 0.0, -5.0], [0.0, 0.0, -6.0], [0.0, 1.0, 0.0]),    # w = -z / 5: EXACTLY 0 at a vertex with z = 0
    "straddle_moved": ([0.013, 0.007, -4.913], [0.013, 0.007, -5.913], [0.0, 1.0, 0.0]),  # the same, no vertex at w == 0
}
# The cameras whose frame must be defined upstream in every single-pass pipeline (test_view_space_cpu.py asserts it):
# every one but "straddle_w0", whose plane w = 0 passes through the equator vertices of the test spheres (the reference's
# Point3::from_homogeneous(..).unwrap() panics there).
DEFINED_CAMERAS = tuple(k for k in CAMERAS if k != "straddle_w0")
DIABLO_CAMERAS = ("elevated", "distance3", "inside", "behind7")

# 3-D light directions, lengths 0.25 ... 6 (the depth pass of shadow / occlusion takes the light as its look_from:
# the length is that camera's distance)
LIGHTS = {
    "short": [0.1, 0.2, 0.12],           # length 0.255: second view of the texture-shape cases
    "unit3d": [0.3, 0.7, 0.6],           # 0.97
    "down": [0.4, -0.8, 0.5],            # 1.02, negative y: third view of the uv-edge cases
    "back": [0.5, 0.6, -1.2],            # 1.43, negative z: second view of the uv-edge cases
    "long": [1.5, -2.0, 2.5],            # 3.5, negative y: second view of the near-w soups
    "longest": [-3.0, 4.0, -3.3],        # 5.99
}
# The two lights every camera x pipeline case uses.  Shadow and occlusion look their shadow buffer up at the position the
# LIGHT's camera projects a fragment to, and the reference panics when that leaves the buffer: a light closer than the
# camera magnifies the mesh beyond the frame, and so does a mesh behind the light's camera.  "unit3d" and "longest" keep
# those lookups inside for every designed camera but "straddle_moved" (test_view_space_cpu.py asserts which cases are
# defined; "long" and "down" leave the buffer under the behind-camera views).
CASE_LIGHTS = ("unit3d", "longest")
# occlusion alone: Rotation3::rotation_between((0, 0, 1), light) does not exist for a light along -z and the reference's
# unwrap() panics (shader.rs:921) whatever the camera -- the one designed SINGULAR case
ANTIPARALLEL_LIGHT = [0.0, 0.0, -2.0]


def view_row(light, camera):
    """One row of render_frames' table: light, look_from, look_at, up."""
    f, a, u = camera
    return np.array(list(light) + list(f) + list(a) + list(u), F)


# an ordinary view: what a scene renders after an undefined one, to show that it is still usable
GOOD_VIEW = view_row([0.5, 0.0, 0.8], ([0.3, 0.0, 0.95], [0.0, 0.0, 0.0], [0.0, 1.0, 0.0]))


def case_view(camera_name, light_name):
    return view_row(LIGHTS[light_name], CAMERAS[camera_name])


NEAR_W_CAMERA = ([0.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.0, 1.0, 0.0])   # z_cam = z of the vertex: w = 1 - z / 5
NEAR_W_LIGHT = [0.2, 0.3, 1.0]
# seven soups that are defined upstream and one (4) in which a vertex lands on w == 0 exactly
NEAR_W_SEEDS = (1, 2, 3, 4, 5, 6, 7, 8)


def near_w_soup(seed, n=60):
    """n polygons for NEAR_W_CAMERA (at the origin, looking down -z): x, y in [-1, 1], z in [-3, 4.5] (w from 1.6 down to
    0.1), and in every third polygon one vertex at z = nextafter(5, 0) or nextafter(5, 10) (w = +-1 ulp around 0: raster
    coordinates of +-1e6 ... +-1e7 and beyond), in every other third one vertex at 5 +- 1e-4 and one at 6.5 (w = -0.3).
    Returns (mesh, textures)."""
    rng = np.random.default_rng(seed)
    pts = np.zeros((n, 3, 3), F)
    for i in range(n):
        pts[i, :, :2] = rng.uniform(-1, 1, (3, 2))
        pts[i, :, 2] = rng.uniform(-3, 4.5, 3)
        k = i % 3
        if k == 0:
            pts[i, 0, 2] = np.nextafter(F(5.0), F(0.0)) if i % 2 else np.nextafter(F(5.0), F(10.0))
        if k == 1:
            pts[i, 1, 2] = F(5.0) + F(rng.uniform(-1e-4, 1e-4))
            pts[i, 2, 2] = F(6.5)
    pos = pts.reshape(-1, 3)
    nrm = rng.standard_normal((n * 3, 3)).astype(F)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    tex = np.concatenate([rng.uniform(0.05, 0.95, (n * 3, 2)).astype(F), np.zeros((n * 3, 1), F)], 1)
    idx = np.arange(n * 3, dtype=np.uint32).reshape(n, 3).repeat(3, axis=1)
    texs = [rng.integers(0, 256, (32, 32, 3), dtype=np.uint8) for _ in range(4)]
    return {"pos": pos, "tex": tex, "nrm": nrm, "idx": idx}, texs


def _unit(v):
    return v / np.linalg.norm(v)


def random_view(rng):
    """A row of render_frames' table: look_from in a shell of radius 0.2 ... 12 around a look_at within 0.5 of the origin, up
    a random vector of length 0.3 ... 3 at least 10 degrees off the view axis, a light of length 0.25 ... 6."""
    at = _unit(rng.standard_normal(3)) * rng.uniform(0.0, 0.5)
    axis = _unit(rng.standard_normal(3))
    frm = at + axis * np.exp(rng.uniform(np.log(0.2), np.log(12.0)))
    while True:
        up = _unit(rng.standard_normal(3))
        if abs(float(np.dot(up, axis))) < np.cos(np.radians(10.0)):
            break
    up = up * rng.uniform(0.3, 3.0)
    light = _unit(rng.standard_normal(3)) * rng.uniform(0.25, 6.0)
    return np.concatenate([light, frm, at, up]).astype(F)


RANDOM_SEEDS = tuple(range(24))
RANDOM_PIPES = ("phong", "darboux", "default", "specular", "normal_map", "shadow", "occlusion")
RANDOM_SIZES = ((640, 400), (801, 603), (1030, 70), (320, 200))


def random_case(seed):
    """(pipeline, (W, H), views[5, 12]) of a seed: pipeline and size rotate with it."""
    rng = np.random.default_rng(9000 + seed)
    views = np.stack([random_view(rng) for _ in range(5)])
    return RANDOM_PIPES[seed % len(RANDOM_PIPES)], RANDOM_SIZES[seed % len(RANDOM_SIZES)], views


# name -> four (w, h): texture, normal_map, normal_map_tangent, specular_map
TEXTURE_SHAPES = {
    "all_37x51": [(37, 51)] * 4,
    "all_203x250": [(203, 250)] * 4,
    "all_1x1": [(1, 1)] * 4,
    "all_8x4": [(8, 4)] * 4,                  # exactly one block of a one-word set, two by two of a four-word set
    "all_9x5": [(9, 5)] * 4,                  # one texel more than a block on both sides
    "all_51x37": [(51, 37)] * 4,              # the first one transposed: a swapped width and height shows
    "small_normal_maps": [(64, 64), (32, 48), (32, 48), (64, 64)],
    "specular_16x128": [(64, 64), (64, 64), (64, 64), (16, 128)],
    "tangent_larger": [(50, 20), (50, 20), (60, 30), (50, 20)],     # defined upstream: indexed inside a larger image
    "tangent_smaller": [(64, 64), (64, 64), (32, 32), (64, 64)],    # darboux panics upstream at most fragments
}
TEXTURE_PIPES = ("default", "phong", "normal_map", "specular", "darboux", "shadow")
TEXTURE_CAMERA = ([0.5, 0.3, 0.9], [0.0, 0.0, 0.0], [0.0, 1.0, 0.0])
TEXTURE_LIGHT = [0.3, 0.5, 0.8]
TEXTURE_SIZE = (300, 200)


def texture_views():
    """The two views of every texture-shape case: the plain one, and the elevated camera under the short light."""
    return np.stack([view_row(TEXTURE_LIGHT, TEXTURE_CAMERA), view_row(LIGHTS["short"], CAMERAS["elevated"])])


def shape_textures(name):
    """Random images of TEXTURE_SHAPES[name] (uint8 [h, w, 3]); the content depends on the name only."""
    rng = np.random.default_rng(sum(ord(c) * (i + 1) for i, c in enumerate(name)))
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for (w, h) in TEXTURE_SHAPES[name]]


UV_EDGE_SIDE = 24            # the images of the uv edge mesh are 24 x 24 texels
UV_EDGE_CAMERA = ([0.0, 0.0, 1.0], [0.0, 0.0, 0.0], [0.0, 1.0, 0.0])
UV_EDGE_LIGHT = [0.2, 0.4, 0.9]


def uv_edge_views():
    """The three views of the uv-edge cases: one camera, three lights (two of them from behind / below)."""
    return np.stack([view_row(l, UV_EDGE_CAMERA) for l in (UV_EDGE_LIGHT, LIGHTS["back"], LIGHTS["down"])])


def near_w_views():
    return np.stack([view_row(NEAR_W_LIGHT, NEAR_W_CAMERA), view_row(LIGHTS["long"], NEAR_W_CAMERA)])


def uv_edge_mesh(with_v0=False):
    """Three screen-filling quads (two polygons each) in front of UV_EDGE_CAMERA, at three depths, whose uv corners are
    exactly representable: u from 0.0 exactly (texel column 0) to 23.5 / 24 and 23.96875 / 24 -- u * 24 lands on column 23
    plus a fraction --, v from 1/64 (1 - v just below 1: the last row) to 1.0 (1 - v = 0.0 exactly: row 0).  with_v0: one
    more small quad with a v = 0 corner, so 1 - v = 1.0 and the row index equals the image's height: out of range
    upstream (util.rs:40 panics).  Returns (mesh, textures)."""
    s = UV_EDGE_SIDE
    quads = [   # (x0, y0, x1, y1, z, u0, v0, u1, v1)
        (-0.9, -0.9, 0.9, 0.9, -0.2, 0.0, 1.0 / 64.0, 23.5 / s, 1.0),
        (-0.7, -0.8, 0.2, 0.8, 0.0, 0.0, 0.5, 23.96875 / s, 1.0),
        (-0.1, -0.6, 0.8, 0.5, 0.2, 0.125, 1.0 / 64.0, 23.96875 / s, 0.75),
    ]
    if with_v0:
        quads.append((-0.2, -0.2, 0.2, 0.2, 0.4, 0.25, 0.0, 0.75, 0.5))
    pos, tex, idx = [], [], []
    for (x0, y0, x1, y1, z, u0, v0, u1, v1) in quads:
        b = len(pos)
        pos += [[x0, y0, z], [x1, y0, z], [x1, y1, z], [x0, y1, z]]
        tex += [[u0, v0, 0.0], [u1, v0, 0.0], [u1, v1, 0.0], [u0, v1, 0.0]]
        for tri in ((0, 1, 2), (0, 2, 3)):                          # counter-clockwise seen from +z
            idx.append([c for k in tri for c in (b + k, b + k, 0)])
    rng = np.random.default_rng(77)
    texs = [rng.integers(0, 256, (s, s, 3), dtype=np.uint8) for _ in range(4)]
    mesh = {"pos": np.array(pos, F), "tex": np.array(tex, F), "nrm": np.array([[0.0, 0.0, 1.0]], F),
            "idx": np.array(idx, np.uint32)}
    return mesh, texs
