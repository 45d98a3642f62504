"""Procedural stand-in scene for boxes without the reference's assets,
and the 8x8 instancing rule of BASELINE.json's configs[4]."""
import numpy as np


def _splitmix64(seed, n):
    x = (np.uint64(seed) + np.arange(1, n + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15))
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def _noise_image(seed, size, smooth=8):
    """Deterministic low-pass noise in [0,1), float32 [size,size,3]."""
    with np.errstate(over="ignore"):
        r = _splitmix64(seed, size * size * 3)
    a = ((r >> np.uint64(40)).astype(np.float64) / float(1 << 24)).reshape(size, size, 3)
    for axis in (0, 1):
        acc = np.zeros_like(a)
        for k in range(smooth):
            acc += np.roll(a, k, axis=axis)
        a = acc / smooth
    return a.astype(np.float32)


def synthetic_scene(n_lat=31, n_lon=81, tex_size=1024, radius=0.8):
    """UV sphere with 2*n_lat*n_lon triangles (default 5 022 = diablo's polygon count),
    vertex normals = position / r, uv = (lon/2pi, lat/pi) clamped to [0.001, 0.999], and
    four deterministic textures (diffuse, two normal maps, specular exponent 0..64)."""
    lat = np.linspace(0.0, np.pi, n_lat + 1, dtype=np.float64)
    lon = np.linspace(0.0, 2.0 * np.pi, n_lon + 1, dtype=np.float64)
    la, lo = np.meshgrid(lat, lon, indexing="ij")
    nrm = np.stack([np.sin(la) * np.sin(lo), np.cos(la), np.sin(la) * np.cos(lo)], -1).reshape(-1, 3)
    pos = (nrm * radius).astype(np.float32)
    nrm = nrm.astype(np.float32)
    uv = np.stack([np.clip(lo / (2 * np.pi), 0.001, 0.999), np.clip(la / np.pi, 0.001, 0.999),
                   np.zeros_like(la)], -1).reshape(-1, 3).astype(np.float32)
    idx = []
    stride = n_lon + 1
    for i in range(n_lat):
        for j in range(n_lon):
            a, b = i * stride + j, i * stride + j + 1
            c, d = (i + 1) * stride + j, (i + 1) * stride + j + 1
            idx.append([a, a, a, c, c, c, b, b, b])
            idx.append([b, b, b, c, c, c, d, d, d])
    mesh = {"pos": pos, "tex": uv, "nrm": nrm, "idx": np.array(idx, np.uint32)}

    diffuse = (_noise_image(0x5EED0000, tex_size) * 200.0 + 40.0).astype(np.uint8)

    def normal_map(seed):
        n = (_noise_image(seed, tex_size) - 0.5) * 0.4
        n[..., 2] = 1.0
        n /= np.linalg.norm(n, axis=-1, keepdims=True)
        return np.clip((n * 0.5 + 0.5) * 255.0, 0, 255).astype(np.uint8)

    spec = (_noise_image(0x5EED0003, tex_size)[..., :1] * 64.0).astype(np.uint8).repeat(3, axis=-1)
    return mesh, [diffuse, normal_map(0x5EED0001), normal_map(0x5EED0002), spec]


def grid_instances(n=8):
    """instanced_grid's placements as an instance table ([n*n, 4] float32: offset x, y, z, scale; (i major, j
    minor)) for Scene.set_instances: the library's rule p * scale + offset reproduces instanced_grid(mesh, n)'s
    positions bit for bit."""
    table = np.empty((n * n, 4), np.float32)
    for i in range(n):
        for j in range(n):
            table[i * n + j] = ((2 * i + 1) / n - 1.0, (2 * j + 1) / n - 1.0, 0.0, np.float32(1.0 / n))
    return table


def apply_instances(mesh, table):
    """The mesh a table of instances draws, built on the host: positions p * scale + offset (two float32
    roundings) per instance, concatenated in table order; shared normals and uvs.  What an instanced scene must
    render bit for bit."""
    pos, idx = np.asarray(mesh["pos"], np.float32), np.asarray(mesh["idx"], np.uint32)
    table = np.asarray(table, np.float32).reshape(-1, 4)
    all_pos, all_idx = [], []
    for k, (ox, oy, oz, sc) in enumerate(table):
        all_pos.append(((pos * sc).astype(np.float32) + np.array([ox, oy, oz], np.float32)).astype(np.float32))
        q = idx.copy()
        q[:, 0::3] += np.uint32(k * pos.shape[0])
        all_idx.append(q)
    return {"pos": np.concatenate(all_pos), "tex": mesh["tex"], "nrm": mesh["nrm"], "idx": np.concatenate(all_idx)}


def instance_transforms(linear, offset):
    """A transform table for Scene.set_instance_transforms: [n, 24] float32 entries (tr_instance_xform) from `linear`
    [n, 3, 3] and `offset` [n, 3].  m = [linear | offset] row-major, rounded to float32; n = the inverse transpose of
    the float32 linear part, computed in float64 and rounded once.  A singular linear part is a ValueError."""
    lin = np.asarray(linear, np.float32).reshape(-1, 3, 3)
    off = np.asarray(offset, np.float32).reshape(-1, 3)
    if lin.shape[0] != off.shape[0]:
        raise ValueError("one offset per linear part")
    table = np.zeros((lin.shape[0], 24), np.float32)
    for k in range(lin.shape[0]):
        a = lin[k].astype(np.float64)
        if not np.isfinite(a).all() or np.linalg.matrix_rank(a) < 3:
            raise ValueError("instance %d: singular linear part" % k)
        table[k, 0:12] = np.concatenate([lin[k], off[k][:, None]], axis=1).reshape(12)
        table[k, 12:21] = np.linalg.inv(a).T.astype(np.float32).reshape(9)
    return table


def rotation_instances(yaw, pitch, roll, offset, scale):
    """instance_transforms for rigid placements: instance k is turned by yaw[k] about y, then pitch[k] about x, then
    roll[k] about z (radians; linear part = Ry(yaw) Rx(pitch) Rz(roll) * scale[k]) and moved by offset[k]."""
    yaw, pitch, roll, scale = (np.atleast_1d(np.asarray(v, np.float64)) for v in (yaw, pitch, roll, scale))
    offset = np.asarray(offset, np.float64).reshape(-1, 3)
    n = offset.shape[0]
    yaw, pitch, roll, scale = (np.broadcast_to(v, (n,)) for v in (yaw, pitch, roll, scale))
    lin = np.empty((n, 3, 3), np.float64)
    for k in range(n):
        cy, sy, cp, sp, cr, sr = np.cos(yaw[k]), np.sin(yaw[k]), np.cos(pitch[k]), np.sin(pitch[k]), np.cos(roll[k]), np.sin(roll[k])
        ry = np.array([[cy, 0.0, sy], [0.0, 1.0, 0.0], [-sy, 0.0, cy]])
        rx = np.array([[1.0, 0.0, 0.0], [0.0, cp, -sp], [0.0, sp, cp]])
        rz = np.array([[cr, -sr, 0.0], [sr, cr, 0.0], [0.0, 0.0, 1.0]])
        lin[k] = ry @ rx @ rz * scale[k]
    return instance_transforms(lin, offset)


def apply_instance_transforms(mesh, table):
    """The mesh a transform table draws, built on the host in numpy: what a scene with that table must render bit for
    bit.  Per instance (table row e: m = e[0:12] row-major 3 x 4, n = e[12:21] row-major 3 x 3), component r of every
    position (x, y, z) and every normal (a, b, c) becomes, all in float32, each operation rounded once and none fused:
        t = m[4r] * x;  t = t + m[4r+1] * y;  t = t + m[4r+2] * z;  p'_r = t + m[4r+3]
        t = n[3r] * a;  t = t + n[3r+1] * b;                         n'_r = t + n[3r+2] * c
    Positions and normals are concatenated in table order and the position and normal indices rebased; texture
    coordinates are shared.  (apply_instances' counterpart for tr_instance_xform.)"""
    pos, nrm = np.asarray(mesh["pos"], np.float32).reshape(-1, 3), np.asarray(mesh["nrm"], np.float32).reshape(-1, 3)
    idx = np.asarray(mesh["idx"], np.uint32)
    table = np.asarray(table, np.float32).reshape(-1, 24)
    all_pos, all_nrm, all_idx = [], [], []
    x, y, z = pos[:, 0], pos[:, 1], pos[:, 2]
    a, b, c = nrm[:, 0], nrm[:, 1], nrm[:, 2]
    for k, e in enumerate(table):
        p, q = np.empty_like(pos), np.empty_like(nrm)
        for r in range(3):
            t = (e[4 * r] * x).astype(np.float32)
            t = (t + (e[4 * r + 1] * y).astype(np.float32)).astype(np.float32)
            t = (t + (e[4 * r + 2] * z).astype(np.float32)).astype(np.float32)
            p[:, r] = (t + e[4 * r + 3]).astype(np.float32)
            t = (e[12 + 3 * r] * a).astype(np.float32)
            t = (t + (e[13 + 3 * r] * b).astype(np.float32)).astype(np.float32)
            q[:, r] = (t + (e[14 + 3 * r] * c).astype(np.float32)).astype(np.float32)
        all_pos.append(p)
        all_nrm.append(q)
        i = idx.copy()
        i[:, 0::3] += np.uint32(k * pos.shape[0])
        i[:, 2::3] += np.uint32(k * nrm.shape[0])
        all_idx.append(i)
    return {"pos": np.concatenate(all_pos), "tex": mesh["tex"], "nrm": np.concatenate(all_nrm), "idx": np.concatenate(all_idx)}


def instanced_grid(mesh, n=8):
    """BASELINE.json configs[4]: n x n grid of scaled copies, instance (i, j) =
    p / n + ((2i+1)/n - 1, (2j+1)/n - 1, 0), shared normals and uvs, polygons concatenated in
    (i major, j minor) instance order.  The reference has no instancing; this rule is ours."""
    pos, idx = mesh["pos"], mesh["idx"]
    n_pos = pos.shape[0]
    all_pos, all_idx = [], []
    for i in range(n):
        for j in range(n):
            off = np.array([(2 * i + 1) / n - 1.0, (2 * j + 1) / n - 1.0, 0.0], np.float32)
            all_pos.append((pos * np.float32(1.0 / n) + off).astype(np.float32))
            k = idx.copy()
            k[:, 0::3] += np.uint32((i * n + j) * n_pos)
            all_idx.append(k)
    return {"pos": np.concatenate(all_pos), "tex": mesh["tex"], "nrm": mesh["nrm"],
            "idx": np.concatenate(all_idx)}
