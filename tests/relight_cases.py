"""What tests/test_relight_host.py (CPU) and tests/test_relight.py (GPU) share: the sizes, the light sets, the frames,
and the relight rule restated in numpy from the words of tiny_renderer_amd/csrc/tr_relight.h -- float32 operations one at
a time as numpy float32 arrays, np.sqrt and / on float32, the integer steps in int64, the blend as layer_cases.blend_np.
Every array of the restatement is [H, W] with row index y UP like z; the frame's colour is flipped on the way in and out."""
import numpy as np

from tests import layer_cases as LC
from tests import projector_cases as PC

F32_MIN_BITS, F32_MIN, bits = PC.F32_MIN_BITS, PC.F32_MIN, PC.bits
MODES = LC.MODES
CAM, LIGHT = PC.CAM, PC.LIGHT
HOST_SIZES = PC.HOST_SIZES
# below one tile; one tile exactly; a partial tile column and row (the halo crosses tile borders); two and four tile
# columns; the WIDE width that is no multiple of 16 (132); the byte path (131)
GPU_SIZES = ((5, 3), (128, 16), (130, 17), (257, 33), (512, 48), (132, 17), (131, 19))
table = PC.table
f32 = np.float32
IDENTITY = np.eye(4, dtype=np.float64)


def flat(m):
    """A [4, 4] matrix indexed [row, column] as the 16 column-major float32 of tr_relight_params.u."""
    return np.asarray(m, np.float64).T.reshape(16).astype(np.float32)


def random_frame(rng, W, Hh, holes=True):
    return PC.random_frame(rng, W, Hh, holes)


def random_u(rng, W, Hh):
    """A mild perspective from raster to a box around the origin: x, y to about -1..1, depth 10..90 to about -1..1, w
    between 0.7 and 1.3 -- [row, column]."""
    m = np.zeros((4, 4))
    m[0] = [2.0 / max(W - 1, 1), rng.uniform(-0.002, 0.002), rng.uniform(-0.001, 0.001), -1.0]
    m[1] = [rng.uniform(-0.002, 0.002), 2.0 / max(Hh - 1, 1), rng.uniform(-0.001, 0.001), -1.0]
    m[2] = [0.0, 0.0, 1.0 / 40.0, -1.25]
    m[3] = [rng.uniform(-0.0002, 0.0002), rng.uniform(-0.0002, 0.0002), rng.uniform(-0.003, 0.003), 1.0]
    return m


def random_lights(rng, n, specular=True):
    """n lights of all three kinds in turn around the box of random_u, with and without a highlight."""
    import tiny_renderer_amd as T
    out = []
    for k in range(n):
        col = [int(v) for v in rng.integers(0, 256, 3)]
        spec = float(rng.uniform(0.1, 1.0)) if specular and k % 2 == 0 else 0.0
        shin = int(rng.integers(0, 11))
        inten = float(rng.uniform(0.2, 3.0))
        pos = [float(v) for v in rng.uniform(-2.0, 2.0, 3)]
        pos[2] = float(rng.uniform(1.5, 4.0))
        if k % 3 == 0:
            out.append(T.light_directional([float(v) for v in rng.uniform(-1.0, 1.0, 2)] + [float(rng.uniform(0.2, 1.0))], col, inten, spec, shin))
        elif k % 3 == 1:
            out.append(T.light_point(pos, col, inten, float(rng.uniform(0.0, 0.5)), spec, shin))
        else:
            out.append(T.light_spot(pos, [float(v) for v in rng.uniform(-0.5, 0.5, 3)], float(rng.uniform(5.0, 30.0)), float(rng.uniform(35.0, 80.0)), col,
                                    inten, float(rng.uniform(0.0, 0.5)), spec, shin))
    return out


def eye_of(uniforms, look_from):
    """The centre of projection of prepare_uniforms' camera in model space: 5 units behind look_from along the camera's
    direction (its projection's w is 1 - z_cam / 5)."""
    return [float(look_from[i]) + 5.0 * float(uniforms.camera_direction[i]) for i in range(3)]


def view_params(W, Hh, cam=CAM, **kw):
    """relight_params for the frame the tests' drive() renders at camera angle `cam`."""
    import tiny_renderer_amd as T
    from tests import helpers as H
    frm, at, up = H.camera(cam)
    st, view = T.prepare_uniforms(2, W, Hh, H.light(LIGHT), frm, at, up)
    assert st == 0
    return T.relight_params(view, eye_of(view, frm), **kw)


def scene_lights(n, specular=True):
    """n lights of mixed kinds around the unit model of the synthetic scenes."""
    import tiny_renderer_amd as T
    base = [T.light_point([1.5, 1.0, 2.0], (255, 120, 40), 1.5, 0.3, 0.6 if specular else 0.0, 4),
            T.light_spot([-1.5, 1.5, 2.5], [0.0, 0.0, 0.0], 8.0, 25.0, (60, 140, 255), 2.5, 0.1, 0.4 if specular else 0.0, 6),
            T.light_directional([0.3, 1.0, 0.4], (200, 255, 200), 0.5),
            T.light_point([0.0, -1.0, 1.5], (255, 0, 255), 0.8, 1.0),
            T.light_spot([0.5, 0.2, 3.0], [0.3, 0.0, 0.0], 2.0, 6.0, (255, 255, 255), 6.0, 0.0, 1.0 if specular else 0.0, 10),
            T.light_directional([-1.0, 0.2, 0.6], (30, 30, 120), 1.0, 0.3 if specular else 0.0, 2),
            T.light_point([2.0, 2.0, 2.0], (90, 200, 90), 20.0, 2.0),
            T.light_spot([0.0, 2.5, 0.5], [0.0, 0.0, 0.2], 20.0, 60.0, (255, 220, 160), 1.0, 0.05, 0.0, 0)]
    return base[:n]


# ---------------------------------------------------------------------------------------------------------------------
# The rule in numpy
# ---------------------------------------------------------------------------------------------------------------------
def _all_f32(*arrays):
    for a in arrays:
        assert a.dtype == f32, a.dtype


def _finite(flag, *arrays):
    for a in arrays:
        flag &= np.isfinite(a)


def dot3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def cross3(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def normalize3(a):
    n = np.sqrt(dot3(a, a))
    return [a[0] / n, a[1] / n, a[2] / n]


def position_np(u16, z):
    """Step position: (ok, [Px, Py, Pz], finite) over the frame."""
    u = np.asarray(u16, f32)
    Hh, W = z.shape
    yy, xx = np.mgrid[0:Hh, 0:W]
    x, y, z = xx.astype(f32), yy.astype(f32), z.astype(f32)
    drawn = bits(z) != F32_MIN_BITS
    finite = np.ones(z.shape, bool)
    c = []
    with np.errstate(all="ignore"):
        for i in range(4):
            t0, t1, t2 = u[i] * x, u[4 + i] * y, u[8 + i] * z
            s0 = t0 + t1
            s1 = s0 + t2
            ci = s1 + u[12 + i]
            _all_f32(t0, t1, t2, s0, s1, ci)
            _finite(finite, t0, t1, t2, s0, s1, ci)
            c.append(ci)
        w = c[3]
        ok = drawn & np.isfinite(w) & (w != 0)
        r = f32(1.0) / np.where(ok, w, f32(1.0))
        P = [c[0] * r, c[1] * r, c[2] * r]
        _all_f32(r, *P)
        _finite(finite, r, *P)
        ok &= np.isfinite(P[0]) & np.isfinite(P[1]) & np.isfinite(P[2])
    finite |= ~drawn          # (a pixel that is not drawn takes no step)
    return ok, P, finite


def shifted(a, dx, dy, fill):
    """a at (x + dx, y + dy), `fill` outside the frame."""
    Hh, W = a.shape
    out = np.full((Hh + 2, W + 2), fill, a.dtype)
    out[1:-1, 1:-1] = a
    return out[1 + dy:1 + dy + Hh, 1 + dx:1 + dx + W]


def _difference(ok, P, z, axis):
    dx, dy = (1, 0) if axis == 0 else (0, 1)
    a_ok, b_ok = shifted(ok, dx, dy, False), shifted(ok, -dx, -dy, False)
    za, zb = shifted(z, dx, dy, f32(0)), shifted(z, -dx, -dy, f32(0))
    with np.errstate(all="ignore"):
        da, db = np.abs(za - z), np.abs(zb - z)
        use_a = np.where(a_ok & b_ok, da <= db, a_ok)
        d = [np.where(use_a, shifted(P[k], dx, dy, f32(0)) - P[k], P[k] - shifted(P[k], -dx, -dy, f32(0))) for k in range(3)]
    _all_f32(da, db, *d)
    return a_ok | b_ok, d, use_a


def normal_np(u16, eye, z):
    """Steps position and normal: (has, n, v, P, finite)."""
    z = np.asarray(z, f32)
    ok, P, finite = position_np(u16, z)
    e = np.asarray(eye, f32)
    hx, dx, _ = _difference(ok, P, z, 0)
    hy, dy, _ = _difference(ok, P, z, 1)
    has = ok & hx & hy
    with np.errstate(all="ignore"):
        N = cross3(dx, dy)
        V = [e[k] - P[k] for k in range(3)]
        nv = dot3(N, V)
        N = [np.where(nv < 0, -N[k], N[k]) for k in range(3)]
        nn, vv = dot3(N, N), dot3(V, V)
        has &= (nn > 0) & np.isfinite(nn) & ~np.isnan(nv) & (vv > 0) & np.isfinite(vv)
        n, v = normalize3(N), normalize3(V)
    _all_f32(nv, nn, vv, *N, *V, *n, *v)
    fin = np.ones(z.shape, bool)
    _finite(fin, nv, nn, vv, *dx, *dy, *N, *V, *n, *v)
    finite &= fin | ~has
    return has, n, v, P, finite


def level_np(l, P, n, v, has):
    """Step light for one tr_light: (q [H, W] int64 -- 0 where the light adds nothing --, finite)."""
    shape = has.shape
    pos, dr = np.array(list(l.pos), f32), np.array(list(l.dir), f32)
    fin = np.ones(shape, bool)
    live = has.copy()
    with np.errstate(all="ignore"):
        if l.kind == 0:
            L = [np.full(shape, dr[k], f32) for k in range(3)]
            att = np.full(shape, 1.0, f32)
        else:
            D = [pos[k] - P[k] for k in range(3)]
            d2 = dot3(D, D)
            live &= (d2 > 0) & np.isfinite(d2)
            L = normalize3(D)
            t = f32(l.falloff) * d2
            att = f32(1.0) / (f32(1.0) + t)
            _finite(fin, d2, t, att, *D, *L)
            if l.kind == 2:
                c = dot3([-L[0], -L[1], -L[2]], [np.full(shape, dr[k], f32) for k in range(3)])
                ramp = (c - f32(l.cos_outer)) * f32(l.cone_scale)
                cone = np.where(ramp > 0, np.where(ramp < 1, ramp, f32(1.0)), f32(0.0)).astype(f32)
                att = att * cone
                _finite(fin, c, ramp, att)
        diff = dot3(n, L)
        _finite(fin, diff)
        live &= diff > 0
        if l.specular > 0:
            h = normalize3([L[k] + v[k] for k in range(3)])
            nh = dot3(n, h)
            s = np.where(nh > 0, nh, f32(0.0)).astype(f32)
            for _ in range(int(l.shininess_log2)):
                s = s * s
            hl = f32(l.specular) * s
            diff = diff + hl
            _finite(fin, nh, s, hl, diff, *h)
        lit = diff * att
        e = lit * f32(l.intensity)
        m = np.where(e > 16, f32(16.0), e).astype(f32) * f32(256.0)
        _all_f32(diff, att, lit, e, m)
        _finite(fin, lit, e, m)
        q = np.where(np.isnan(m), 0.0, np.clip(np.nan_to_num(m, nan=0.0), 0.0, 4294967295.0)).astype(np.int64)
    return np.where(live, q, 0), fin | ~live


def rule_np(rgb, z, u16, eye, lights=(), ambient=(0, 0, 0), mode="add", opacity=256, albedo=False, show_normals=False):
    """The lit frame: rgb [H, W, 3] row 0 = top, z [H, W] y up, lights a sequence of tr_light.  Returns (out, has,
    finite): has and finite [H, W] y up -- which pixels have a normal, and for which every intermediate stayed finite."""
    has, n, v, P, finite = normal_np(u16, eye, z)
    d = rgb[::-1].astype(np.int64)
    if show_normals:
        with np.errstate(all="ignore"):
            comps = [((n[k] * f32(0.5) + f32(0.5)) * f32(255.0)) for k in range(3)]
            _all_f32(*comps)
            s = np.stack([np.clip(np.nan_to_num(c, nan=0.0), 0.0, 255.0).astype(np.int64) for c in comps], axis=2)
    else:
        acc = np.zeros(z.shape + (3,), np.int64)
        for l in lights:
            q, fin = level_np(l, P, n, v, has)
            finite &= fin
            for c in range(3):
                acc[..., c] += q * int(l.colour[c])
        s = np.minimum(255, (256 * np.array([int(a) for a in ambient], np.int64) + acc + 128) >> 8)
    if albedo:
        s = (s * d + 127) // 255
    cov = 255 * int(opacity)
    lit = (LC.blend_np(mode, s, d) * cov + d * (65280 - cov) + 32640) // 65280
    out = np.where(has[..., None], lit, d).astype(np.uint8)[::-1]
    return out, has, finite
