"""Python mirror of the reference's `Scene` (src/scene.rs:25-269) over the C ABI."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, load_library

# shader.rs:100-109
PIPELINES = ("default", "phong", "normal_map", "specular", "darboux", "shadow", "occlusion")


def _f3(v):
    return (C.c_float * 3)(*[float(x) for x in v])


def _mesh_struct(mesh, keep):
    pos = np.ascontiguousarray(mesh["pos"], np.float32).reshape(-1, 3)
    tex = np.ascontiguousarray(mesh["tex"], np.float32).reshape(-1, 3)
    nrm = np.ascontiguousarray(mesh["nrm"], np.float32).reshape(-1, 3)
    idx = np.ascontiguousarray(mesh["idx"], np.uint32).reshape(-1, 9)
    keep += [pos, tex, nrm, idx]
    fp = C.POINTER(C.c_float)
    return _lib.Mesh(pos.ctypes.data_as(fp), tex.ctypes.data_as(fp), nrm.ctypes.data_as(fp),
                     idx.ctypes.data_as(C.POINTER(C.c_uint32)), pos.shape[0], tex.shape[0],
                     nrm.shape[0], idx.shape[0])


def _instance_table(instances, per_frame=False):
    """[n, 4] float32 (offset x, y, z, scale) -- or [n_frames, n, 4] with per_frame -- as a contiguous array."""
    a = np.ascontiguousarray(instances, np.float32)
    if a.shape[-1:] != (4,) or a.ndim != (3 if per_frame else 2):
        raise ValueError("instance table must be [%sn, 4] float32 (offset xyz, scale)" % ("n_frames, " if per_frame else ""))
    return a


def _transform_table(table, per_frame=False):
    """[n, 24] float32 (tr_instance_xform: m 3 x 4, n 3 x 3, 3 unused) -- or [n_frames, n, 24] with per_frame."""
    a = np.ascontiguousarray(table, np.float32)
    if a.shape[-1:] != (24,) or a.ndim != (3 if per_frame else 2):
        raise ValueError("instance transform table must be [%sn, 24] float32 (instance_transforms builds one)"
                         % ("n_frames, " if per_frame else ""))
    return a


def transform_mesh(mesh, table):
    """tr_instance_transform_mesh: (pos [n * n_pos, 3], nrm [n * n_nrm, 3]) of the concatenated mesh the [n, 24] transform
    table draws, by the inline function the vertex stage calls, on the host (no GPU needed)."""
    a = _transform_table(table)
    keep = []
    m = _mesh_struct(mesh, keep)
    pos = np.empty((a.shape[0] * m.n_pos, 3), np.float32)
    nrm = np.empty((a.shape[0] * m.n_nrm, 3), np.float32)
    check(load_library().tr_instance_transform_mesh(C.byref(m), a.shape[0], a.ctypes.data, pos.ctypes.data, nrm.ctypes.data))
    return pos, nrm


def _morph_deltas(mesh, dpos, dnrm):
    """(dpos [T, n_pos, 3], dnrm [T, n_nrm, 3]) float32, contiguous, checked against the mesh's arrays."""
    n_pos = np.asarray(mesh["pos"]).reshape(-1, 3).shape[0]
    n_nrm = np.asarray(mesh["nrm"]).reshape(-1, 3).shape[0]
    dp = np.ascontiguousarray(dpos, np.float32)
    dn = np.ascontiguousarray(dnrm, np.float32)
    if dp.ndim != 3 or dn.ndim != 3 or dp.shape[1:] != (n_pos, 3) or dn.shape[1:] != (n_nrm, 3) or dp.shape[0] != dn.shape[0]:
        raise ValueError("morph targets must be dpos [T, %d, 3] and dnrm [T, %d, 3] float32" % (n_pos, n_nrm))
    if dp.shape[0] > _lib.TR_MORPH_MAX_TARGETS:
        raise ValueError("at most %d morph targets" % _lib.TR_MORPH_MAX_TARGETS)
    return dp, dn


def _morph_weights(w, n_targets, per_frame=False):
    """[T] float32 -- or [n_frames, T] with per_frame -- as a contiguous array."""
    a = np.ascontiguousarray(w, np.float32)
    if a.ndim != (2 if per_frame else 1) or a.shape[-1] != n_targets:
        raise ValueError("morph weights must be [%s%d] float32 (one weight per target)" % ("n_frames, " if per_frame else "", n_targets))
    return a


def morph_deltas(base, target):
    """One morph target from a second mesh of identical topology: (dpos [1, n_pos, 3], dnrm [1, n_nrm, 3]) =
    target - base in float32; stack several with np.concatenate for set_morph_targets."""
    if not np.array_equal(np.asarray(base["idx"], np.uint32).reshape(-1, 9), np.asarray(target["idx"], np.uint32).reshape(-1, 9)):
        raise ValueError("morph target has different indices: the meshes must share their topology")
    out = []
    for key in ("pos", "nrm"):
        b = np.asarray(base[key], np.float32).reshape(-1, 3)
        t = np.asarray(target[key], np.float32).reshape(-1, 3)
        if b.shape != t.shape:
            raise ValueError("morph target has %d %s entries, the mesh %d" % (t.shape[0], key, b.shape[0]))
        out.append((t - b)[None])
    return out[0], out[1]


def morph_mesh(mesh, dpos, dnrm, weights):
    """tr_morph_mesh: (pos [n_pos, 3], nrm [n_nrm, 3]) of `mesh` under the pose `weights` [T] of the targets dpos
    [T, n_pos, 3], dnrm [T, n_nrm, 3], by the inline function k_morph calls, on the host (no GPU needed)."""
    dp, dn = _morph_deltas(mesh, dpos, dnrm)
    w = _morph_weights(weights, dp.shape[0])
    keep = []
    m = _mesh_struct(mesh, keep)
    pos = np.empty((m.n_pos, 3), np.float32)
    nrm = np.empty((m.n_nrm, 3), np.float32)
    check(load_library().tr_morph_mesh(C.byref(m), dp.shape[0], dp.ctypes.data, dn.ctypes.data, w.ctypes.data,
                                       pos.ctypes.data, nrm.ctypes.data))
    return pos, nrm


def _skin(mesh, bones, weights):
    """(bones [n_pos, 4] uint32, weights [n_pos, 4] float32) contiguous, checked against the mesh's positions."""
    n_pos = np.asarray(mesh["pos"]).reshape(-1, 3).shape[0]
    b = np.asarray(bones)
    w = np.ascontiguousarray(weights, np.float32)
    if b.shape != (n_pos, _lib.TR_SKIN_INFLUENCES) or w.shape != b.shape:
        raise ValueError("a skin is bones [%d, 4] uint32 and weights [%d, 4] float32 (four influences per position)" % (n_pos, n_pos))
    if b.size and (not np.issubdtype(b.dtype, np.integer) or b.min() < 0):
        raise ValueError("bone indices must be non-negative integers")
    return np.ascontiguousarray(b, np.uint32), w


def _palette(palette, n_bones=None, per_frame=False):
    """[n_bones, 24] float32 (tr_instance_xform per bone) -- or [n_frames, n_bones, 24] with per_frame."""
    a = np.ascontiguousarray(palette, np.float32)
    if a.shape[-1:] != (24,) or a.ndim != (3 if per_frame else 2) or a.shape[-2] == 0:
        raise ValueError("a bone palette must be [%sn_bones, 24] float32 (instance_transforms builds one)"
                         % ("n_frames, " if per_frame else ""))
    if a.shape[-2] > _lib.TR_SKIN_MAX_BONES:
        raise ValueError("at most %d bones" % _lib.TR_SKIN_MAX_BONES)
    if n_bones is not None and a.shape[-2] != n_bones:
        raise ValueError("the palette has %d bones, the skin %d" % (a.shape[-2], n_bones))
    return a


def skin_mesh(mesh, bones, weights, palette):
    """tr_skin_mesh: the mesh skinned on the host (no GPU needed) by the inline function k_skin calls -- bones [n_pos, 4]
    uint32 and weights [n_pos, 4] float32 per position index, palette [n_bones, 24] float32.  Returns a mesh dict whose
    pos [n_tri * 3, 3], nrm [n_tri * 3, 3] and idx [n_tri, 9] are unrolled (a position and a normal per corner); tex and
    everything else are the mesh's own."""
    b, w = _skin(mesh, bones, weights)
    pal = _palette(palette)
    if b.size and int(b.max()) >= pal.shape[0]:
        raise ValueError("bone index %d beyond the palette's %d bones" % (int(b.max()), pal.shape[0]))
    keep = []
    m = _mesh_struct(mesh, keep)
    pos = np.empty((m.n_tri * 3, 3), np.float32)
    nrm = np.empty((m.n_tri * 3, 3), np.float32)
    idx = np.empty((m.n_tri, 9), np.uint32)
    check(load_library().tr_skin_mesh(C.byref(m), pal.shape[0], b.ctypes.data, w.ctypes.data, pal.ctypes.data,
                                      pos.ctypes.data, nrm.ctypes.data, idx.ctypes.data))
    return dict(mesh, pos=pos, nrm=nrm, idx=idx)


def composite_host(z_dst, rgb_dst, z_src, rgb_src, win_dst=None, win_src=None, winner_base=0):
    """tr_composite_host: the rule of Scene.composite on the host (no GPU needed), by the inline function k_composite
    calls.  z [..] float32, rgb [.., 3] uint8 and optional winner words [..] uint32, all in one pixel order; src wins a
    pixel where it is covered (z bits != f32::MIN) and not (zs <= zd).  Returns new (z, rgb) -- or (z, rgb, winner) with
    win_dst -- and leaves its arguments alone."""
    z = np.array(z_dst, np.float32, order="C")
    rgb = np.array(rgb_dst, np.uint8, order="C")
    zs = np.ascontiguousarray(z_src, np.float32)
    rs = np.ascontiguousarray(rgb_src, np.uint8)
    if zs.shape != z.shape or rgb.shape != z.shape + (3,) or rs.shape != rgb.shape:
        raise ValueError("composite_host: z arrays of one shape, rgb arrays of that shape + (3,)")
    win = ws = None
    if win_dst is not None:
        if win_src is None:
            raise ValueError("composite_host: win_dst needs win_src")
        win = np.array(win_dst, np.uint32, order="C")
        ws = np.ascontiguousarray(win_src, np.uint32)
        if win.shape != z.shape or ws.shape != z.shape:
            raise ValueError("composite_host: winner arrays must have the shape of z")
    check(load_library().tr_composite_host(z.size, z.ctypes.data, rgb.ctypes.data, win.ctypes.data if win is not None else None,
                                           zs.ctypes.data, rs.ctypes.data, ws.ctypes.data if ws is not None else None,
                                           int(winner_base) & 0xFFFFFFFF))
    return (z, rgb) if win is None else (z, rgb, win)


def shadow_merge_host(dst, src):
    """tr_shadow_merge_host: the rule of Scene.shadow_merge on the host (no GPU needed), by the inline function
    k_shadow_merge calls -- per value `if (zs >= zd) zd = zs`, the reference's light-space test.  Two float32 arrays of
    one shape; returns the merged array and leaves its arguments alone."""
    z = np.array(dst, np.float32, order="C")
    zs = np.ascontiguousarray(src, np.float32)
    if zs.shape != z.shape:
        raise ValueError("shadow_merge_host: the arrays must have one shape")
    check(load_library().tr_shadow_merge_host(z.size, z.ctypes.data, zs.ctypes.data))
    return z


TWO_PASS_PIPELINES = ("shadow", "occlusion")   # the pipelines with a light-space depth pass and a shadow buffer of their own


AO_MAX_RADIUS, AO_MAX_RINGS = 16, 4   # (TR_AO_MAX_RADIUS, TR_AO_MAX_RINGS)


class AoParams(C.Structure):
    """tr_ao_params"""
    _fields_ = [("struct_size", C.c_uint32), ("radius", C.c_uint32), ("rings", C.c_uint32), ("flags", C.c_uint32),
                ("threshold", C.c_float), ("falloff", C.c_float)]


def ao_params(radius=8, rings=1, threshold=1.0, falloff=20.0, grey=False):
    """tr_ao_params from the keyword arguments of Scene.ambient_occlusion / ambient_occlusion_host; ValueError for what
    the library would refuse (include/tiny_renderer.h)."""
    for name, v in (("radius", radius), ("rings", rings)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError("ambient occlusion: %s must be an integer" % name)
    if not 1 <= radius <= AO_MAX_RADIUS:
        raise ValueError("ambient occlusion: radius must be 1..%d pixels" % AO_MAX_RADIUS)
    if not 1 <= rings <= min(AO_MAX_RINGS, radius):
        raise ValueError("ambient occlusion: rings must be 1..%d and at most the radius" % AO_MAX_RINGS)
    threshold, falloff = float(threshold), float(falloff)
    with np.errstate(over="ignore"):   # (as f32: what the library gets)
        t32, f32 = np.float32(threshold), np.float32(falloff)
    if not np.isfinite(t32) or t32 < 0.0:
        raise ValueError("ambient occlusion: threshold must be finite and >= 0")
    if not np.isfinite(f32) or not f32 > 0.0:
        raise ValueError("ambient occlusion: falloff must be finite and > 0")
    return AoParams(C.sizeof(AoParams), int(radius), int(rings), 1 if grey else 0, threshold, falloff)


def ambient_occlusion_host(z, rgb, radius=8, rings=1, threshold=1.0, falloff=20.0, grey=False):
    """tr_ao_host: the rule of Scene.ambient_occlusion on the host (no GPU needed), by the inline functions k_ao calls.
    z [H, W] float32 with row 0 = bottom (read_z_f32), rgb [H, W, 3] uint8 with row 0 = top (get_frame_buffer).  Returns
    the shaded frame and leaves its arguments alone."""
    p = ao_params(radius, rings, threshold, falloff, grey)
    zz = np.ascontiguousarray(z, np.float32)
    out = np.array(rgb, np.uint8, order="C")
    if zz.ndim != 2 or out.shape != zz.shape + (3,):
        raise ValueError("ambient_occlusion_host: z [H, W] and rgb [H, W, 3]")
    check(load_library().tr_ao_host(zz.shape[1], zz.shape[0], zz.ctypes.data, out.ctypes.data, C.addressof(p)))
    return out


def ao_offsets(radius, rings=1):
    """tr_ao_offsets: the [16 * rings, 2] int8 sample offsets {dx, dy} of a call, in the rule's order."""
    ao_params(radius, rings)
    out = np.zeros((16 * int(rings), 2), np.int8)
    check(load_library().tr_ao_offsets(int(radius), int(rings), out.ctypes.data))
    return out


ACCUMULATE_MAX_FRAMES = 32   # (TR_ACCUMULATE_MAX_FRAMES)


def accumulate_weights(n_frames, weights=None):
    """(n, uint32 array or None) as tr_scene_accumulate takes them; ValueError for what the library would refuse
    (include/tiny_renderer.h) as far as the host alone can tell."""
    if isinstance(n_frames, bool) or not isinstance(n_frames, (int, np.integer)):
        raise ValueError("accumulate: n_frames must be an integer")
    n = int(n_frames)
    if not 1 <= n <= ACCUMULATE_MAX_FRAMES:
        raise ValueError("accumulate: n_frames must be 1..%d" % ACCUMULATE_MAX_FRAMES)
    if weights is None:
        return n, None
    w = np.asarray(weights)
    if w.ndim != 1 or w.shape[0] != n or w.dtype.kind not in "iu":
        raise ValueError("accumulate: weights must be %d integers" % n)
    if (w < 0).any() or (w > 255).any():
        raise ValueError("accumulate: weights must be 0..255")
    if not w.any():
        raise ValueError("accumulate: every weight is zero")
    return n, np.ascontiguousarray(w, np.uint32)


def accumulate_host(frames, weights=None):
    """tr_accumulate_host: the rule of Scene.accumulate on the host (no GPU needed), by the inline function k_accumulate
    calls.  frames: n uint8 arrays of one shape (or an [n, ...] array), frames[k] weighted weights[k] (None: all 1);
    returns (sum of w_k * F_k + D // 2) // D with D = sum of w_k, in the frames' shape."""
    fr = [np.ascontiguousarray(f, np.uint8) for f in frames]
    n, w = accumulate_weights(len(fr), weights)
    if any(f.shape != fr[0].shape for f in fr):
        raise ValueError("accumulate_host: the frames differ in shape")
    out = np.empty(fr[0].shape, np.uint8)
    ptrs = (C.c_void_p * n)(*[f.ctypes.data for f in fr])
    check(load_library().tr_accumulate_host(out.size, n, ptrs, w.ctypes.data if w is not None else None, out.ctypes.data))
    return out


DOF_MAX_RADIUS, DOF_SHOW_COC = 8, 1   # (TR_DOF_MAX_RADIUS, TR_DOF_SHOW_COC)


class DofParams(C.Structure):
    """tr_dof_params"""
    _fields_ = [("struct_size", C.c_uint32), ("max_radius", C.c_uint32), ("background_radius", C.c_uint32), ("flags", C.c_uint32),
                ("focus", C.c_float), ("range", C.c_float), ("scale", C.c_float)]


def dof_params(focus, scale, max_radius=4, background_radius=0, flags=0, range=0.0):
    """tr_dof_params for Scene.depth_of_field / depth_of_field_host / dof_coc: the circle of confusion of a drawn pixel is
    min(max_radius, ((|z - focus| - range) * scale) as u32) pixels, that of a pixel not drawn background_radius; flags:
    DOF_SHOW_COC or 0.  ValueError for what the library would refuse (include/tiny_renderer.h)."""
    for name, v in (("max_radius", max_radius), ("background_radius", background_radius), ("flags", flags)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError("depth of field: %s must be an integer" % name)
    if not 1 <= max_radius <= DOF_MAX_RADIUS:
        raise ValueError("depth of field: max_radius must be 1..%d pixels" % DOF_MAX_RADIUS)
    if not 0 <= background_radius <= max_radius:
        raise ValueError("depth of field: background_radius must be 0..max_radius")
    if flags & ~DOF_SHOW_COC:
        raise ValueError("depth of field: unknown flags")
    focus, range, scale = float(focus), float(range), float(scale)
    with np.errstate(over="ignore"):   # (as f32: what the library gets)
        f32, r32, s32 = np.float32(focus), np.float32(range), np.float32(scale)
    if not np.isfinite(f32):
        raise ValueError("depth of field: focus must be finite")
    if not np.isfinite(r32) or r32 < 0.0:
        raise ValueError("depth of field: range must be finite and >= 0")
    if not np.isfinite(s32) or not s32 > 0.0:
        raise ValueError("depth of field: scale must be finite and > 0")
    return DofParams(C.sizeof(DofParams), int(max_radius), int(background_radius), int(flags), focus, range, scale)


def _check_params(params, kind, who, maker):
    """The refusal of `params` that `maker` did not build (who: the caller's name in the text)."""
    if not isinstance(params, kind):
        raise ValueError("%s: params must come from %s" % (who, maker))


def depth_of_field_host(z, rgb, params):
    """tr_dof_host: the rule of Scene.depth_of_field on the host (no GPU needed), by the inline functions k_dof calls.
    z [H, W] float32 with row 0 = bottom (read_z_f32), rgb [H, W, 3] uint8 with row 0 = top (get_frame_buffer), params
    from dof_params.  Returns the blurred frame and leaves its arguments alone."""
    _check_params(params, DofParams, "depth_of_field_host", "dof_params")
    zz = np.ascontiguousarray(z, np.float32)
    src = np.ascontiguousarray(rgb, np.uint8)
    if zz.ndim != 2 or src.shape != zz.shape + (3,):
        raise ValueError("depth_of_field_host: z [H, W] and rgb [H, W, 3]")
    out = np.empty_like(src)
    check(load_library().tr_dof_host(zz.shape[1], zz.shape[0], zz.ctypes.data, src.ctypes.data, out.ctypes.data, C.addressof(params)))
    return out


def dof_coc(params, z):
    """tr_dof_coc: the circles of confusion (uint8, z's shape) of the depths z under params (dof_params)."""
    _check_params(params, DofParams, "dof_coc", "dof_params")
    zz = np.ascontiguousarray(z, np.float32)
    out = np.empty(zz.shape, np.uint8)
    check(load_library().tr_dof_coc(C.addressof(params), zz.size, zz.ctypes.data, out.ctypes.data))
    return out


OUTLINE_MAX_RADIUS, OUTLINE_CREASES, OUTLINE_ONLY = 3, 1, 2   # (TR_OUTLINE_MAX_RADIUS, TR_OUTLINE_CREASES, TR_OUTLINE_ONLY)
OUTLINE_SIL, OUTLINE_STEP, OUTLINE_CREASE = 1, 2, 4           # the kind bits of outline_kinds


class OutlineParams(C.Structure):
    """tr_outline_params"""
    _fields_ = [("struct_size", C.c_uint32), ("radius", C.c_uint32), ("flags", C.c_uint32), ("opacity", C.c_uint32),
                ("ink", C.c_uint8 * 4), ("paper", C.c_uint8 * 4), ("depth_step", C.c_float), ("crease", C.c_float)]


def _rgb0(colour, name):
    c = [int(v) for v in colour]
    if len(c) != 3 or not all(0 <= v <= 255 for v in c):
        raise ValueError("outline: %s must be three values 0..255" % name)
    return (C.c_uint8 * 4)(c[0], c[1], c[2], 0)


def outline_params(radius=1, depth_step=1.0, crease=None, ink=(0, 0, 0), opacity=256, only=False, paper=(255, 255, 255)):
    """tr_outline_params for Scene.outline / outline_host / outline_kinds: ink reaches `radius` pixels (0..3, Chebyshev)
    from a seed -- a drawn pixel beside one not drawn, on the nearer side of a depth step larger than depth_step, or, with
    crease given (which sets OUTLINE_CREASES), on a fold whose second difference of depth exceeds it.  opacity 0..256;
    only=True draws on `paper` instead of the frame (OUTLINE_ONLY).  ValueError for what the library would refuse
    (include/tiny_renderer.h)."""
    for name, v in (("radius", radius), ("opacity", opacity)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError("outline: %s must be an integer" % name)
    if not 0 <= radius <= OUTLINE_MAX_RADIUS:
        raise ValueError("outline: radius must be 0..%d pixels" % OUTLINE_MAX_RADIUS)
    if not 0 <= opacity <= 256:
        raise ValueError("outline: opacity must be 0..256")
    flags = (OUTLINE_CREASES if crease is not None else 0) | (OUTLINE_ONLY if only else 0)
    for name, v in (("depth_step", depth_step), ("crease", 0.0 if crease is None else crease)):
        with np.errstate(over="ignore"):   # (as f32: what the library gets)
            v32 = np.float32(float(v))
        if not np.isfinite(v32) or v32 < 0.0:
            raise ValueError("outline: %s must be finite and >= 0" % name)
    return OutlineParams(C.sizeof(OutlineParams), int(radius), flags, int(opacity), _rgb0(ink, "ink"), _rgb0(paper, "paper"),
                         float(depth_step), 0.0 if crease is None else float(crease))


def outline_host(z, rgb, params, in_place=False):
    """tr_outline_host: the rule of Scene.outline on the host (no GPU needed), by the inline functions k_outline calls.
    z [H, W] float32 with row 0 = bottom (read_z_f32), rgb [H, W, 3] uint8 with row 0 = top (get_frame_buffer), params
    from outline_params.  Returns the outlined frame and leaves its arguments alone; in_place=True hands the library
    one buffer as rgb and out (a copy of rgb), which the rule allows."""
    _check_params(params, OutlineParams, "outline_host", "outline_params")
    zz = np.ascontiguousarray(z, np.float32)
    src = np.ascontiguousarray(rgb, np.uint8)
    if zz.ndim != 2 or src.shape != zz.shape + (3,):
        raise ValueError("outline_host: z [H, W] and rgb [H, W, 3]")
    out = src.copy() if in_place else np.empty_like(src)
    check(load_library().tr_outline_host(zz.shape[1], zz.shape[0], zz.ctypes.data, out.ctypes.data if in_place else src.ctypes.data,
                                         out.ctypes.data, C.addressof(params)))
    return out


def outline_kinds(z, params):
    """tr_outline_kinds: the kind bits (OUTLINE_SIL 1, OUTLINE_STEP 2, OUTLINE_CREASE 4; uint8, z's shape and orientation)
    of every pixel of the depths z [H, W] under params (outline_params) -- for choosing depth_step and crease."""
    _check_params(params, OutlineParams, "outline_kinds", "outline_params")
    zz = np.ascontiguousarray(z, np.float32)
    if zz.ndim != 2:
        raise ValueError("outline_kinds: z [H, W]")
    out = np.zeros(zz.shape, np.uint8)
    check(load_library().tr_outline_kinds(zz.shape[1], zz.shape[0], zz.ctypes.data, C.addressof(params), out.ctypes.data))
    return out


AA_MAX_SEARCH, AA_SHOW_BLEND = 8, 1   # (TR_AA_MAX_SEARCH, TR_AA_SHOW_BLEND)


class AaParams(C.Structure):
    """tr_aa_params"""
    _fields_ = [("struct_size", C.c_uint32), ("contrast_min", C.c_uint32), ("contrast_rel", C.c_uint32), ("search", C.c_uint32),
                ("subpixel", C.c_uint32), ("flags", C.c_uint32)]


def aa_params(contrast_min=8, contrast_rel=32, search=8, subpixel=192, show_blend=False):
    """tr_aa_params for Scene.antialias / Scene.get_antialiased / aa_host: a pixel is filtered when the luma range of
    itself and its four neighbours reaches contrast_min (0..255) and contrast_rel / 256 (0..256) of their brightest; the
    edge's ends are looked for up to `search` pixels away (1..8); subpixel (0..256) weighs the term that pulls a lone
    pixel towards its surroundings; show_blend=True shows the blend weight instead of the picture (AA_SHOW_BLEND).
    ValueError for what the library would refuse (include/tiny_renderer.h)."""
    for name, v in (("contrast_min", contrast_min), ("contrast_rel", contrast_rel), ("search", search), ("subpixel", subpixel)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError("antialias: %s must be an integer" % name)
    if not 0 <= contrast_min <= 255:
        raise ValueError("antialias: contrast_min must be 0..255")
    if not 0 <= contrast_rel <= 256:
        raise ValueError("antialias: contrast_rel must be 0..256")
    if not 1 <= search <= AA_MAX_SEARCH:
        raise ValueError("antialias: search must be 1..%d pixels" % AA_MAX_SEARCH)
    if not 0 <= subpixel <= 256:
        raise ValueError("antialias: subpixel must be 0..256")
    return AaParams(C.sizeof(AaParams), int(contrast_min), int(contrast_rel), int(search), int(subpixel), AA_SHOW_BLEND if show_blend else 0)


def aa_host(rgb, params):
    """tr_aa_host: the rule of Scene.antialias on the host (no GPU needed), by the inline functions k_aa calls.  rgb
    [H, W, 3] uint8 with row 0 = top (get_frame_buffer), params from aa_params.  Returns the filtered frame and leaves its
    arguments alone."""
    _check_params(params, AaParams, "aa_host", "aa_params")
    src = np.ascontiguousarray(rgb, np.uint8)
    if src.ndim != 3 or src.shape[2] != 3:
        raise ValueError("aa_host: rgb [H, W, 3]")
    out = np.empty_like(src)
    check(load_library().tr_aa_host(src.shape[1], src.shape[0], src.ctypes.data, out.ctypes.data, C.addressof(params)))
    return out


RESIZE_AREA, RESIZE_BILINEAR, RESIZE_MAX_TAPS, RESIZE_MAX_SIDE = 0, 1, 16, 8192   # (TR_RESIZE_AREA, TR_RESIZE_BILINEAR, TR_RESIZE_MAX_TAPS)
RESIZE_FILTERS = {"area": RESIZE_AREA, "bilinear": RESIZE_BILINEAR}


class ResizeParams(C.Structure):
    """tr_resize_params"""
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("filter", C.c_uint32), ("flags", C.c_uint32)]


def _resize_filter(filter, who):
    if filter in RESIZE_FILTERS:
        return RESIZE_FILTERS[filter]
    if not isinstance(filter, (bool, str)) and filter in RESIZE_FILTERS.values():
        return int(filter)
    raise ValueError("%s: filter must be TR_RESIZE_AREA or TR_RESIZE_BILINEAR" % who)


def resize_params(src_width, src_height, width, height, filter="area", who="resize"):
    """tr_resize_params for a source of src_width x src_height pixels: the output's width x height, each 1..8192 and at
    least an eighth of the source's (rounded up), and the filter, "area" or "bilinear" (or RESIZE_AREA / RESIZE_BILINEAR).
    ValueError, in the library's words, for what it would refuse (include/tiny_renderer.h)."""
    f = _resize_filter(filter, who)
    for v in (width, height):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 1 <= v <= RESIZE_MAX_SIDE:
            raise ValueError("%s: width and height must be 1..8192" % who)
    if src_width < 1 or src_height < 1:
        raise ValueError("%s: the source is empty" % who)
    if 8 * width < src_width or 8 * height < src_height:
        raise ValueError("%s: a side shrinks by more than 8 (width and height must be at least an eighth of the source's, rounded up)" % who)
    return ResizeParams(int(width), int(height), f, 0)


def resize_host(rgb, width, height, filter="area"):
    """tr_resize_host: the rule of Scene.resize on the host (no GPU needed), through the tables k_resize is fed.  rgb
    [H, W, 3] uint8 with row 0 = top (get_frame_buffer).  Returns the [height, width, 3] frame and leaves its argument
    alone."""
    src = np.ascontiguousarray(rgb, np.uint8)
    if src.ndim != 3 or src.shape[2] != 3:
        raise ValueError("tr_resize_host: rgb [H, W, 3]")
    p = resize_params(src.shape[1], src.shape[0], width, height, filter, "tr_resize_host")
    out = np.empty((p.height, p.width, 3), np.uint8)
    check(load_library().tr_resize_host(src.shape[1], src.shape[0], src.ctypes.data, C.addressof(p), out.ctypes.data))
    return out


def resize_taps(filter, n_src, n_dst):
    """tr_resize_taps: the tables of one axis as k_resize is fed them -- (first [n_dst], count [n_dst], weights
    [n_dst, 16]) uint16: output index X sums count[X] source samples from first[X] on under weights[X, :count[X]], which
    add up to 4096; zeros beyond."""
    f = _resize_filter(filter, "tr_resize_taps")
    if isinstance(n_dst, bool) or not isinstance(n_dst, (int, np.integer)) or not 1 <= n_dst <= RESIZE_MAX_SIDE or n_src < 1 or 8 * n_dst < n_src:
        raise ValueError("tr_resize_taps: n_dst must be 1..8192 and at least an eighth of n_src, rounded up")
    first, count = np.empty(n_dst, np.uint16), np.empty(n_dst, np.uint16)
    weights = np.empty((n_dst, RESIZE_MAX_TAPS), np.uint16)
    check(load_library().tr_resize_taps(f, int(n_src), int(n_dst), first.ctypes.data, count.ctypes.data, weights.ctypes.data))
    return first, count, weights


YUV_I420, YUV_NV12, YUV_I444, YUV_BT601, YUV_BT709, YUV_FULL, YUV_LIMITED, YUV_MAX_SIDE = 0, 1, 2, 0, 1, 0, 1, 8192   # (TR_YUV_*)
YUV_LAYOUTS = {"i420": YUV_I420, "nv12": YUV_NV12, "i444": YUV_I444}
YUV_MATRICES = {"bt601": YUV_BT601, "bt709": YUV_BT709}
YUV_RANGES = {"full": YUV_FULL, "limited": YUV_LIMITED}


class YuvParams(C.Structure):
    """tr_yuv_params"""
    _fields_ = [("layout", C.c_uint32), ("matrix", C.c_uint32), ("range", C.c_uint32), ("flags", C.c_uint32)]


def _yuv_choice(value, names, text):
    if isinstance(value, str) and value in names:
        return names[value]
    if not isinstance(value, (bool, str)) and value in names.values():
        return int(value)
    raise ValueError(text)


def yuv_params(layout="i420", matrix="bt709", range="limited", who="to_yuv"):
    """tr_yuv_params: layout "i420", "nv12" or "i444", matrix "bt601" or "bt709", range "full" or "limited" (or the
    YUV_* numbers).  ValueError, in the library's words, for what it would refuse (include/tiny_renderer.h)."""
    return YuvParams(_yuv_choice(layout, YUV_LAYOUTS, "%s: layout must be TR_YUV_I420, TR_YUV_NV12 or TR_YUV_I444" % who),
                     _yuv_choice(matrix, YUV_MATRICES, "%s: matrix must be TR_YUV_BT601 or TR_YUV_BT709" % who),
                     _yuv_choice(range, YUV_RANGES, "%s: range must be TR_YUV_FULL or TR_YUV_LIMITED" % who), 0)


def _yuv_size(width, height, who):
    for v in (width, height):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 1 <= v <= YUV_MAX_SIDE:
            raise ValueError("%s: width and height must be 1..8192" % who)
    return int(width), int(height)


def yuv_bytes(width, height, layout="i420"):
    """tr_yuv_bytes: the bytes of all planes of a width x height image (each 1..8192)."""
    w, h = _yuv_size(width, height, "tr_yuv_bytes")
    return int(load_library().tr_yuv_bytes(w, h, yuv_params(layout, who="tr_yuv_bytes").layout))


def yuv_planes(flat, width, height, layout="i420"):
    """The planes of one flat uint8 array of yuv_bytes bytes, as views into it (tr_yuv_plane): (Y [H, W], U [ch, cw],
    V [ch, cw]) for "i420", (Y [H, W], UV [ch, cw, 2]) for "nv12", (Y, U, V), each [H, W], for "i444"."""
    w, h = _yuv_size(width, height, "tr_yuv_plane")
    lay = yuv_params(layout, who="tr_yuv_plane").layout
    flat = np.asarray(flat)
    if flat.dtype != np.uint8 or flat.ndim != 1 or flat.size != yuv_bytes(w, h, lay):
        raise ValueError("tr_yuv_plane: flat must be a uint8 array of yuv_bytes(width, height, layout) bytes")
    planes = []
    for k in (0, 1) if lay == YUV_NV12 else (0, 1, 2):
        off, pw, ph, step = C.c_size_t(), C.c_uint32(), C.c_uint32(), C.c_uint32()
        check(load_library().tr_yuv_plane(w, h, lay, k, C.addressof(off), C.addressof(pw), C.addressof(ph), C.addressof(step)))
        shape = (ph.value, pw.value) if step.value == 1 else (ph.value, pw.value, step.value)
        planes.append(flat[off.value:off.value + ph.value * pw.value * step.value].reshape(shape))
    return tuple(planes)


def yuv_coefficients(matrix="bt709", range="limited"):
    """tr_yuv_coefficients: (Y row, U row, V row, y0) of a table as the library holds it, in units of 1 / 65536."""
    p = yuv_params("i420", matrix, range, "tr_yuv_coefficients")
    out = np.empty(10, np.int32)
    check(load_library().tr_yuv_coefficients(p.matrix, p.range, out.ctypes.data))
    return tuple(int(v) for v in out[0:3]), tuple(int(v) for v in out[3:6]), tuple(int(v) for v in out[6:9]), int(out[9])


def yuv_host(rgb, layout="i420", matrix="bt709", range="limited", flat=False):
    """tr_yuv_host: the rule of Scene.to_yuv on the host (no GPU needed).  rgb [H, W, 3] uint8 with row 0 = top
    (get_frame_buffer).  Returns the planes as yuv_planes gives them -- views into one flat array --, or that array
    with flat=True; leaves its argument alone."""
    src = np.ascontiguousarray(rgb, np.uint8)
    if src.ndim != 3 or src.shape[2] != 3:
        raise ValueError("tr_yuv_host: rgb [H, W, 3]")
    p = yuv_params(layout, matrix, range, "tr_yuv_host")
    w, h = _yuv_size(src.shape[1], src.shape[0], "tr_yuv_host")
    out = np.empty(yuv_bytes(w, h, p.layout), np.uint8)
    check(load_library().tr_yuv_host(w, h, src.ctypes.data, C.addressof(p), out.ctypes.data))
    return out if flat else yuv_planes(out, w, h, p.layout)


class Y4MWriter:
    """A YUV4MPEG2 file of width x height frames at `fps` frames a second (an integer, or (numerator, denominator)):
    write(frame) appends one frame, a flat array of yuv_bytes bytes or the tuple of planes yuv_planes gives.  "i420" is
    written as C420jpeg (the centred siting of the rule), "i444" as C444; the range goes into XCOLORRANGE=FULL or
    LIMITED.  "nv12" is refused: the format has no interleaved chroma."""

    def __init__(self, path, width, height, fps=30, layout="i420", range="limited"):
        lay = yuv_params(layout, who="Y4MWriter").layout
        if lay == YUV_NV12:
            raise ValueError("Y4MWriter: YUV4MPEG2 has no NV12 (interleaved chroma): use i420 or i444")
        rng = _yuv_choice(range, YUV_RANGES, "Y4MWriter: range must be TR_YUV_FULL or TR_YUV_LIMITED")
        self.width, self.height = _yuv_size(width, height, "Y4MWriter")
        num, den = (fps if isinstance(fps, (tuple, list)) else (fps, 1))
        if isinstance(num, bool) or int(num) != num or int(den) != den or num < 1 or den < 1:
            raise ValueError("Y4MWriter: fps must be a positive integer or a pair of them")
        self.layout, self.frames = lay, 0
        self.frame_bytes = yuv_bytes(self.width, self.height, lay)
        self._f = open(path, "wb")
        self._f.write(("YUV4MPEG2 W%d H%d F%d:%d Ip A1:1 %s XCOLORRANGE=%s\n"
                       % (self.width, self.height, int(num), int(den), "C420jpeg" if lay == YUV_I420 else "C444",
                          "FULL" if rng == YUV_FULL else "LIMITED")).encode("ascii"))

    def write(self, frame):
        if isinstance(frame, (tuple, list)):
            frame = np.concatenate([np.ascontiguousarray(p, np.uint8).reshape(-1) for p in frame])
        frame = np.ascontiguousarray(frame, np.uint8).reshape(-1)
        if frame.size != self.frame_bytes:
            raise ValueError("Y4MWriter: a frame is %d bytes, not %d" % (self.frame_bytes, frame.size))
        self._f.write(b"FRAME\n")
        self._f.write(frame.tobytes())
        self.frames += 1

    def close(self):
        if self._f is not None:
            self._f.close()
            self._f = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


LAYER_MODES = {"normal": 0, "add": 1, "multiply": 2, "screen": 3, "lighten": 4, "darken": 5, "difference": 6}   # (TR_LAYER_*)
LAYER_RGB8, LAYER_RGBA8, LAYER_KEY, LAYER_WHERE_DRAWN, LAYER_WHERE_UNDRAWN, LAYER_MAX_SIDE = 0, 1, 1, 2, 4, 8192
LAYER_WHERE = {None: 0, "drawn": LAYER_WHERE_DRAWN, "undrawn": LAYER_WHERE_UNDRAWN}


class LayerParams(C.Structure):
    """tr_layer_params"""
    _fields_ = [("mode", C.c_uint32), ("format", C.c_uint32), ("flags", C.c_uint32), ("opacity", C.c_uint32), ("x", C.c_int32), ("y", C.c_int32),
                ("width", C.c_uint32), ("height", C.c_uint32), ("stride", C.c_uint32), ("key", C.c_uint8 * 4)]


def layer_params(width, height, x=0, y=0, mode="normal", format="rgb8", opacity=256, where=None, key=None, stride=0, who="layer"):
    """tr_layer_params: a layer of width x height pixels (each 1..8192; both 0 for Scene.layer_from) of format "rgb8" or
    "rgba8", rows `stride` bytes apart (0: tightly packed), its top-left pixel on frame pixel (x, y) -- signed, row 0 =
    top.  mode: "normal", "add", "multiply", "screen", "lighten", "darken" or "difference"; opacity 0..256; where: None,
    "drawn" (the model only) or "undrawn" (a backdrop); key: None or (r, g, b), the layer colour that covers nothing.
    ValueError, in the library's words, for what it would refuse (include/tiny_renderer.h)."""
    for v in (width, height, x, y, opacity, stride):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError("%s: width, height, x, y, opacity and stride must be integers" % who)
    if mode not in LAYER_MODES:
        raise ValueError("%s: mode must be TR_LAYER_NORMAL .. TR_LAYER_DIFFERENCE" % who)
    if format not in ("rgb8", "rgba8"):
        raise ValueError("%s: format must be TR_LAYER_RGB8 or TR_LAYER_RGBA8" % who)
    if where not in LAYER_WHERE:
        raise ValueError("%s: where must be None, \"drawn\" or \"undrawn\"" % who)
    if not 0 <= opacity <= 256:
        raise ValueError("%s: opacity must be 0..256" % who)
    if not -2 ** 31 <= x < 2 ** 31 or not -2 ** 31 <= y < 2 ** 31:
        raise ValueError("%s: x and y must fit 32 bits" % who)
    bpp = 4 if format == "rgba8" else 3
    if (width, height, stride) != (0, 0, 0):
        if not 1 <= width <= LAYER_MAX_SIDE or not 1 <= height <= LAYER_MAX_SIDE:
            raise ValueError("%s: width and height must be 1..8192" % who)
        if stride != 0 and not width * bpp <= stride < 2 ** 32:
            raise ValueError("%s: stride must be 0 or at least the bytes of a row" % who)
    flags = LAYER_WHERE[where] | (LAYER_KEY if key is not None else 0)
    k = (C.c_uint8 * 4)(0, 0, 0, 0)
    if key is not None:
        c = [int(v) for v in key]
        if len(c) != 3 or not all(0 <= v <= 255 for v in c):
            raise ValueError("%s: key must be three values 0..255" % who)
        k = (C.c_uint8 * 4)(c[0], c[1], c[2], 0)
    return LayerParams(LAYER_MODES[mode], LAYER_RGBA8 if bpp == 4 else LAYER_RGB8, flags, int(opacity), int(x), int(y), int(width), int(height),
                       int(stride), k)


def _layer_array(image, who):
    """(format, width, height, stride) of a layer held in a uint8 array or tensor [h, w, 3 | 4] whose pixels are packed
    and whose rows lie `stride` bytes apart."""
    shape = tuple(image.shape)
    strides = tuple(image.stride()) if hasattr(image, "data_ptr") else tuple(image.strides)
    item = image.element_size() if hasattr(image, "data_ptr") else image.itemsize
    if len(shape) != 3 or shape[2] not in (3, 4) or item != 1 or shape[0] < 1 or shape[1] < 1:
        raise ValueError("%s: image must be a uint8 [h, w, 3] or [h, w, 4] array" % who)
    if strides[2] != 1 or strides[1] != shape[2] or (shape[0] > 1 and strides[0] < shape[1] * shape[2]):
        raise ValueError("%s: image must have packed pixels and rows at a non-negative stride" % who)
    return ("rgba8" if shape[2] == 4 else "rgb8"), shape[1], shape[0], (strides[0] if shape[0] > 1 else shape[1] * shape[2])


def layer_host(rgb, image, x=0, y=0, mode="normal", opacity=256, where=None, key=None, z=None, in_place=False):
    """tr_layer_host: the rule of Scene.layer on the host (no GPU needed), by the inline functions k_layer calls.  rgb
    [H, W, 3] uint8 with row 0 = top (get_frame_buffer); image [h, w, 3 | 4] uint8, its rows at any stride; z [H, W]
    float32 with row 0 = bottom (read_z_f32), needed with `where`.  Returns the layered frame and leaves its arguments
    alone; in_place=True hands the library one buffer as rgb and out (a copy of rgb), which the rule allows."""
    src = np.ascontiguousarray(rgb, np.uint8)
    if src.ndim != 3 or src.shape[2] != 3 or src.shape[0] < 1 or src.shape[1] < 1:
        raise ValueError("tr_layer_host: rgb [H, W, 3]")
    img = np.asarray(image)
    fmt, w, h, stride = _layer_array(img, "tr_layer_host")
    p = layer_params(w, h, x, y, mode, fmt, opacity, where, key, stride, "tr_layer_host")
    zz = None
    if where is not None:
        zz = np.ascontiguousarray(z, np.float32)
        if zz.shape != src.shape[:2]:
            raise ValueError("tr_layer_host: a WHERE flag needs z [H, W]")
    out = src.copy() if in_place else np.empty_like(src)
    check(load_library().tr_layer_host(src.shape[1], src.shape[0], out.ctypes.data if in_place else src.ctypes.data,
                                       None if zz is None else zz.ctypes.data, C.addressof(p), img.ctypes.data, out.ctypes.data))
    return out


def _layer_size(w, h, who):
    for v in (w, h):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 1 <= v <= LAYER_MAX_SIDE:
            raise ValueError("%s: width and height must be 1..8192" % who)
    return int(w), int(h)


def layer_gradient(w, h, top, bottom):
    """An rgb8 layer [h, w, 3] that runs from the colour `top` in row 0 to `bottom` in the last row -- a sky behind the
    model (where="undrawn").  Row r is round(top + (bottom - top) r / (h - 1)) per channel, halves up."""
    w, h = _layer_size(w, h, "layer_gradient")
    a, b = np.asarray(top, np.int64).reshape(3), np.asarray(bottom, np.int64).reshape(3)
    if a.min() < 0 or a.max() > 255 or b.min() < 0 or b.max() > 255:
        raise ValueError("layer_gradient: colours must be three values 0..255")
    r, n = np.arange(h, dtype=np.int64)[:, None], max(h - 1, 1)
    rows = (2 * (a * (n - r) + b * r) + n) // (2 * n)
    return np.ascontiguousarray(np.broadcast_to(rows[:, None, :], (h, w, 3)).astype(np.uint8))


def layer_vignette(w, h, strength):
    """A grey rgb8 mask [h, w, 3] for mode="multiply": 255 at the centre, falling with the square of the distance to
    255 - strength (0..255) in the corners."""
    w, h = _layer_size(w, h, "layer_vignette")
    if isinstance(strength, bool) or not isinstance(strength, (int, np.integer)) or not 0 <= strength <= 255:
        raise ValueError("layer_vignette: strength must be an integer 0..255")
    # in integers: the squared distance of pixel centres from the centre, in units of half pixels
    dx, dy = (2 * np.arange(w, dtype=np.int64) + 1 - w) ** 2, (2 * np.arange(h, dtype=np.int64) + 1 - h) ** 2
    d2, most = dy[:, None] * (w * w) + dx[None, :] * (h * h), 2 * (w * w) * (h * h)   # (scaled so both axes reach 1 at the edge)
    grey = 255 - (2 * int(strength) * d2 + most) // (2 * most)
    return np.ascontiguousarray(np.repeat(np.clip(grey, 0, 255).astype(np.uint8)[:, :, None], 3, axis=2))


def layer_checker(w, h, cell=8, a=(255, 255, 255), b=(0, 0, 0)):
    """An rgb8 layer [h, w, 3] of cell x cell squares that alternate between the colours a (top left) and b."""
    w, h = _layer_size(w, h, "layer_checker")
    if isinstance(cell, bool) or not isinstance(cell, (int, np.integer)) or cell < 1:
        raise ValueError("layer_checker: cell must be a positive integer")
    ca, cb = np.asarray(a, np.int64).reshape(3), np.asarray(b, np.int64).reshape(3)
    if min(ca.min(), cb.min()) < 0 or max(ca.max(), cb.max()) > 255:
        raise ValueError("layer_checker: colours must be three values 0..255")
    odd = ((np.arange(h)[:, None] // cell + np.arange(w)[None, :] // cell) % 2).astype(bool)
    return np.where(odd[:, :, None], cb.astype(np.uint8), ca.astype(np.uint8))


def layer_letterbox(w, h, bar, colour=(0, 0, 0)):
    """An rgba8 layer [h, w, 4]: `bar` rows of opaque `colour` at the top and at the bottom, transparent between."""
    w, h = _layer_size(w, h, "layer_letterbox")
    if isinstance(bar, bool) or not isinstance(bar, (int, np.integer)) or not 0 <= 2 * bar <= h:
        raise ValueError("layer_letterbox: bar must be an integer with 0 <= 2 bar <= h")
    c = np.asarray(colour, np.int64).reshape(3)
    if c.min() < 0 or c.max() > 255:
        raise ValueError("layer_letterbox: colour must be three values 0..255")
    out = np.zeros((h, w, 4), np.uint8)
    out[:, :, :3] = c.astype(np.uint8)
    out[:bar, :, 3] = 255
    out[h - bar:, :, 3] = 255
    return out


RAMP_MAX_N, RAMP_REPEAT, RAMP_NO_POSITION = 1024, 1, 0xFFFFFFFF   # (TR_RAMP_MAX_N, TR_RAMP_REPEAT; ramp_positions: not drawn)


class RampParams(C.Structure):
    """tr_ramp_params"""
    _fields_ = [("z0", C.c_float), ("scale", C.c_float), ("mode", C.c_uint32), ("opacity", C.c_uint32), ("undrawn", C.c_uint32),
                ("flags", C.c_uint32), ("reserved", C.c_uint32 * 2)]


def ramp_params(z0, scale, mode="normal", opacity=256, undrawn=(0, 0, 0, 0), repeat=False, who="ramp"):
    """tr_ramp_params for Scene.ramp / get_ramped / ramp_host / ramp_positions: a drawn pixel with depth z takes table
    position ((z - z0) * scale) as u32, in 1/256 of a table step, clamped to the last entry or, with repeat=True, wrapped;
    scale may be negative (nearer is larger: ramp_span).  mode: a layer mode; opacity 0..256; undrawn: the (r, g, b, a)
    entry of a pixel that is not drawn -- alpha 0 leaves the background alone.  ValueError, in the library's words, for
    what it would refuse (include/tiny_renderer.h)."""
    with np.errstate(over="ignore"):   # (as f32: what the library gets)
        z32, s32 = np.float32(float(z0)), np.float32(float(scale))
    if not np.isfinite(z32):
        raise ValueError("%s: z0 must be finite" % who)
    if not np.isfinite(s32) or s32 == 0.0:
        raise ValueError("%s: scale must be finite and not 0" % who)
    if mode not in LAYER_MODES:
        raise ValueError("%s: mode must be TR_LAYER_NORMAL .. TR_LAYER_DIFFERENCE" % who)
    if isinstance(opacity, bool) or not isinstance(opacity, (int, np.integer)) or not 0 <= opacity <= 256:
        raise ValueError("%s: opacity must be 0..256" % who)
    u = [int(v) for v in undrawn]
    if len(u) != 4 or not all(0 <= v <= 255 for v in u):
        raise ValueError("%s: undrawn must be four values 0..255 (r, g, b, a)" % who)
    return RampParams(float(z32), float(s32), LAYER_MODES[mode], int(opacity), u[0] | (u[1] << 8) | (u[2] << 16) | (u[3] << 24),
                      RAMP_REPEAT if repeat else 0, (C.c_uint32 * 2)(0, 0))


def _ramp_table(table, who):
    """The table of a ramp as the library takes it: a contiguous uint8 [n, 4] array, n = 2..1024."""
    if not isinstance(table, np.ndarray) or table.dtype != np.uint8 or table.ndim != 2 or table.shape[1] != 4:
        raise ValueError("%s: the table must be a uint8 array [n, 4] (r, g, b, a)" % who)
    if not 2 <= table.shape[0] <= RAMP_MAX_N:
        raise ValueError("%s: the table's length n must be 2..TR_RAMP_MAX_N" % who)
    return np.ascontiguousarray(table)


def ramp_host(rgb, z, table, params, in_place=False):
    """tr_ramp_host: the rule of Scene.ramp on the host (no GPU needed), by the inline functions k_ramp calls.  rgb
    [H, W, 3] uint8 with row 0 = top (get_frame_buffer), z [H, W] float32 with row 0 = bottom (read_z_f32), table uint8
    [n, 4], params from ramp_params.  Returns the ramped frame and leaves its arguments alone; in_place=True hands the
    library one buffer as rgb and out (a copy of rgb), which the rule allows."""
    _check_params(params, RampParams, "ramp_host", "ramp_params")
    tab = _ramp_table(table, "ramp_host")
    src = np.ascontiguousarray(rgb, np.uint8)
    zz = np.ascontiguousarray(z, np.float32)
    if src.ndim != 3 or src.shape[2] != 3 or src.shape[0] < 1 or src.shape[1] < 1 or zz.shape != src.shape[:2]:
        raise ValueError("ramp_host: rgb [H, W, 3] and z [H, W]")
    out = src.copy() if in_place else np.empty_like(src)
    check(load_library().tr_ramp_host(src.shape[1], src.shape[0], out.ctypes.data if in_place else src.ctypes.data, zz.ctypes.data,
                                      C.addressof(params), tab.shape[0], tab.ctypes.data, out.ctypes.data))
    return out


def ramp_positions(params, n, z):
    """tr_ramp_positions: the table position (uint32, z's shape; 1/256 of a step, after the clamp or the wrap) of every
    depth in z under params (ramp_params) and a table of n entries; RAMP_NO_POSITION where nothing is drawn -- for
    choosing z0 and scale."""
    _check_params(params, RampParams, "ramp_positions", "ramp_params")
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not 2 <= n <= RAMP_MAX_N:
        raise ValueError("ramp_positions: the table's length n must be 2..TR_RAMP_MAX_N")
    zz = np.ascontiguousarray(z, np.float32)
    out = np.zeros(zz.shape, np.uint32)
    check(load_library().tr_ramp_positions(C.addressof(params), int(n), zz.size, zz.ctypes.data, out.ctypes.data))
    return out


def _ramp_n(n, who):
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not 2 <= n <= RAMP_MAX_N:
        raise ValueError("%s: n must be an integer 2..%d" % (who, RAMP_MAX_N))
    return int(n)


def _ramp_colour(colour, who):
    c = [int(v) for v in colour]
    if len(c) != 3 or not all(0 <= v <= 255 for v in c):
        raise ValueError("%s: colour must be three values 0..255" % who)
    return c


def ramp_span(near, far, n):
    """(z0, scale) as np.float32 for a table of n entries that starts at the depth `near` and reaches its last entry at
    `far`: z0 = f32(near), scale = f32((n - 1) * 256 / (f32(far) - f32(near))), the quotient taken in float64.  Nearer is
    larger in this renderer, so far < near and scale < 0 for a ramp that grows with distance."""
    n = _ramp_n(n, "ramp_span")
    with np.errstate(over="ignore"):
        a, b = np.float32(float(near)), np.float32(float(far))
    if not np.isfinite(a) or not np.isfinite(b) or a == b:
        raise ValueError("ramp_span: near and far must be finite and differ")
    with np.errstate(over="ignore"):
        scale = np.float32(float((n - 1) * 256) / (float(b) - float(a)))
    if not np.isfinite(scale) or scale == 0.0:
        raise ValueError("ramp_span: the span gives no finite non-zero scale")
    return a, scale


def ramp_span_auto(scene, n=256):
    """ramp_span from the nearest to the farthest drawn depth of the scene's current frame, taken from
    Scene.get_frame_stats(depth=True) -- reduced on the device, no z is read back.  ValueError where nothing is drawn; a
    frame of one depth gets a span of one unit behind it."""
    stats = scene.get_frame_stats(depth=True)
    if stats.n_drawn == 0:
        raise ValueError("ramp_span_auto: nothing is drawn")
    near, far = np.float32(stats.z_max), np.float32(stats.z_min)
    return ramp_span(near, far if far != near else near - np.float32(1.0), n)


def ramp_fog(colour, n=256, kind="linear", density=2.0):
    """A table [n, 4] for Scene.set_ramp: `colour` everywhere, alpha 0 at entry 0 rising to 255 at the last.  kind
    "linear": alpha_k = round(255 k / (n - 1)), in integers; "exp": 1 - exp(-density t) and "exp2": 1 - exp(-(density t)^2)
    with t = k / (n - 1), each divided by its value at t = 1 and rounded to 0..255."""
    n, c = _ramp_n(n, "ramp_fog"), _ramp_colour(colour, "ramp_fog")
    k = np.arange(n, dtype=np.int64)
    if kind == "linear":
        alpha = (2 * 255 * k + (n - 1)) // (2 * (n - 1))
    elif kind in ("exp", "exp2"):
        d = float(density)
        if not np.isfinite(d) or not d > 0.0:
            raise ValueError("ramp_fog: density must be finite and > 0")
        t = k.astype(np.float64) / float(n - 1)
        x = d * t if kind == "exp" else (d * t) ** 2
        a = -np.expm1(-x)
        alpha = np.floor(255.0 * a / a[-1] + 0.5).astype(np.int64)
        alpha[0], alpha[-1] = 0, 255
        alpha = np.maximum.accumulate(alpha)
    else:
        raise ValueError("ramp_fog: kind must be \"linear\", \"exp\" or \"exp2\"")
    out = np.empty((n, 4), np.uint8)
    out[:, :3] = c
    out[:, 3] = np.clip(alpha, 0, 255)
    return out


def ramp_grey(n=256):
    """An opaque table [n, 4] from black at entry 0 to white at the last: a grey depth view under mode "normal"."""
    n = _ramp_n(n, "ramp_grey")
    k = np.arange(n, dtype=np.int64)
    out = np.full((n, 4), 255, np.uint8)
    out[:, :3] = ((2 * 255 * k + (n - 1)) // (2 * (n - 1)))[:, None]
    return out


def ramp_false_colour(n=256):
    """An opaque table [n, 4] through blue, cyan, green, yellow and red: a false-colour depth view."""
    n = _ramp_n(n, "ramp_false_colour")
    anchors = np.array([[0, 0, 160], [0, 0, 255], [0, 255, 255], [0, 255, 0], [255, 255, 0], [255, 0, 0], [160, 0, 0]], np.int64)
    m = len(anchors) - 1
    pos = np.arange(n, dtype=np.int64) * m                 # in units of 1 / (n - 1) of a segment
    seg = np.minimum(pos // (n - 1), m - 1)
    f = pos - seg * (n - 1)
    out = np.full((n, 4), 255, np.uint8)
    out[:, :3] = (2 * (anchors[seg] * (n - 1 - f)[:, None] + anchors[seg + 1] * f[:, None]) + (n - 1)) // (2 * (n - 1))
    return out


def ramp_contours(n, every, colour=(0, 0, 0)):
    """A table [n, 4] of `colour`: opaque at every `every`-th entry from entry 0, transparent between -- contour bands."""
    n, c = _ramp_n(n, "ramp_contours"), _ramp_colour(colour, "ramp_contours")
    if isinstance(every, bool) or not isinstance(every, (int, np.integer)) or every < 1:
        raise ValueError("ramp_contours: every must be a positive integer")
    out = np.zeros((n, 4), np.uint8)
    out[:, :3] = c
    out[::int(every), 3] = 255
    return out


def ramp_slice(n, lo, hi, colour=(255, 255, 255)):
    """A table [n, 4] of `colour`: opaque at the entries lo <= k < hi, transparent elsewhere -- a depth slice or matte."""
    n, c = _ramp_n(n, "ramp_slice"), _ramp_colour(colour, "ramp_slice")
    for v in (lo, hi):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError("ramp_slice: lo and hi must be integers")
    if not 0 <= lo < hi <= n:
        raise ValueError("ramp_slice: 0 <= lo < hi <= n")
    out = np.zeros((n, 4), np.uint8)
    out[:, :3] = c
    out[int(lo):int(hi), 3] = 255
    return out


LINES_MAX_N, LINES_MAX_WIDTH, LINES_DEPTH_TEST, LINES_PAINTER, LINES_COORD_MAX = 1 << 20, 15, 1, 2, 1 << 20   # (TR_LINES_*)
# tr_line as a numpy record: 32 bytes
LINE_DTYPE = np.dtype([("x0", "<i4"), ("y0", "<i4"), ("z0", "<f4"), ("x1", "<i4"), ("y1", "<i4"), ("z1", "<f4"), ("rgba", "u1", (4,)), ("reserved", "<u4")])


class LinesParams(C.Structure):
    """tr_lines_params"""
    _fields_ = [("width", C.c_uint32), ("opacity", C.c_uint32), ("flags", C.c_uint32), ("depth_bias", C.c_float), ("reserved", C.c_uint32 * 4)]


def lines_params(width=1, opacity=256, depth_test=True, painter=False, depth_bias=0.0, who="lines"):
    """tr_lines_params for Scene.lines / get_lined / lines_host: width 1..15 pixels across the minor axis, opacity 0..256,
    depth_test: a candidate survives iff !(z + depth_bias <= zbuf); painter: the greatest segment index wins whatever its
    depth; depth_bias: added to every step's depth (nearer is larger: > 0 lifts a line off its surface).  ValueError, in
    the library's words, for what it would refuse (include/tiny_renderer.h)."""
    if isinstance(width, bool) or not isinstance(width, (int, np.integer)) or not 1 <= width <= LINES_MAX_WIDTH:
        raise ValueError("%s: width must be 1..15" % who)
    if isinstance(opacity, bool) or not isinstance(opacity, (int, np.integer)) or not 0 <= opacity <= 256:
        raise ValueError("%s: opacity must be 0..256" % who)
    with np.errstate(over="ignore"):
        b32 = np.float32(float(depth_bias))
    if not np.isfinite(b32):
        raise ValueError("%s: depth_bias must be finite" % who)
    return LinesParams(int(width), int(opacity), (LINES_DEPTH_TEST if depth_test else 0) | (LINES_PAINTER if painter else 0), float(b32),
                       (C.c_uint32 * 4)(0, 0, 0, 0))


def _lines_table(lines, who):
    """A table of segments as the library takes it: a contiguous LINE_DTYPE array of 0..2^20 records."""
    if not isinstance(lines, np.ndarray) or lines.dtype != LINE_DTYPE or lines.ndim != 1:
        raise ValueError("%s: the table must be a one-dimensional array of LINE_DTYPE records (lines_table builds one)" % who)
    if lines.shape[0] > LINES_MAX_N:
        raise ValueError("%s: the table's length n must be 0..TR_LINES_MAX_N" % who)
    return np.ascontiguousarray(lines)


def lines_table(xy0, z0, xy1, z1, colour=(255, 255, 255, 255)):
    """A table for Scene.set_lines / lines_host from endpoints in raster coordinates (x right, y UP, what Scene.project
    gives): xy0, xy1 integer [n, 2], z0, z1 float [n]; colour: one (r, g, b[, a]) or an [n, 3 or 4] array."""
    a, b = np.asarray(xy0), np.asarray(xy1)
    if a.ndim != 2 or a.shape[1] != 2 or b.shape != a.shape:
        raise ValueError("lines_table: xy0 and xy1 are [n, 2]")
    n = a.shape[0]
    za, zb = np.asarray(z0, np.float32).reshape(-1), np.asarray(z1, np.float32).reshape(-1)
    if za.shape[0] != n or zb.shape[0] != n:
        raise ValueError("lines_table: z0 and z1 are [n]")
    c = np.asarray(colour)
    if c.ndim == 1:
        c = np.broadcast_to(c, (n, c.shape[0]))
    if c.ndim != 2 or c.shape[0] != n or c.shape[1] not in (3, 4) or (c.size and (c.min() < 0 or c.max() > 255)):
        raise ValueError("lines_table: colour is (r, g, b[, a]) or [n, 3 or 4] with values 0..255")
    t = np.zeros(n, LINE_DTYPE)
    t["x0"], t["y0"], t["z0"], t["x1"], t["y1"], t["z1"] = a[:, 0], a[:, 1], za, b[:, 0], b[:, 1], zb
    t["rgba"][:, :c.shape[1]] = c
    if c.shape[1] == 3:
        t["rgba"][:, 3] = 255
    return t


def lines_host(rgb, z, lines, params, in_place=False):
    """tr_lines_host: the rule of Scene.lines on the host (no GPU needed), by the inline functions k_lines calls.  rgb
    [H, W, 3] uint8 with row 0 = top (get_frame_buffer), z [H, W] float32 with row 0 = bottom (read_z_f32; None is allowed
    without the depth test), lines a LINE_DTYPE array, params from lines_params.  Returns the frame with the lines and
    leaves its arguments alone; in_place=True hands the library one buffer as rgb and out, which the rule allows."""
    _check_params(params, LinesParams, "lines_host", "lines_params")
    tab = _lines_table(lines, "lines_host")
    src = np.ascontiguousarray(rgb, np.uint8)
    if src.ndim != 3 or src.shape[2] != 3 or src.shape[0] < 1 or src.shape[1] < 1:
        raise ValueError("lines_host: rgb [H, W, 3] and z [H, W]")
    zz = None
    if z is not None:
        zz = np.ascontiguousarray(z, np.float32)
        if zz.shape != src.shape[:2]:
            raise ValueError("lines_host: rgb [H, W, 3] and z [H, W]")
    out = src.copy() if in_place else np.empty_like(src)
    check(load_library().tr_lines_host(src.shape[1], src.shape[0], out.ctypes.data if in_place else src.ctypes.data,
                                       zz.ctypes.data if zz is not None else None, C.addressof(params), tab.shape[0],
                                       tab.ctypes.data if tab.shape[0] else None, out.ctypes.data))
    return out


def project_points(uniforms, points):
    """tr_project_points: model-space points [n, 3] through uniforms.vpmv (prepare_uniforms) exactly as the draw chain
    transforms a vertex.  Returns (xy int32 [n, 2], z float32 [n], ok bool [n]): the pixel (x right, y up) and the depth
    the renderer gives a mesh vertex there; ok is False where w is 0 or the point leaves what a tr_line may hold."""
    p = np.ascontiguousarray(points, np.float32)
    if p.ndim != 2 or p.shape[1] != 3:
        raise ValueError("project_points: points are [n, 3]")
    n = p.shape[0]
    xy, z, ok = np.zeros((n, 2), np.int32), np.zeros(n, np.float32), np.zeros(n, np.uint8)
    check(load_library().tr_project_points(C.byref(uniforms), n, p.ctypes.data, xy.ctypes.data, z.ctypes.data, ok.ctypes.data))
    return xy, z, ok.astype(bool)


PROJECTOR_MAX_SIDE, PROJECTOR_OCCLUDE, PROJECTOR_SOFT = 8192, 1, 2   # (TR_PROJECTOR_MAX_SIDE, TR_PROJECTOR_OCCLUDE, TR_PROJECTOR_SOFT)


class ProjectorParams(C.Structure):
    """tr_projector_params"""
    _fields_ = [("m", C.c_float * 16), ("pw", C.c_uint32), ("ph", C.c_uint32), ("channels", C.c_uint32), ("mode", C.c_uint32),
                ("opacity", C.c_uint32), ("flags", C.c_uint32), ("depth_bias", C.c_float), ("reserved", C.c_uint32 * 9)]


def projector_params(m, pw, ph, channels=3, mode="add", opacity=256, occlude=False, soft=False, depth_bias=0.0, who="projector"):
    """tr_projector_params for Scene.projector / get_projector / projector_host: m, 16 floats column-major (or a [4, 4]
    array indexed [row, column]), maps frame raster (x, y, z, 1) -- y up -- to the projector's raster (projector_matrix
    builds it from two cameras); the image is pw x ph pixels (each 1..8192) of 3 or 4 channels; mode: a layer mode;
    opacity 0..256; occlude: shadow by an occluder's depth, soft: filter that shadow over 2 x 2 texels; depth_bias is
    added to the pixel's depth before the test (nearer is larger: > 0 lifts).  ValueError, in the library's words, for what
    it would refuse (include/tiny_renderer.h)."""
    mm = np.asarray(m, np.float64)
    if mm.shape == (4, 4):
        mm = mm.T.reshape(16)   # ([row, column] to column-major)
    if mm.shape != (16,):
        raise ValueError("%s: m must be 16 values (column-major) or a [4, 4] array" % who)
    with np.errstate(over="ignore"):
        m32, b32 = mm.astype(np.float32), np.float32(float(depth_bias))
    for v in (pw, ph, channels, opacity):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError("%s: pw, ph, channels and opacity must be integers" % who)
    if not 1 <= pw <= PROJECTOR_MAX_SIDE or not 1 <= ph <= PROJECTOR_MAX_SIDE:
        raise ValueError("%s: pw and ph must be 1..8192" % who)
    if channels not in (3, 4):
        raise ValueError("%s: channels must be 3 or 4" % who)
    if mode not in LAYER_MODES:
        raise ValueError("%s: mode must be TR_LAYER_NORMAL .. TR_LAYER_DIFFERENCE" % who)
    if soft and not occlude:
        raise ValueError("%s: TR_PROJECTOR_SOFT needs TR_PROJECTOR_OCCLUDE" % who)
    if not 0 <= opacity <= 256:
        raise ValueError("%s: opacity must be 0..256" % who)
    if not np.isfinite(b32):
        raise ValueError("%s: depth_bias must be finite" % who)
    if not np.isfinite(m32).all():
        raise ValueError("%s: every entry of m must be finite" % who)
    return ProjectorParams((C.c_float * 16)(*[float(v) for v in m32]), int(pw), int(ph), int(channels), LAYER_MODES[mode], int(opacity),
                           (PROJECTOR_OCCLUDE if occlude else 0) | (PROJECTOR_SOFT if soft else 0), float(b32), (C.c_uint32 * 9)(*([0] * 9)))


def projector_matrix(view_uniforms, projector_uniforms):
    """tr_projector_matrix: the 16 floats (column-major) of projector.vpmv * view.i_vpmv, accumulated in double and rounded
    once -- frame raster to projector raster for two prepare_uniforms results, the frame's camera at W x H (kind 2: it
    fills i_vpmv) and the projector's at pw x ph (kind 0)."""
    m = np.zeros(16, np.float32)
    check(load_library().tr_projector_matrix(C.byref(view_uniforms), C.byref(projector_uniforms), m.ctypes.data))
    return m


def projector_host(rgb, z, params, image, occluder_z=None, in_place=False):
    """tr_projector_host: the rule of Scene.projector on the host (no GPU needed), by the inline functions k_projector
    calls.  rgb [H, W, 3] uint8 with row 0 = top (get_frame_buffer), z [H, W] float32 with row 0 = bottom (read_z_f32),
    params from projector_params, image [ph, pw, 3 | 4] uint8 with its rows at any stride, occluder_z [ph, pw] float32
    with row 0 = bottom (the projector scene's read_z_f32) under occlude.  Returns the frame with the image cast on it and
    leaves its arguments alone; in_place=True hands the library one buffer as rgb and out, which the rule allows."""
    _check_params(params, ProjectorParams, "projector_host", "projector_params")
    src = np.ascontiguousarray(rgb, np.uint8)
    zz = np.ascontiguousarray(z, np.float32)
    if src.ndim != 3 or src.shape[2] != 3 or src.shape[0] < 1 or src.shape[1] < 1 or zz.shape != src.shape[:2]:
        raise ValueError("projector_host: rgb [H, W, 3] and z [H, W]")
    img = np.asarray(image)
    fmt, w, h, stride = _layer_array(img, "projector_host")
    if (w, h, 4 if fmt == "rgba8" else 3) != (params.pw, params.ph, params.channels):
        raise ValueError("projector_host: image must be [ph, pw, channels] of the params")
    oz = None
    if occluder_z is not None:
        oz = np.ascontiguousarray(occluder_z, np.float32)
        if oz.shape != (params.ph, params.pw):
            raise ValueError("projector_host: occluder_z [ph, pw]")
    out = src.copy() if in_place else np.empty_like(src)
    check(load_library().tr_projector_host(src.shape[1], src.shape[0], out.ctypes.data if in_place else src.ctypes.data, zz.ctypes.data,
                                           C.addressof(params), img.ctypes.data, stride, None if oz is None else oz.ctypes.data, out.ctypes.data))
    return out


RELIGHT_MAX_LIGHTS, RELIGHT_ALBEDO, RELIGHT_SHOW_NORMALS = 8, 1, 2   # (TR_RELIGHT_MAX_LIGHTS, TR_RELIGHT_ALBEDO, TR_RELIGHT_SHOW_NORMALS)
LIGHT_KINDS = {"directional": 0, "point": 1, "spot": 2}                # (TR_LIGHT_*)


class Light(C.Structure):
    """tr_light"""
    _fields_ = [("kind", C.c_uint32), ("pos", C.c_float * 3), ("dir", C.c_float * 3), ("colour", C.c_uint8 * 4), ("intensity", C.c_float),
                ("falloff", C.c_float), ("cos_outer", C.c_float), ("cone_scale", C.c_float), ("specular", C.c_float),
                ("shininess_log2", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class RelightParams(C.Structure):
    """tr_relight_params"""
    _fields_ = [("u", C.c_float * 16), ("eye", C.c_float * 3), ("ambient", C.c_uint8 * 4), ("mode", C.c_uint32), ("opacity", C.c_uint32),
                ("flags", C.c_uint32), ("reserved", C.c_uint32 * 9)]


def _light(kind, pos, direction, colour, intensity, falloff, cos_outer, cone_scale, specular, shininess_log2, who):
    """A checked tr_light: ValueError, in the library's words, for what it would refuse."""
    with np.errstate(over="ignore"):
        f = np.array(list(pos) + list(direction) + [intensity, falloff, cos_outer, cone_scale, specular], np.float64).astype(np.float32)
    if f.shape != (11,) or not np.isfinite(f).all():
        raise ValueError("%s: every float must be finite" % who)
    if isinstance(shininess_log2, bool) or not isinstance(shininess_log2, (int, np.integer)):
        raise ValueError("%s: shininess_log2 must be an integer" % who)
    col = [int(v) for v in colour]
    if len(col) != 3 or min(col) < 0 or max(col) > 255:
        raise ValueError("%s: colour takes three values 0..255" % who)
    if f[6] < 0:
        raise ValueError("%s: intensity must be >= 0" % who)
    if f[7] < 0:
        raise ValueError("%s: falloff must be >= 0" % who)
    if f[10] < 0:
        raise ValueError("%s: specular must be >= 0" % who)
    if kind == LIGHT_KINDS["spot"] and not f[9] > 0:
        raise ValueError("%s: cone_scale must be > 0" % who)
    if not 0 <= shininess_log2 <= 10:
        raise ValueError("%s: shininess_log2 must be 0..10" % who)
    return Light(kind, (C.c_float * 3)(*[float(v) for v in f[0:3]]), (C.c_float * 3)(*[float(v) for v in f[3:6]]), (C.c_uint8 * 4)(*col, 0),
                 float(f[6]), float(f[7]), float(f[8]), float(f[9]), float(f[10]), int(shininess_log2), (C.c_uint32 * 2)(0, 0))


def _unit3(v, who, what):
    """v / |v| in double, for the builders: the rule takes direction and axis vectors as given."""
    a = np.asarray(v, np.float64)
    n = float(np.sqrt((a * a).sum())) if a.shape == (3,) else 0.0
    if a.shape != (3,) or not np.isfinite(n) or n == 0.0:
        raise ValueError("%s: %s must be three finite values, not all 0" % (who, what))
    return a / n


def light_directional(direction, colour=(255, 255, 255), intensity=1.0, specular=0.0, shininess_log2=0):
    """A TR_LIGHT_DIRECTIONAL tr_light: `direction` points TOWARDS the light (normalised here), in model space."""
    return _light(0, (0.0, 0.0, 0.0), _unit3(direction, "light_directional", "direction"), colour, intensity, 0.0, 0.0, 0.0, specular, shininess_log2,
                  "light_directional")


def light_point(pos, colour=(255, 255, 255), intensity=1.0, falloff=0.0, specular=0.0, shininess_log2=0):
    """A TR_LIGHT_POINT tr_light at `pos` (model space): att = 1 / (1 + falloff * distance^2)."""
    return _light(1, pos, (0.0, 0.0, 0.0), colour, intensity, falloff, 0.0, 0.0, specular, shininess_log2, "light_point")


def light_spot(pos, at, inner_deg, outer_deg, colour=(255, 255, 255), intensity=1.0, falloff=0.0, specular=0.0, shininess_log2=0):
    """A TR_LIGHT_SPOT tr_light at `pos` shining towards `at` (model space): full inside the half angle inner_deg, none
    outside outer_deg, a linear ramp in the cosine between; 0 <= inner_deg < outer_deg <= 90."""
    if not 0.0 <= float(inner_deg) < float(outer_deg) <= 90.0:
        raise ValueError("light_spot: 0 <= inner_deg < outer_deg <= 90")
    axis = _unit3(np.asarray(at, np.float64) - np.asarray(pos, np.float64), "light_spot", "at - pos")
    ci, co = np.cos(np.radians(float(inner_deg))), np.cos(np.radians(float(outer_deg)))
    return _light(2, pos, axis, colour, intensity, falloff, co, 1.0 / (ci - co), specular, shininess_log2, "light_spot")


def relight_params(uniforms, eye, ambient=(0, 0, 0), mode="add", opacity=256, albedo=None, show_normals=False, who="relight"):
    """tr_relight_params for Scene.relight / get_relit / relight_host / relight_normals_host.  uniforms: the view's
    Uniforms from prepare_uniforms(2, W, H, ..) -- kind 2 fills i_vpmv, frame raster to model space --, or that matrix
    itself as 16 floats column-major or a [4, 4] array indexed [row, column].  eye: the camera's position in model space
    (for prepare_uniforms' camera: look_from + 5 * camera_direction).  ambient: r, g, b; mode: a layer mode; opacity
    0..256; albedo: multiply the light by the pixel's own colour first (default: on under "add", off otherwise);
    show_normals: the normal map instead of the lights.  ValueError, in the library's words, for what it would refuse."""
    if isinstance(uniforms, _lib.Uniforms):
        mm = np.array(list(uniforms.i_vpmv), np.float64)
        if not mm.any():
            raise ValueError("%s: uniforms.i_vpmv is all zeros (prepare_uniforms kind 2 fills it)" % who)
    else:
        mm = np.asarray(uniforms, np.float64)
        if mm.shape == (4, 4):
            mm = mm.T.reshape(16)   # ([row, column] to column-major)
    if mm.shape != (16,):
        raise ValueError("%s: u must be Uniforms, 16 values (column-major) or a [4, 4] array" % who)
    with np.errstate(over="ignore"):
        u32, e32 = mm.astype(np.float32), np.asarray(eye, np.float64).astype(np.float32)
    if isinstance(opacity, bool) or not isinstance(opacity, (int, np.integer)):
        raise ValueError("%s: opacity must be an integer" % who)
    if mode not in LAYER_MODES:
        raise ValueError("%s: mode must be TR_LAYER_NORMAL .. TR_LAYER_DIFFERENCE" % who)
    if not 0 <= opacity <= 256:
        raise ValueError("%s: opacity must be 0..256" % who)
    if not np.isfinite(u32).all():
        raise ValueError("%s: every entry of u must be finite" % who)
    if e32.shape != (3,) or not np.isfinite(e32).all():
        raise ValueError("%s: every entry of eye must be finite" % who)
    amb = [int(v) for v in ambient]
    if len(amb) != 3 or min(amb) < 0 or max(amb) > 255:
        raise ValueError("%s: ambient takes three values 0..255" % who)
    if albedo is None:
        albedo = mode == "add"
    return RelightParams((C.c_float * 16)(*[float(v) for v in u32]), (C.c_float * 3)(*[float(v) for v in e32]), (C.c_uint8 * 4)(*amb, 0),
                         LAYER_MODES[mode], int(opacity), (RELIGHT_ALBEDO if albedo else 0) | (RELIGHT_SHOW_NORMALS if show_normals else 0),
                         (C.c_uint32 * 9)(*([0] * 9)))


def _light_table(lights, who):
    """(ctypes array or None, n) of a sequence of Light."""
    ls = list(lights) if lights is not None else []
    for l in ls:
        if not isinstance(l, Light):
            raise ValueError("%s: lights must come from light_directional, light_point or light_spot" % who)
    if len(ls) > RELIGHT_MAX_LIGHTS:
        raise ValueError("%s: n_lights must be 0..TR_RELIGHT_MAX_LIGHTS" % who)
    return ((Light * len(ls))(*ls) if ls else None), len(ls)


def relight_host(rgb, z, params, lights=(), in_place=False):
    """tr_relight_host: the rule of Scene.relight on the host (no GPU needed), by the inline functions k_relight calls.
    rgb [H, W, 3] uint8 with row 0 = top (get_frame_buffer), z [H, W] float32 with row 0 = bottom (read_z_f32), params
    from relight_params, lights: up to 8 from light_directional / light_point / light_spot.  Returns the lit frame and
    leaves its arguments alone; in_place=True hands the library one buffer as rgb and out, which the rule allows."""
    _check_params(params, RelightParams, "relight_host", "relight_params")
    table, n = _light_table(lights, "relight_host")
    src = np.ascontiguousarray(rgb, np.uint8)
    zz = np.ascontiguousarray(z, np.float32)
    if src.ndim != 3 or src.shape[2] != 3 or src.shape[0] < 1 or src.shape[1] < 1 or zz.shape != src.shape[:2]:
        raise ValueError("relight_host: rgb [H, W, 3] and z [H, W]")
    out = src.copy() if in_place else np.empty_like(src)
    check(load_library().tr_relight_host(src.shape[1], src.shape[0], out.ctypes.data if in_place else src.ctypes.data, zz.ctypes.data,
                                         C.addressof(params), table, n, out.ctypes.data))
    return out


def relight_normals_host(z, params):
    """tr_relight_normals_host: the normals the rule recovers from a depth array, on the host.  z [H, W] float32 with row
    0 = bottom (read_z_f32); of params (relight_params) u and eye count.  Returns (normals [H, W, 3] float32, valid [H, W]
    bool), both with row 0 = bottom like z; a pixel without a normal has zeros."""
    _check_params(params, RelightParams, "relight_normals_host", "relight_params")
    zz = np.ascontiguousarray(z, np.float32)
    if zz.ndim != 2 or zz.shape[0] < 1 or zz.shape[1] < 1:
        raise ValueError("relight_normals_host: z [H, W]")
    normals, valid = np.empty(zz.shape + (3,), np.float32), np.empty(zz.shape, np.uint8)
    check(load_library().tr_relight_normals_host(zz.shape[1], zz.shape[0], zz.ctypes.data, C.addressof(params), normals.ctypes.data, valid.ctypes.data))
    return normals, valid.astype(bool)


def mesh_edges(mesh):
    """The unique edges of a mesh's faces as position-index pairs [m, 2] (int64, the smaller index first, sorted)."""
    idx = np.asarray(mesh["idx"]).astype(np.int64)
    p = idx[:, (0, 3, 6)]
    e = np.concatenate([p[:, (0, 1)], p[:, (1, 2)], p[:, (2, 0)]])
    e = np.sort(e, axis=1)
    return np.unique(e[e[:, 0] != e[:, 1]], axis=0)


def wireframe_lines(scene, mesh, colour=(255, 255, 255, 255)):
    """The mesh's unique edges projected by the scene's last camera (Scene.project) as a table for Scene.set_lines; an
    edge with an endpoint that is not ok is dropped."""
    e = mesh_edges(mesh)
    xy, z, ok = scene.project(np.asarray(mesh["pos"], np.float32))
    e = e[ok[e[:, 0]] & ok[e[:, 1]]]
    return lines_table(xy[e[:, 0]], z[e[:, 0]], xy[e[:, 1]], z[e[:, 1]], colour)


def lines_polyline(points, closed=False):
    """Model-space endpoints (a [m, 3], b [m, 3]) of the segments joining consecutive points [n, 3]."""
    p = np.asarray(points, np.float32)
    if p.ndim != 2 or p.shape[1] != 3 or p.shape[0] < 2:
        raise ValueError("lines_polyline: points are [n, 3], n >= 2")
    return (p.copy(), np.roll(p, -1, axis=0)) if closed else (p[:-1].copy(), p[1:].copy())


def lines_box(lo, hi):
    """Model-space endpoints (a [12, 3], b [12, 3]) of the twelve edges of the box from corner lo to corner hi."""
    lo, hi = np.asarray(lo, np.float32).reshape(3), np.asarray(hi, np.float32).reshape(3)
    c = np.array([[(hi if (k >> d) & 1 else lo)[d] for d in range(3)] for k in range(8)], np.float32)
    pairs = [(k, k | (1 << d)) for k in range(8) for d in range(3) if not (k >> d) & 1]
    return c[[p[0] for p in pairs]], c[[p[1] for p in pairs]]


def lines_axes(length=1.0):
    """Model-space endpoints (a [3, 3], b [3, 3]) of the three axes from the origin; colour them red, green, blue."""
    return np.zeros((3, 3), np.float32), (np.eye(3) * float(length)).astype(np.float32)


def lines_grid(n, step=1.0, y=0.0):
    """Model-space endpoints (a [2 (2 n + 1), 3], b) of a ground grid in the plane at height y: 2 n + 1 lines each way,
    `step` apart, centred on the origin."""
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 1:
        raise ValueError("lines_grid: n must be a positive integer")
    t = np.arange(-n, n + 1, dtype=np.float32) * np.float32(step)
    e, yy = np.full_like(t, n * np.float32(step)), np.full_like(t, np.float32(y))
    a = np.concatenate([np.stack([t, yy, -e], 1), np.stack([-e, yy, t], 1)])
    b = np.concatenate([np.stack([t, yy, e], 1), np.stack([e, yy, t], 1)])
    return a, b


DIST_SEEDS = {"drawn": 0, "key": 1}   # (TR_DIST_SEED_*)
DIST_INVERT, DIST_REPEAT, DIST_KEEP_SEEDS, DIST_MAX_RADIUS, DIST_FAR = 1, 1, 2, 255, 0xFFFF   # (TR_DIST_*)


class DistanceParams(C.Structure):
    """tr_distance_params"""
    _fields_ = [("seed", C.c_uint32), ("threshold", C.c_uint32), ("radius", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32 * 4)]


class DistanceRampParams(C.Structure):
    """tr_distance_ramp_params"""
    _fields_ = [("field", DistanceParams), ("step", C.c_uint32), ("mode", C.c_uint32), ("opacity", C.c_uint32), ("far", C.c_uint32),
                ("flags", C.c_uint32), ("reserved", C.c_uint32 * 3)]


def _dist_int(v, lo, hi, text):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
        raise ValueError(text)
    return int(v)


def distance_params(radius, seed="drawn", threshold=0, invert=False, who="distance"):
    """tr_distance_params for Scene.distance / get_distance / distance_host: the squared distance of every pixel to the
    nearest seed, kept up to radius (1..255) squared, DIST_FAR beyond.  seed "drawn": a pixel with a depth; "key": a pixel
    whose largest stored channel is >= threshold (0..255).  invert=True: the complement -- the distance inside a shape to
    its border.  ValueError, in the library's words, for what it would refuse (include/tiny_renderer.h)."""
    if seed not in DIST_SEEDS:
        raise ValueError("%s: seed must be TR_DIST_SEED_DRAWN or TR_DIST_SEED_KEY" % who)
    t = _dist_int(threshold, 0, 255, "%s: threshold must be 0..255" % who)
    r = _dist_int(radius, 1, DIST_MAX_RADIUS, "%s: radius must be 1..TR_DIST_MAX_RADIUS" % who)
    return DistanceParams(DIST_SEEDS[seed], t, r, DIST_INVERT if invert else 0, (C.c_uint32 * 4)(0, 0, 0, 0))


def distance_ramp_params(radius, step=256, seed="drawn", threshold=0, invert=False, mode="normal", opacity=256, far=(0, 0, 0, 0), repeat=False,
                         keep_seeds=False, who="distance_ramp"):
    """tr_distance_ramp_params for Scene.distance_ramp / get_distance_ramped / distance_ramp_host: distance_params, and
    for the ramp step (1..65536 table positions, 1/256 of an entry, per pixel of distance: 256 is one entry a pixel), a
    layer mode, opacity 0..256, the (r, g, b, a) entry `far` of a pixel beyond the radius, repeat (the position wraps)
    and keep_seeds (a seed keeps its colour)."""
    f = distance_params(radius, seed, threshold, invert, who)
    st = _dist_int(step, 1, 65536, "%s: step must be 1..65536" % who)
    if mode not in LAYER_MODES:
        raise ValueError("%s: mode must be TR_LAYER_NORMAL .. TR_LAYER_DIFFERENCE" % who)
    op = _dist_int(opacity, 0, 256, "%s: opacity must be 0..256" % who)
    u = [int(v) for v in far]
    if len(u) != 4 or not all(0 <= v <= 255 for v in u):
        raise ValueError("%s: far must be four values 0..255 (r, g, b, a)" % who)
    return DistanceRampParams(f, st, LAYER_MODES[mode], op, u[0] | (u[1] << 8) | (u[2] << 16) | (u[3] << 24),
                              (DIST_REPEAT if repeat else 0) | (DIST_KEEP_SEEDS if keep_seeds else 0), (C.c_uint32 * 3)(0, 0, 0))


def _dist_frame(rgb, z, seed_is_key, who):
    src = np.ascontiguousarray(rgb, np.uint8)
    if src.ndim != 3 or src.shape[2] != 3 or src.shape[0] < 1 or src.shape[1] < 1:
        raise ValueError("%s: rgb [H, W, 3] and z [H, W]" % who)
    if z is None:
        if not seed_is_key:
            raise ValueError("%s: z may be None under seed \"key\" only" % who)
        return src, None
    zz = np.ascontiguousarray(z, np.float32)
    if zz.shape != src.shape[:2]:
        raise ValueError("%s: rgb [H, W, 3] and z [H, W]" % who)
    return src, zz


def distance_host(rgb, z, params):
    """tr_distance_host: the rule of Scene.distance on the host (no GPU needed), by the inline functions the kernels
    call.  rgb [H, W, 3] uint8 with row 0 = top (get_frame_buffer), z [H, W] float32 with row 0 = bottom (read_z_f32) or
    None under seed "key", params from distance_params.  Returns the field, uint16 [H, W] with row 0 = top."""
    _check_params(params, DistanceParams, "distance_host", "distance_params")
    src, zz = _dist_frame(rgb, z, params.seed == DIST_SEEDS["key"], "distance_host")
    out = np.empty(src.shape[:2], np.uint16)
    check(load_library().tr_distance_host(src.shape[1], src.shape[0], src.ctypes.data, None if zz is None else zz.ctypes.data,
                                          C.addressof(params), out.ctypes.data))
    return out


def distance_ramp_host(rgb, z, table, params, in_place=False):
    """tr_distance_ramp_host: the rule of Scene.distance_ramp on the host (no GPU needed).  Arguments as for distance_host,
    table uint8 [n, 4], params from distance_ramp_params.  Returns the ramped frame; in_place=True hands the library one
    buffer as rgb and out (a copy of rgb), which the rule allows."""
    _check_params(params, DistanceRampParams, "distance_ramp_host", "distance_ramp_params")
    tab = _ramp_table(table, "distance_ramp_host")
    src, zz = _dist_frame(rgb, z, params.field.seed == DIST_SEEDS["key"], "distance_ramp_host")
    out = src.copy() if in_place else np.empty_like(src)
    check(load_library().tr_distance_ramp_host(src.shape[1], src.shape[0], out.ctypes.data if in_place else src.ctypes.data,
                                               None if zz is None else zz.ctypes.data, C.addressof(params), tab.shape[0], tab.ctypes.data,
                                               out.ctypes.data))
    return out


def distance_positions(d2, step=256):
    """tr_distance_positions: (dq, p) as uint32 arrays of d2's shape -- dq = floor(sqrt(d2 * 65536)), the distance in 1/256
    of a pixel, and p = (dq * step) >> 8, the table position before the clamp or the wrap -- of field values <= 65025."""
    dd = np.ascontiguousarray(d2, np.uint16)
    dq, p = np.zeros(dd.shape, np.uint32), np.zeros(dd.shape, np.uint32)
    check(load_library().tr_distance_positions(int(step), dd.size, dd.ctypes.data, dq.ctypes.data, p.ctypes.data))
    return dq, p


def _dist_rgba(colour, who):
    c = [int(v) for v in colour]
    if len(c) == 3:
        c.append(255)
    if len(c) != 4 or not all(0 <= v <= 255 for v in c):
        raise ValueError("%s: colour must be three or four values 0..255" % who)
    return c


def ramp_glow(colour, radius, falloff="linear"):
    """(table, step) for Scene.set_ramp and Scene.distance_ramp: a glow of `colour` (r, g, b[, a]) that is strongest at
    the seeds and gone `radius` pixels (1..255) away.  256 entries over the radius; alpha falls from the colour's to 0 by
    falloff "linear" (1 - t), "smooth" ((1 - t)^2) or "exp" (exp(-4 t), less its value at t = 1)."""
    c = _dist_rgba(colour, "ramp_glow")
    r = _dist_int(radius, 1, DIST_MAX_RADIUS, "ramp_glow: radius must be 1..%d" % DIST_MAX_RADIUS)
    t = np.arange(256, dtype=np.float64) / 255.0
    if falloff == "linear":
        a = 1.0 - t
    elif falloff == "smooth":
        a = (1.0 - t) ** 2
    elif falloff == "exp":
        a = (np.exp(-4.0 * t) - np.exp(-4.0)) / (1.0 - np.exp(-4.0))
    else:
        raise ValueError("ramp_glow: falloff must be \"linear\", \"smooth\" or \"exp\"")
    table = np.empty((256, 4), np.uint8)
    table[:, :3] = c[:3]
    table[:, 3] = np.clip(np.floor(c[3] * a + 0.5), 0, 255).astype(np.uint8)
    table[-1, 3] = 0
    return table, -(-255 * 256 // r)   # (the last entry is reached at the radius: ceil(255 * 256 / radius))


def ramp_stroke(colour, width):
    """(table, step) for a stroke of `colour` (r, g, b[, a]) `width` pixels (1..254) wide around the seeds: one entry a
    pixel (step 256), the colour's alpha up to the width, 0 from one pixel further on, interpolated between."""
    c = _dist_rgba(colour, "ramp_stroke")
    w = _dist_int(width, 1, DIST_MAX_RADIUS - 1, "ramp_stroke: width must be 1..%d" % (DIST_MAX_RADIUS - 1))
    table = np.empty((w + 2, 4), np.uint8)
    table[:] = c
    table[-1, 3] = 0
    return table, 256


def ramp_rings(colour, spacing, width):
    """(table, step) for contour rings of `colour` (r, g, b[, a]) around the seeds under repeat=True: a ring `width`
    pixels wide every `spacing` pixels (1 <= width < spacing <= 1023), the first on the seeds' border.  One entry a pixel
    (step 256); the last entry repeats the first, so that the wrap is seamless."""
    c = _dist_rgba(colour, "ramp_rings")
    sp = _dist_int(spacing, 2, RAMP_MAX_N - 1, "ramp_rings: spacing must be 2..%d" % (RAMP_MAX_N - 1))
    w = _dist_int(width, 1, sp - 1, "ramp_rings: width must be 1..spacing - 1")
    table = np.empty((sp + 1, 4), np.uint8)
    table[:] = c
    table[w:sp, 3] = 0
    return table, 256


def _dist_field(field, r, who):
    f = np.asarray(field)
    if f.dtype != np.uint16:
        raise ValueError("%s: field must be a uint16 array (Scene.get_distance, distance_host)" % who)
    return f, _dist_int(r, 0, DIST_MAX_RADIUS, "%s: r must be 0..%d" % (who, DIST_MAX_RADIUS))


def mask_dilate(field, r):
    """The seeds of a field dilated by a disc of radius r, as a bool array: field <= r * r.  r must not exceed the radius
    the field was computed with."""
    f, r = _dist_field(field, r, "mask_dilate")
    return f <= r * r


def mask_erode(field, r):
    """The shape eroded by a disc of radius r, as a bool array, from a field computed with invert=True (its seeds are the
    shape's complement, so it holds each pixel's distance to the nearest pixel outside the shape): field > r * r.  r must
    not exceed the radius the field was computed with."""
    f, r = _dist_field(field, r, "mask_erode")
    return f > r * r


WARP_CELL, WARP_BORDER, WARP_CLAMP, WARP_PER_CHANNEL, WARP_MAX_SIDE, WARP_NODE_MAX = 16, 0, 1, 1, 8192, 1 << 22   # (TR_WARP_*)
WARP_EDGES = {"border": WARP_BORDER, "clamp": WARP_CLAMP}


class WarpParams(C.Structure):
    """tr_warp_params"""
    _fields_ = [("edge", C.c_uint32), ("border", C.c_uint8 * 3), ("pad", C.c_uint8), ("flags", C.c_uint32)]


def warp_params(edge="border", border=(0, 0, 0), per_channel=False, who="warp"):
    """tr_warp_params: the edge mode, "border" (a texel outside the image is `border`, r g b) or "clamp" (texel indices
    are clamped to the image), and whether the scene's grid is three grids, one a channel.  ValueError, in the library's
    words, for what it would refuse."""
    if edge in WARP_EDGES:
        e = WARP_EDGES[edge]
    elif not isinstance(edge, (bool, str)) and edge in WARP_EDGES.values():
        e = int(edge)
    else:
        raise ValueError("%s: edge must be TR_WARP_BORDER or TR_WARP_CLAMP" % who)
    b = [int(v) for v in border]
    if len(b) != 3 or any(not 0 <= v <= 255 for v in b):
        raise ValueError("%s: border is three values 0..255" % who)
    return WarpParams(e, (C.c_uint8 * 3)(*b), 0, WARP_PER_CHANNEL if per_channel else 0)


def warp_grid_shape(width, height):
    """(gh, gw): the nodes of a grid for an output of width x height -- one every 16 pixels and one behind the last cell."""
    return (int(height) + WARP_CELL - 1) // WARP_CELL + 1, (int(width) + WARP_CELL - 1) // WARP_CELL + 1


def _warp_grid(grid, width, height, who):
    """`grid` as the library takes it: int32 [n, gh, gw, 2] with n = 1 or 3 ([gh, gw, 2] is one grid), its size and every
    node checked in the library's words."""
    for v in (width, height):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 1 <= v <= WARP_MAX_SIDE:
            raise ValueError("%s: width and height must be 1..8192" % who)
    if grid is None:
        raise ValueError("%s: null grid" % who)
    g = np.asarray(grid)
    if g.dtype.kind not in "iu":
        raise ValueError("%s: the grid is an integer array (units of 1/256 source pixel)" % who)
    if g.ndim == 3:
        g = g[None]
    gh, gw = warp_grid_shape(width, height)
    if g.ndim != 4 or g.shape[0] not in (1, 3):
        raise ValueError("%s: n_grids must be 1 or 3 (TR_WARP_PER_CHANNEL)" % who)
    if g.shape[1:] != (gh, gw, 2):
        raise ValueError("%s: a grid for %d x %d is [%d, %d, 2] (gh, gw, (sx, sy))" % (who, width, height, gh, gw))
    if g.size and (int(g.min()) < -WARP_NODE_MAX or int(g.max()) > WARP_NODE_MAX):
        raise ValueError("%s: a node value outside [-2^22, 2^22]" % who)
    return np.ascontiguousarray(g, np.int32)


def warp_host(rgb, grid, width, height, params):
    """tr_warp_host: the rule of Scene.warp on the host (no GPU needed).  rgb [H, W, 3] uint8 with row 0 = top
    (get_frame_buffer), grid as for Scene.set_warp for an output of width x height, params from warp_params.  Returns the
    [height, width, 3] frame and leaves its arguments alone."""
    src = np.ascontiguousarray(rgb, np.uint8)
    if src.ndim != 3 or src.shape[2] != 3:
        raise ValueError("tr_warp_host: rgb [H, W, 3]")
    _check_params(params, WarpParams, "tr_warp_host", "warp_params")
    g = _warp_grid(grid, width, height, "tr_warp_host")
    out = np.empty((int(height), int(width), 3), np.uint8)
    check(load_library().tr_warp_host(src.shape[1], src.shape[0], src.ctypes.data, int(width), int(height), g.shape[0], g.ctypes.data,
                                      C.addressof(params), out.ctypes.data))
    return out


def warp_grid_from_function(f, width, height):
    """A grid for an output of width x height from f(X, Y) -> (sx, sy): X and Y are float64 arrays [gh, gw] of the nodes'
    OUTPUT pixel indices (0, 16, 32, ... -- the last column and row may lie outside the output), sx and sy the SOURCE
    sample each should show, in pixels (sample indices: 0 is the first sample's centre).  Evaluated in floating point;
    a node is floor(256 v + 0.5), clipped to [-2^22, 2^22].  int32 [gh, gw, 2].  Between the nodes the device
    interpolates linearly: a grid follows a smooth function to within its curvature over 16 pixels."""
    gh, gw = warp_grid_shape(width, height)
    Y, X = np.meshgrid(np.arange(gh, dtype=np.float64) * WARP_CELL, np.arange(gw, dtype=np.float64) * WARP_CELL, indexing="ij")
    sx, sy = f(X, Y)
    g = np.stack([np.broadcast_to(np.asarray(sx, np.float64), X.shape), np.broadcast_to(np.asarray(sy, np.float64), X.shape)], axis=-1)
    g = np.nan_to_num(np.floor(256.0 * g + 0.5), nan=0.0, posinf=float(WARP_NODE_MAX), neginf=-float(WARP_NODE_MAX))
    return np.clip(g, -WARP_NODE_MAX, WARP_NODE_MAX).astype(np.int32)


def warp_grid_identity(width, height):
    """The grid that shows every source sample where it is: at the frame's own size Scene.warp is then a copy."""
    return warp_grid_from_function(lambda X, Y: (X, Y), width, height)


def warp_grid_rotate(deg, width, height, src_width=None, src_height=None, zoom=1.0):
    """The picture turned counter-clockwise by `deg` degrees (and magnified by `zoom`) about its centre: the centre of
    the width x height output shows the centre of the src_width x src_height source (default: the same size).
    Multiples of 90 degrees take exact sines, so a quarter turn with the sides exchanged is np.rot90 in every byte."""
    sw = width if src_width is None else src_width
    sh = height if src_height is None else src_height
    q = float(deg) / 90.0
    if q == int(q):
        c, s = ((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0))[int(q) % 4]
    else:
        c, s = float(np.cos(np.radians(deg))), float(np.sin(np.radians(deg)))
    c, s = c / zoom, s / zoom
    cxo, cyo, cxs, cys = (width - 1) / 2.0, (height - 1) / 2.0, (sw - 1) / 2.0, (sh - 1) / 2.0
    return warp_grid_from_function(lambda X, Y: (cxs + c * (X - cxo) - s * (Y - cyo), cys + s * (X - cxo) + c * (Y - cyo)), width, height)


def warp_grid_lens(k1, k2=0.0, width=None, height=None, scale=1.0):
    """A Brown-Conrady radial lens: the output pixel at distance r from the centre (r = 1 at the corner) shows the source
    at distance r (1 + k1 r^2 + k2 r^4) * scale along the same ray.  k1 < 0 gives a barrel, k1 > 0 a pincushion; apply
    the model's own coefficients to distort a rendered frame like the lens, their inverse fit to undistort one."""
    cx, cy = (width - 1) / 2.0, (height - 1) / 2.0
    R2 = max(cx * cx + cy * cy, 1.0)

    def f(X, Y):
        dx, dy = X - cx, Y - cy
        r2 = (dx * dx + dy * dy) / R2
        m = (1.0 + k1 * r2 + k2 * r2 * r2) * scale
        return cx + dx * m, cy + dy * m
    return warp_grid_from_function(f, width, height)


def warp_grid_homography(M, width, height):
    """A projective map (keystone, perspective correction): M, 3 x 3, takes an output pixel (X, Y, 1) to the source's
    homogeneous (x, y, w); the node is (x / w, y / w).  A node whose w is not positive is thrown far outside."""
    M = np.asarray(M, np.float64).reshape(3, 3)

    def f(X, Y):
        x, y, w = (M[i, 0] * X + M[i, 1] * Y + M[i, 2] for i in range(3))
        ok = w > 1e-12
        w = np.where(ok, w, 1.0)
        far = float(WARP_NODE_MAX)
        return np.where(ok, x / w, -far), np.where(ok, y / w, -far)
    return warp_grid_from_function(f, width, height)


def warp_grid_chromatic(px, width, height):
    """Three grids [3, gh, gw, 2] for TR_WARP_PER_CHANNEL: red is scaled up and blue down about the centre so that at the
    corner they lie `px` source pixels to either side of green, which stays (lateral chromatic aberration)."""
    cx, cy = (width - 1) / 2.0, (height - 1) / 2.0
    e = float(px) / max(float(np.hypot(cx, cy)), 1.0)
    return np.stack([warp_grid_from_function(lambda X, Y, m=m: (cx + (X - cx) * m, cy + (Y - cy) * m), width, height)
                     for m in (1.0 - e, 1.0, 1.0 + e)])


CONVOLVE_SEPARABLE, CONVOLVE_ABS, CONVOLVE_UNSHARP, CONVOLVE_BORDER, CONVOLVE_CLAMP = 1, 2, 4, 0, 1   # (TR_CONVOLVE_*)
CONVOLVE_EDGES = {"border": CONVOLVE_BORDER, "clamp": CONVOLVE_CLAMP}
CONVOLVE_AXIS_SHIFT = 11   # the builders' normalised rows sum to 2^11: a row and a column make A = 2^22, the largest allowed


class ConvolveParams(C.Structure):
    """tr_convolve_params"""
    _fields_ = [("struct_size", C.c_uint32), ("kw", C.c_uint32), ("kh", C.c_uint32), ("flags", C.c_uint32), ("shift", C.c_uint32),
                ("bias", C.c_int32), ("amount", C.c_uint32), ("edge", C.c_uint32), ("border", C.c_uint8 * 3), ("pad", C.c_uint8),
                ("weights", C.c_int16 * 82)]


def convolve_params(kernel, shift=0, bias=0, edge="border", border=(0, 0, 0), absolute=False, unsharp=None):
    """tr_convolve_params for Scene.convolve / Scene.get_convolved / convolve_host.  kernel: an integer array [kh, kw]
    (the general form, kw and kh odd and 1..9; kernel[j][i] is the weight of row j from the top, column i from the left)
    or a pair (row, col) of 1-D integer arrays (the separable form, 1..31 taps each, w(i, j) = row[i] * col[j]).  The sum
    of the weighted neighbours is shifted right by `shift` (0..22, rounded), made absolute with absolute=True, and `bias`
    (-255..255) is added; unsharp=AMOUNT (0..1024 in 1/256) sharpens instead: F + AMOUNT / 256 * (F - filtered).  edge:
    "border" (a tap outside the image is `border`, r g b) or "clamp".  ValueError, in the library's words, for what it
    would refuse (include/tiny_renderer.h)."""
    if edge in CONVOLVE_EDGES:
        e = CONVOLVE_EDGES[edge]
    elif not isinstance(edge, (bool, str)) and edge in CONVOLVE_EDGES.values():
        e = int(edge)
    else:
        raise ValueError("convolve: edge must be TR_CONVOLVE_BORDER or TR_CONVOLVE_CLAMP")
    b = [int(v) for v in border]
    if len(b) != 3 or any(not 0 <= v <= 255 for v in b):
        raise ValueError("convolve: border is three values 0..255")
    for name, v in (("shift", shift), ("bias", bias)) + ((("unsharp", unsharp),) if unsharp is not None else ()):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError("convolve: %s must be an integer" % name)
    if not 0 <= shift <= 22:
        raise ValueError("convolve: shift must be 0..22")
    if not -255 <= bias <= 255:
        raise ValueError("convolve: bias must be -255..255")
    if unsharp is not None and not 0 <= unsharp <= 1024:
        raise ValueError("convolve: amount must be 0..1024")
    flags = (CONVOLVE_ABS if absolute else 0) | (CONVOLVE_UNSHARP if unsharp is not None else 0)
    if isinstance(kernel, tuple) and len(kernel) == 2:
        flags |= CONVOLVE_SEPARABLE
        parts = [np.asarray(v) for v in kernel]
        if any(v.ndim != 1 or v.dtype.kind not in "iu" for v in parts):
            raise ValueError("convolve: (row, col) are two 1-D integer arrays")
        kw, kh = parts[0].size, parts[1].size
        if kw % 2 == 0 or kh % 2 == 0 or kw > 31 or kh > 31:
            raise ValueError("convolve: kw and kh must be odd and 1..31 (TR_CONVOLVE_SEPARABLE)")
        taps = np.concatenate(parts)
    else:
        k = np.asarray(kernel)
        if k.ndim != 2 or k.dtype.kind not in "iu":
            raise ValueError("convolve: the kernel is a 2-D integer array [kh, kw], or a pair (row, col)")
        kh, kw = k.shape
        if kw % 2 == 0 or kh % 2 == 0 or kw > 9 or kh > 9:
            raise ValueError("convolve: kw and kh must be odd and 1..9 (1..31 with TR_CONVOLVE_SEPARABLE)")
        taps = k.reshape(-1)
    if taps.size and (int(taps.min()) < -32768 or int(taps.max()) > 32767):
        raise ValueError("convolve: a weight does not fit an int16")
    p = ConvolveParams(C.sizeof(ConvolveParams), kw, kh, flags, int(shift), int(bias), int(unsharp or 0), e, (C.c_uint8 * 3)(*b), 0)
    for i, v in enumerate(taps):
        p.weights[i] = int(v)
    L = load_library()
    if L.tr_convolve_host(0, 0, None, None, C.addressof(p)) != 0:   # (an empty image: the parameter checks alone)
        raise ValueError(L.tr_last_error().decode().replace("tr_convolve_host", "convolve", 1))
    return p


def convolve_host(rgb, params):
    """tr_convolve_host: the rule of Scene.convolve on the host (no GPU needed), by the inline functions k_convolve calls.
    rgb [H, W, 3] uint8 with row 0 = top (get_frame_buffer), params from convolve_params.  Returns the filtered frame and
    leaves its arguments alone."""
    _check_params(params, ConvolveParams, "convolve_host", "convolve_params")
    src = np.ascontiguousarray(rgb, np.uint8)
    if src.ndim != 3 or src.shape[2] != 3:
        raise ValueError("convolve_host: rgb [H, W, 3]")
    out = np.empty_like(src)
    check(load_library().tr_convolve_host(src.shape[1], src.shape[0], src.ctypes.data, out.ctypes.data, C.addressof(params)))
    return out


def _convolve_normalise(w, shift=CONVOLVE_AXIS_SHIFT):
    """The symmetric positive taps `w` (odd length) as integers that sum to exactly 2^shift and stay symmetric: the left
    half by cumulative rounding (each tap is the difference of two rounded running sums), mirrored, the centre takes the
    rest -- the way the resize tables reach 4096."""
    w = np.asarray(w, np.float64)
    r = w.size // 2
    run = np.floor(np.cumsum(w[:r]) / w.sum() * (1 << shift) + 0.5).astype(np.int64)
    left = np.diff(np.concatenate([[0], run]))
    return np.concatenate([left, [(1 << shift) - 2 * int(left.sum())], left[::-1]]).astype(np.int32)


def kernel_gaussian(sigma, radius=None):
    """((row, col), shift): a separable Gaussian of standard deviation `sigma` pixels, cut at `radius` (default
    ceil(3 sigma), at most 15).  Each axis sums to 2^11, shift is 22: a flat colour stays."""
    r = int(min(15, max(1, np.ceil(3.0 * float(sigma))))) if radius is None else int(radius)
    if not 0 <= r <= 15 or not float(sigma) > 0.0:
        raise ValueError("kernel_gaussian: sigma above 0, radius 0..15")
    d = np.arange(-r, r + 1, dtype=np.float64)
    g = _convolve_normalise(np.exp(-0.5 * (d / float(sigma)) ** 2))
    return (g, g.copy()), 2 * CONVOLVE_AXIS_SHIFT


def kernel_box(rx, ry):
    """((row, col), shift): the mean over (2 rx + 1) x (2 ry + 1) pixels, rx and ry 0..15; each axis sums to 2^11."""
    if not (0 <= int(rx) <= 15 and 0 <= int(ry) <= 15):
        raise ValueError("kernel_box: rx and ry 0..15")
    return (_convolve_normalise(np.ones(2 * int(rx) + 1)), _convolve_normalise(np.ones(2 * int(ry) + 1))), 2 * CONVOLVE_AXIS_SHIFT


def kernel_tent(R):
    """((row, col), shift): the tent of radius R (0..15) on both axes.  Where R + 1 is a power of two the taps are the
    plain [1 .. R + 1 .. 1] and shift = 4 log2(R + 1) -- under a border of 0 tr_scene_bloom's glow at threshold 0;
    otherwise each axis is normalised to 2^11."""
    R = int(R)
    if not 0 <= R <= 15:
        raise ValueError("kernel_tent: R 0..15")
    t = (R + 1 - np.abs(np.arange(-R, R + 1))).astype(np.int32)
    if (R + 1) & R == 0:
        return (t, t.copy()), 4 * int(R + 1).bit_length() - 4
    t = _convolve_normalise(t)
    return (t, t.copy()), 2 * CONVOLVE_AXIS_SHIFT


def kernel_sobel(axis):
    """(kernel, 0): the 3 x 3 Sobel derivative along "x" (left to right) or "y" (top to bottom); use absolute=True or a
    bias of 128 to see both signs."""
    if axis not in ("x", "y"):
        raise ValueError('kernel_sobel: axis "x" or "y"')
    k = np.array([[-1, 0, 1], [-2, 0, 2], [-1, 0, 1]], np.int32)
    return (k if axis == "x" else np.ascontiguousarray(k.T)), 0


def kernel_laplacian():
    """(kernel, 0): the 3 x 3 four-neighbour Laplacian; with absolute=True an edge detector."""
    return np.array([[0, 1, 0], [1, -4, 1], [0, 1, 0]], np.int32), 0


def kernel_emboss():
    """(kernel, 0): a 3 x 3 emboss lit from the top left; its weights sum to 0, so use a bias of 128."""
    return np.array([[-1, -1, 0], [-1, 0, 1], [0, 1, 1]], np.int32), 0


def kernel_motion(length, horizontal=True):
    """((row, col), shift): a directional blur over `length` pixels (odd, 1..31) along x or along y; sums to 2^11."""
    n = int(length)
    if n % 2 == 0 or not 1 <= n <= 31:
        raise ValueError("kernel_motion: length odd and 1..31")
    line, one = _convolve_normalise(np.ones(n)), np.array([1], np.int32)
    return ((line, one) if horizontal else (one, line)), CONVOLVE_AXIS_SHIFT


RANK_VALUE, RANK_RANGE, RANK_MID, RANK_CLAMP_CENTRE, RANK_BORDER, RANK_CLAMP = 0, 1, 2, 3, 0, 1   # (TR_RANK_*)
RANK_OPS = {"value": RANK_VALUE, "range": RANK_RANGE, "mid": RANK_MID, "clamp_centre": RANK_CLAMP_CENTRE}
RANK_EDGES = {"border": RANK_BORDER, "clamp": RANK_CLAMP}


class RankParams(C.Structure):
    """tr_rank_params"""
    _fields_ = [("struct_size", C.c_uint32), ("kw", C.c_uint32), ("kh", C.c_uint32), ("op", C.c_uint32), ("rank", C.c_uint32),
                ("rank2", C.c_uint32), ("edge", C.c_uint32), ("border", C.c_uint8 * 3), ("pad", C.c_uint8), ("rows", C.c_uint16 * 15),
                ("pad2", C.c_uint16)]


def rank_params(footprint, rank="median", rank2=None, op="value", edge="border", border=(0, 0, 0)):
    """tr_rank_params for Scene.rank / Scene.get_ranked / rank_host.  footprint: a 2-D array [kh, kw] (both odd, 1..15)
    whose non-zero entries are the taps, footprint[j][i] being row j from the top, column i from the left
    (footprint_rect, footprint_disc, footprint_cross and footprint_line build the usual ones).  rank: "median"
    ((n - 1) // 2 of the n taps), "min" (0), "max" (n - 1) or an integer; rank2 likewise, for the ops of two ranks.  op:
    "value" (v(rank)), "range" (v(rank2) - v(rank)), "mid" ((v(rank) + v(rank2) + 1) >> 1) or "clamp_centre" (the pixel
    clamped to [v(rank), v(rank2)]).  edge: "border" (a tap outside the image is `border`, r g b) or "clamp".
    ValueError, in the library's words, for what it would refuse (include/tiny_renderer.h)."""
    if edge in RANK_EDGES:
        e = RANK_EDGES[edge]
    elif not isinstance(edge, (bool, str)) and edge in RANK_EDGES.values():
        e = int(edge)
    else:
        raise ValueError("rank: edge must be TR_RANK_BORDER or TR_RANK_CLAMP")
    if op in RANK_OPS:
        o = RANK_OPS[op]
    elif not isinstance(op, (bool, str)) and op in RANK_OPS.values():
        o = int(op)
    else:
        raise ValueError("rank: op must be TR_RANK_VALUE, TR_RANK_RANGE, TR_RANK_MID or TR_RANK_CLAMP_CENTRE")
    b = [int(v) for v in border]
    if len(b) != 3 or any(not 0 <= v <= 255 for v in b):
        raise ValueError("rank: border is three values 0..255")
    f = np.asarray(footprint)
    if f.ndim != 2 or f.dtype.kind not in "biu":
        raise ValueError("rank: the footprint is a 2-D boolean or integer array [kh, kw]")
    kh, kw = f.shape
    if kw % 2 == 0 or kh % 2 == 0 or kw > 15 or kh > 15:
        raise ValueError("rank: kw and kh must be odd and 1..15")
    taps = f != 0
    n = int(taps.sum())

    def which(r, name):
        if isinstance(r, str):
            if r not in ("median", "min", "max"):
                raise ValueError('rank: %s is "median", "min", "max" or an integer' % name)
            return {"median": max(n - 1, 0) // 2, "min": 0, "max": max(n - 1, 0)}[r]
        if isinstance(r, bool) or not isinstance(r, (int, np.integer)) or r < 0 or r > 0xFFFFFFFF:
            raise ValueError('rank: %s is "median", "min", "max" or an integer' % name)
        return int(r)

    p = RankParams(C.sizeof(RankParams), kw, kh, o, which(rank, "rank"), 0 if rank2 is None else which(rank2, "rank2"), e, (C.c_uint8 * 3)(*b), 0)
    for j in range(kh):
        p.rows[j] = sum(1 << i for i in range(kw) if taps[j, i])
    L = load_library()
    if L.tr_rank_host(0, 0, None, None, C.addressof(p)) != 0:   # (an empty image: the parameter checks alone)
        raise ValueError(L.tr_last_error().decode().replace("tr_rank_host", "rank", 1))
    return p


def rank_host(rgb, params):
    """tr_rank_host: the rule of Scene.rank on the host (no GPU needed), by the inline functions k_rank shares.  rgb
    [H, W, 3] uint8 with row 0 = top (get_frame_buffer), params from rank_params.  Returns the filtered frame and leaves
    its arguments alone."""
    _check_params(params, RankParams, "rank_host", "rank_params")
    src = np.ascontiguousarray(rgb, np.uint8)
    if src.ndim != 3 or src.shape[2] != 3:
        raise ValueError("rank_host: rgb [H, W, 3]")
    out = np.empty_like(src)
    check(load_library().tr_rank_host(src.shape[1], src.shape[0], src.ctypes.data, out.ctypes.data, C.addressof(params)))
    return out


def footprint_rect(kw, kh):
    """[kh, kw] of True: every pixel of the box (kw and kh odd, 1..15)."""
    kw, kh = int(kw), int(kh)
    if kw % 2 == 0 or kh % 2 == 0 or not 1 <= kw <= 15 or not 1 <= kh <= 15:
        raise ValueError("footprint_rect: kw and kh odd and 1..15")
    return np.ones((kh, kw), bool)


def footprint_disc(r):
    """[2 r + 1, 2 r + 1]: the taps with dx^2 + dy^2 <= r^2 + r (r 0..7): 9 taps at r = 1, 21 at 2, 37 at 3."""
    r = int(r)
    if not 0 <= r <= 7:
        raise ValueError("footprint_disc: r 0..7")
    d = np.arange(-r, r + 1)
    return np.add.outer(d * d, d * d) <= r * r + r


def footprint_cross(r):
    """[2 r + 1, 2 r + 1]: the centre row and the centre column (r 0..7), 4 r + 1 taps."""
    r = int(r)
    if not 0 <= r <= 7:
        raise ValueError("footprint_cross: r 0..7")
    f = np.zeros((2 * r + 1, 2 * r + 1), bool)
    f[r, :] = f[:, r] = True
    return f


def footprint_line(length, degrees):
    """A line of `length` pixels (odd, 1..15) through the centre at `degrees` counter-clockwise from the x axis as the
    picture is seen: step t = -(length - 1) / 2 .. (length - 1) / 2 is the tap at dx = round(t cos), dy = -round(t sin)
    (halves away from zero), in the smallest box that holds them."""
    n = int(length)
    if n % 2 == 0 or not 1 <= n <= 15:
        raise ValueError("footprint_line: length odd and 1..15")
    t = np.arange(-(n // 2), n // 2 + 1, dtype=np.float64)
    a = np.deg2rad(float(degrees))
    away = lambda v: (np.sign(v) * np.floor(np.abs(v) + 0.5)).astype(np.int64)
    dx, dy = away(t * np.cos(a)), -away(t * np.sin(a))
    rx, ry = int(np.abs(dx).max()), int(np.abs(dy).max())
    f = np.zeros((2 * ry + 1, 2 * rx + 1), bool)
    f[dy + ry, dx + rx] = True
    return f


BILATERAL_GUIDE_COLOUR, BILATERAL_GUIDE_DEPTH, BILATERAL_BORDER, BILATERAL_CLAMP = 0, 1, 0, 1   # (TR_BILATERAL_*)
BILATERAL_GUIDES = {"colour": BILATERAL_GUIDE_COLOUR, "depth": BILATERAL_GUIDE_DEPTH}
BILATERAL_EDGES = {"border": BILATERAL_BORDER, "clamp": BILATERAL_CLAMP}


class BilateralParams(C.Structure):
    """tr_bilateral_params"""
    _fields_ = [("struct_size", C.c_uint32), ("kw", C.c_uint32), ("kh", C.c_uint32), ("guide", C.c_uint32), ("edge", C.c_uint32),
                ("depth_scale", C.c_float), ("border", C.c_uint8 * 3), ("pad", C.c_uint8), ("spatial", C.c_uint8 * 225),
                ("pad2", C.c_uint8 * 3), ("range", C.c_uint8 * 256)]


def bilateral_params(spatial, range_table, guide="colour", depth_scale=0.0, edge="clamp", border=(0, 0, 0)):
    """tr_bilateral_params for Scene.bilateral / Scene.get_bilateral / bilateral_host.  spatial: a 2-D integer array
    [kh, kw] (both odd, 1..15) of weights 0..255, spatial[j][i] being row j from the top, column i from the left; a weight
    of 0 is no tap (spatial_box and spatial_gaussian build the usual ones).  range_table: 256 weights 0..255, entry d for a
    tap at distance d from the centre (range_gaussian, range_step).  guide: "colour" (d = the largest channel difference)
    or "depth" (d = |zT - zC| * depth_scale, cut at 255).  edge: "clamp" or "border" (a tap outside the image is
    `border`, r g b, and not drawn).  ValueError, in the library's words, for what it would refuse
    (include/tiny_renderer.h)."""
    if guide in BILATERAL_GUIDES:
        g = BILATERAL_GUIDES[guide]
    elif not isinstance(guide, (bool, str)) and guide in BILATERAL_GUIDES.values():
        g = int(guide)
    else:
        raise ValueError("bilateral: guide must be TR_BILATERAL_GUIDE_COLOUR or TR_BILATERAL_GUIDE_DEPTH")
    if edge in BILATERAL_EDGES:
        e = BILATERAL_EDGES[edge]
    elif not isinstance(edge, (bool, str)) and edge in BILATERAL_EDGES.values():
        e = int(edge)
    else:
        raise ValueError("bilateral: edge must be TR_BILATERAL_BORDER or TR_BILATERAL_CLAMP")
    b = [int(v) for v in border]
    if len(b) != 3 or any(not 0 <= v <= 255 for v in b):
        raise ValueError("bilateral: border is three values 0..255")
    w = np.asarray(spatial)
    if w.ndim != 2 or w.dtype.kind not in "biu" or (w.size and (int(w.min()) < 0 or int(w.max()) > 255)):
        raise ValueError("bilateral: spatial is a 2-D integer array [kh, kw] of weights 0..255")
    kh, kw = w.shape
    if kw % 2 == 0 or kh % 2 == 0 or kw > 15 or kh > 15:
        raise ValueError("bilateral: kw and kh must be odd and 1..15")
    r = np.asarray(range_table)
    if r.shape != (256,) or r.dtype.kind not in "biu" or int(r.min()) < 0 or int(r.max()) > 255:
        raise ValueError("bilateral: range_table is 256 integer weights 0..255")
    p = BilateralParams(C.sizeof(BilateralParams), kw, kh, g, e, float(depth_scale), (C.c_uint8 * 3)(*b), 0)
    C.memmove(p.spatial, np.ascontiguousarray(w, np.uint8).ctypes.data, kw * kh)
    C.memmove(p.range, np.ascontiguousarray(r, np.uint8).ctypes.data, 256)
    L = load_library()
    if L.tr_bilateral_host(0, 0, None, None, None, C.addressof(p)) != 0:   # (an empty image: the parameter checks alone)
        raise ValueError(L.tr_last_error().decode().replace("tr_bilateral_host", "bilateral", 1))
    return p


def bilateral_host(rgb, params, z=None):
    """tr_bilateral_host: the rule of Scene.bilateral on the host (no GPU needed), by the inline functions k_bilateral
    shares.  rgb [H, W, 3] uint8 with row 0 = top (get_frame_buffer), params from bilateral_params, z [H, W] float32 with
    row 0 = bottom (read_z_f32) -- needed under the depth guide only.  Returns the filtered frame and leaves its arguments
    alone."""
    _check_params(params, BilateralParams, "bilateral_host", "bilateral_params")
    src = np.ascontiguousarray(rgb, np.uint8)
    if src.ndim != 3 or src.shape[2] != 3:
        raise ValueError("bilateral_host: rgb [H, W, 3]")
    zz = None
    if z is not None:
        zz = np.ascontiguousarray(z, np.float32)
        if zz.shape != src.shape[:2]:
            raise ValueError("bilateral_host: z [H, W] beside rgb [H, W, 3]")
    elif params.guide == BILATERAL_GUIDE_DEPTH:
        raise ValueError("bilateral_host: the depth guide needs z")
    out = np.empty_like(src)
    check(load_library().tr_bilateral_host(src.shape[1], src.shape[0], src.ctypes.data, None if zz is None else zz.ctypes.data, out.ctypes.data,
                                           C.addressof(params)))
    return out


def spatial_box(kw, kh):
    """[kh, kw] uint8 of 255: every pixel of the window at the same weight (kw and kh odd, 1..15)."""
    kw, kh = int(kw), int(kh)
    if kw % 2 == 0 or kh % 2 == 0 or not 1 <= kw <= 15 or not 1 <= kh <= 15:
        raise ValueError("spatial_box: kw and kh odd and 1..15")
    return np.full((kh, kw), 255, np.uint8)


def spatial_gaussian(radius, sigma):
    """[2 r + 1, 2 r + 1] uint8: round(255 exp(-(dx^2 + dy^2) / (2 sigma^2))), radius 0..7, sigma above 0; the centre is
    255, and a weight that rounds to 0 is no tap."""
    r = int(radius)
    if not 0 <= r <= 7 or not float(sigma) > 0.0:
        raise ValueError("spatial_gaussian: sigma above 0, radius 0..7")
    d = np.arange(-r, r + 1, dtype=np.float64)
    return np.floor(255.0 * np.exp(-0.5 * np.add.outer(d * d, d * d) / float(sigma) ** 2) + 0.5).astype(np.uint8)


def range_gaussian(sigma):
    """[256] uint8: round(255 exp(-d^2 / (2 sigma^2))) for the distances d = 0..255, sigma above 0."""
    if not float(sigma) > 0.0:
        raise ValueError("range_gaussian: sigma above 0")
    d = np.arange(256, dtype=np.float64)
    return np.floor(255.0 * np.exp(-0.5 * (d / float(sigma)) ** 2) + 0.5).astype(np.uint8)


def range_step(cutoff):
    """[256] uint8: 255 for the distances d <= cutoff (0..255) and 0 beyond -- only taps within the cutoff count, all alike."""
    c = int(cutoff)
    if not 0 <= c <= 255:
        raise ValueError("range_step: cutoff 0..255")
    return np.where(np.arange(256) <= c, 255, 0).astype(np.uint8)


BLOOM_MAX_RADIUS, BLOOM_GLOW_ONLY, BLOOM_MAX_STRENGTH = 15, 1, 1024   # (TR_BLOOM_MAX_RADIUS, TR_BLOOM_GLOW_ONLY)


class BloomParams(C.Structure):
    """tr_bloom_params"""
    _fields_ = [("struct_size", C.c_uint32), ("radius", C.c_uint32), ("threshold", C.c_uint32), ("strength", C.c_uint32),
                ("flags", C.c_uint32)]


def bloom_params(radius, threshold=200, strength=256, flags=0):
    """tr_bloom_params for Scene.bloom / Scene.get_bloom / bloom_host: pixels whose largest channel exceeds threshold
    (0..255) are blurred by a tent of `radius` pixels (1..15) and added back scaled by strength / 256 (0..1024); flags:
    BLOOM_GLOW_ONLY (the blurred highlights alone) or 0.  ValueError for what the library would refuse
    (include/tiny_renderer.h)."""
    for name, v in (("radius", radius), ("threshold", threshold), ("strength", strength), ("flags", flags)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError("bloom: %s must be an integer" % name)
    if not 1 <= radius <= BLOOM_MAX_RADIUS:
        raise ValueError("bloom: radius must be 1..%d pixels" % BLOOM_MAX_RADIUS)
    if not 0 <= threshold <= 255:
        raise ValueError("bloom: threshold must be 0..255")
    if not 0 <= strength <= BLOOM_MAX_STRENGTH:
        raise ValueError("bloom: strength must be 0..%d" % BLOOM_MAX_STRENGTH)
    if flags & ~BLOOM_GLOW_ONLY:
        raise ValueError("bloom: unknown flags")
    return BloomParams(C.sizeof(BloomParams), int(radius), int(threshold), int(strength), int(flags))


def bloom_host(rgb, params):
    """tr_bloom_host: the rule of Scene.bloom on the host (no GPU needed), by the inline functions k_bloom calls.  rgb
    [H, W, 3] uint8 with row 0 = top (get_frame_buffer), params from bloom_params.  Returns the bloomed frame and leaves
    its arguments alone."""
    _check_params(params, BloomParams, "bloom_host", "bloom_params")
    src = np.ascontiguousarray(rgb, np.uint8)
    if src.ndim != 3 or src.shape[2] != 3:
        raise ValueError("bloom_host: rgb [H, W, 3]")
    out = np.empty_like(src)
    check(load_library().tr_bloom_host(src.shape[1], src.shape[0], src.ctypes.data, out.ctypes.data, C.addressof(params)))
    return out


GRADE_MAX_N = 33   # (TR_GRADE_MAX_N)


def _lut_array(lut, who):
    """A colour lookup table as the library takes it: contiguous uint8 [n, n, n, 3] indexed [b][g][r], n = 2..33."""
    if not isinstance(lut, np.ndarray) or lut.dtype != np.uint8:
        raise ValueError("%s: the table must be a uint8 array [n, n, n, 3]" % who)
    if lut.ndim != 4 or lut.shape[3] != 3 or not (lut.shape[0] == lut.shape[1] == lut.shape[2]):
        raise ValueError("%s: the table must have the shape [n, n, n, 3] (indexed [b][g][r])" % who)
    if not 2 <= lut.shape[0] <= GRADE_MAX_N:
        raise ValueError("%s: the table's edge n must be 2..%d" % (who, GRADE_MAX_N))
    return np.ascontiguousarray(lut)


def grade_host(rgb, lut):
    """tr_grade_host: the rule of Scene.grade on the host (no GPU needed), by the inline functions k_grade calls.  rgb
    uint8 [..., 3] in any pixel order, lut uint8 [n, n, n, 3] indexed [b][g][r].  Returns the graded pixels and leaves its
    arguments alone."""
    table = _lut_array(lut, "grade_host")
    if not isinstance(rgb, np.ndarray) or rgb.dtype != np.uint8 or rgb.ndim < 1 or rgb.shape[-1] != 3:
        raise ValueError("grade_host: rgb must be a uint8 array [..., 3]")
    src = np.ascontiguousarray(rgb)
    out = np.empty_like(src)
    check(load_library().tr_grade_host(src.size // 3, src.ctypes.data, out.ctypes.data, table.shape[0], table.ctypes.data))
    return out


def lut_from_function(n, f):
    """The table [n, n, n, 3] (indexed [b][g][r]) of a colour function: f takes a float array [..., 3] of rgb in [0, 1] at
    the table's grid points i / (n - 1) and returns one of the same shape in [0, 1] (clipped), rounded half up to u8."""
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not 2 <= n <= GRADE_MAX_N:
        raise ValueError("lut_from_function: n must be an integer 2..%d" % GRADE_MAX_N)
    axis = np.arange(n, dtype=np.float64) / (n - 1)
    b, g, r = np.meshgrid(axis, axis, axis, indexing="ij")
    out = np.asarray(f(np.stack([r, g, b], -1)), np.float64)
    if out.shape != (n, n, n, 3):
        raise ValueError("lut_from_function: f must return an array of its argument's shape")
    return np.floor(np.clip(out, 0.0, 1.0) * 255.0 + 0.5).astype(np.uint8)


def lut_identity(n):
    """The identity table: E(i) = round(255 i / (n - 1)) in each channel (exact where n - 1 divides 255, else within 1)."""
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not 2 <= n <= GRADE_MAX_N:
        raise ValueError("lut_identity: n must be an integer 2..%d" % GRADE_MAX_N)
    e = ((2 * 255 * np.arange(n, dtype=np.int64) + (n - 1)) // (2 * (n - 1))).astype(np.uint8)
    out = np.empty((n, n, n, 3), np.uint8)
    out[..., 0], out[..., 1], out[..., 2] = e[None, None, :], e[None, :, None], e[:, None, None]
    return out


def load_cube(path):
    """A 3-D table from a .cube text file: LUT_3D_SIZE n, an optional TITLE, DOMAIN_MIN 0 0 0 / DOMAIN_MAX 1 1 1 (the unit
    domain, also the default), then n^3 lines of three floats, red fastest.  Returns uint8 [n, n, n, 3] indexed
    [b][g][r], values clipped to [0, 1] and rounded half up.  ValueError for a 1-D table (LUT_1D_SIZE), another domain,
    n outside 2..33 and a wrong number of entries."""
    n, rows = None, []
    with open(path) as fh:
        for line in fh:
            line = line.split("#", 1)[0].strip()
            if not line:
                continue
            word = line.split()
            key = word[0].upper()
            if key == "TITLE":
                continue
            if key == "LUT_1D_SIZE" or key == "LUT_1D_INPUT_RANGE":
                raise ValueError("load_cube: %s holds a 1-D table; a 3-D table expresses it" % path)
            if key == "LUT_3D_SIZE":
                n = int(word[1])
                if not 2 <= n <= GRADE_MAX_N:
                    raise ValueError("load_cube: LUT_3D_SIZE must be 2..%d, not %d" % (GRADE_MAX_N, n))
                continue
            if key in ("DOMAIN_MIN", "DOMAIN_MAX", "LUT_3D_INPUT_RANGE"):
                want = {"DOMAIN_MIN": [0.0] * 3, "DOMAIN_MAX": [1.0] * 3, "LUT_3D_INPUT_RANGE": [0.0, 1.0]}[key]
                if [float(v) for v in word[1:]] != want:
                    raise ValueError("load_cube: only the unit domain is supported (%s)" % line)
                continue
            if key[0].isalpha():
                raise ValueError("load_cube: unknown keyword %s" % word[0])
            if len(word) != 3:
                raise ValueError("load_cube: an entry is three numbers (%s)" % line)
            rows.append([float(v) for v in word])
    if n is None:
        raise ValueError("load_cube: no LUT_3D_SIZE in %s" % path)
    if len(rows) != n ** 3:
        raise ValueError("load_cube: %d entries for LUT_3D_SIZE %d" % (len(rows), n))
    vals = np.asarray(rows, np.float64).reshape(n, n, n, 3)
    return np.floor(np.clip(vals, 0.0, 1.0) * 255.0 + 0.5).astype(np.uint8)


STATS_DEPTH = 1   # (TR_STATS_DEPTH)


class StatsParams(C.Structure):
    """tr_stats_params"""
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("x0", C.c_uint32), ("y0", C.c_uint32), ("w", C.c_uint32),
                ("h", C.c_uint32), ("z_lo", C.c_float), ("z_scale", C.c_float)]


class FrameStatsRecord(C.Structure):
    """tr_frame_stats"""
    _fields_ = [("hist", (C.c_uint32 * 256) * 5), ("zhist", C.c_uint32 * 256), ("n_pixels", C.c_uint32), ("n_drawn", C.c_uint32),
                ("n_nan", C.c_uint32), ("z_min", C.c_float), ("z_max", C.c_float), ("box_x0", C.c_uint32), ("box_y0", C.c_uint32),
                ("box_x1", C.c_uint32), ("box_y1", C.c_uint32), ("reserved", C.c_uint32 * 3)]


FRAME_STATS_BYTES = C.sizeof(FrameStatsRecord)   # 6192


def stats_params(window=None, depth=False, z_lo=0.0, z_scale=1.0):
    """tr_stats_params for Scene.frame_stats / Scene.get_frame_stats / frame_stats_host.  window: None (the whole frame) or
    (x0, y0, w, h) in output-image coordinates with w, h >= 1; depth: also coverage, the depth range, the box of drawn
    pixels and a depth histogram whose bin is min(255, ((z - z_lo) * z_scale) as u32).  ValueError for what the library
    would refuse (include/tiny_renderer.h) as far as it can be told without the frame's size."""
    x0 = y0 = w = h = 0
    if window is not None:
        try:
            x0, y0, w, h = window
        except (TypeError, ValueError):
            raise ValueError("frame statistics: window must be None or (x0, y0, w, h)")
        for v in (x0, y0, w, h):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= v <= 0xFFFFFFFF:
                raise ValueError("frame statistics: window must hold four integers 0..2^32 - 1")
        if w < 1 or h < 1:
            raise ValueError("frame statistics: a window has w and h >= 1 (None: the whole frame)")
    z_lo, z_scale = float(z_lo), float(z_scale)
    if depth:
        with np.errstate(over="ignore"):   # (as f32: what the library gets)
            l32, s32 = np.float32(z_lo), np.float32(z_scale)
        if not np.isfinite(l32):
            raise ValueError("frame statistics: z_lo must be finite")
        if not np.isfinite(s32) or not s32 > 0.0:
            raise ValueError("frame statistics: z_scale must be finite and > 0")
    return StatsParams(C.sizeof(StatsParams), STATS_DEPTH if depth else 0, int(x0), int(y0), int(w), int(h), z_lo, z_scale)


class FrameStats:
    """A tr_frame_stats record as numpy arrays and scalars: hist uint32 [5, 256] (r, g, b, luma, max channel), zhist uint32
    [256], n_pixels, n_drawn, n_nan (int), z_min, z_max (np.float32), box = (x0, y0, x1, y1) in output-image coordinates,
    x1 and y1 exclusive.  `raw` is the record's 6192 bytes as a uint8 array; two records are equal when those are."""

    def __init__(self, raw):
        raw = np.array(np.asarray(raw).reshape(-1).view(np.uint8), copy=True)
        if raw.nbytes != FRAME_STATS_BYTES:
            raise ValueError("a tr_frame_stats record has %d bytes, not %d" % (FRAME_STATS_BYTES, raw.nbytes))
        self.raw = raw
        w = raw.view(np.uint32)
        self.hist = w[:1280].reshape(5, 256)
        self.zhist = w[1280:1536]
        self.n_pixels, self.n_drawn, self.n_nan = int(w[1536]), int(w[1537]), int(w[1538])
        self.z_min, self.z_max = w[1539:1541].view(np.float32)
        self.box = tuple(int(v) for v in w[1541:1545])
        self.reserved = w[1545:1548]

    luma = property(lambda self: self.hist[3])
    max_channel = property(lambda self: self.hist[4])

    def __eq__(self, other):
        return isinstance(other, FrameStats) and np.array_equal(self.raw, other.raw)

    def __ne__(self, other):
        return not self == other

    __hash__ = None

    def __repr__(self):
        return "FrameStats(n_pixels=%d, n_drawn=%d, n_nan=%d, z_min=%r, z_max=%r, box=%r)" % (
            self.n_pixels, self.n_drawn, self.n_nan, float(self.z_min), float(self.z_max), self.box)


def frame_stats_host(rgb, z=None, window=None, depth=None, z_lo=0.0, z_scale=1.0):
    """tr_frame_stats_host: the rule of Scene.frame_stats on the host (no GPU needed), by the inline functions k_stats calls.
    rgb [H, W, 3] uint8 with row 0 = top (get_frame_buffer); z None or [H, W] float32 with row 0 = bottom (read_z_f32);
    depth: None means "when z is given".  Returns a FrameStats and leaves its arguments alone."""
    src = np.ascontiguousarray(rgb, np.uint8)
    if src.ndim != 3 or src.shape[2] != 3:
        raise ValueError("frame_stats_host: rgb [H, W, 3]")
    if depth is None:
        depth = z is not None
    zz = None
    if depth:
        if z is None:
            raise ValueError("frame_stats_host: depth statistics need z")
        zz = np.ascontiguousarray(z, np.float32)
        if zz.shape != src.shape[:2]:
            raise ValueError("frame_stats_host: z [H, W] beside rgb [H, W, 3]")
    p = stats_params(window, depth, z_lo, z_scale)
    out = np.zeros(FRAME_STATS_BYTES, np.uint8)
    check(load_library().tr_frame_stats_host(src.shape[1], src.shape[0], src.ctypes.data, zz.ctypes.data if zz is not None else None,
                                             C.addressof(p), out.ctypes.data))
    return FrameStats(out)


def frame_stats_merge(a, b):
    """tr_frame_stats_merge: the record (a new FrameStats) of the union of the two disjoint pixel sets whose records are a
    and b -- two bands of a frame, two windows that do not overlap."""
    if not isinstance(a, FrameStats) or not isinstance(b, FrameStats):
        raise ValueError("frame_stats_merge: two FrameStats records")
    dst, src = a.raw.copy(), np.ascontiguousarray(b.raw)
    check(load_library().tr_frame_stats_merge(dst.ctypes.data, src.ctypes.data))
    return FrameStats(dst)


def hist_percentile(hist, q):
    """The smallest bin whose cumulative count reaches q (0..1) of the histogram's total -- at least one count, so q = 0 gives
    the lowest occupied bin and q = 1 the highest.  An empty histogram gives 0."""
    h = np.asarray(hist)
    if h.ndim != 1 or h.dtype.kind not in "iu" or h.size == 0:
        raise ValueError("hist_percentile: a 1-D array of counts")
    q = float(q)
    if not 0.0 <= q <= 1.0:
        raise ValueError("hist_percentile: q must be 0..1")
    cum = np.cumsum(h.astype(np.uint64))
    total = int(cum[-1])
    if total == 0:
        return 0
    need = max(1, int(np.ceil(q * total)))
    return int(np.searchsorted(cum, need, side="left"))


def lut_auto_levels(stats, low=0.01, high=0.99, n=17):
    """A table [n, n, n, 3] for Scene.set_lut that stretches the picture's tones: the luma bins at the `low` and `high`
    percentiles of `stats` (a FrameStats) go to 0 and 255, every channel by the same line, clipped (lut_from_function).  A
    picture whose two bins coincide gets the step at that bin."""
    if not isinstance(stats, FrameStats):
        raise ValueError("lut_auto_levels: stats must be a FrameStats")
    low, high = float(low), float(high)
    if not 0.0 <= low < high <= 1.0:
        raise ValueError("lut_auto_levels: 0 <= low < high <= 1")
    lo, hi = hist_percentile(stats.luma, low), hist_percentile(stats.luma, high)
    hi = max(hi, lo + 1)
    return lut_from_function(n, lambda v: (v * 255.0 - lo) / float(hi - lo))


def depth_median(scene, window=None):
    """The median depth of the drawn pixels of `scene`'s current frame inside `window` (None: the whole frame), by two
    get_frame_stats calls: the depth range first, then a depth histogram of 256 bins over exactly that range; returns the
    centre of the bin the median lies in (within (z_max - z_min) / 512 of it), z_min itself where all depths are equal, and
    None where no pixel with a number for a depth is drawn.  Infinite depths are left to the outermost bins."""
    first = scene.get_frame_stats(window=window, depth=True)
    if first.n_drawn - first.n_nan <= 0:
        return None
    lo, hi = np.float32(first.z_min), np.float32(first.z_max)
    if not np.isfinite(lo) or not np.isfinite(hi):
        fin = np.float32(np.finfo(np.float32).max)
        lo, hi = np.clip(lo, -fin, fin), np.clip(hi, -fin, fin)
    with np.errstate(over="ignore", divide="ignore"):
        scale = np.float32(256.0) / (hi - lo)
    if not hi > lo or not np.isfinite(scale) or not scale > 0.0:
        return float(lo)
    second = scene.get_frame_stats(window=window, depth=True, z_lo=float(lo), z_scale=float(scale))
    b = hist_percentile(second.zhist, 0.5)
    return float(lo) + (b + 0.5) / float(scale)


def texel_set_host(pipeline_name, textures):
    """tr_texel_set_host: (words uint32 [n], blocks_per_row) -- the texel set tr_scene_create builds for the pipeline from
    four uint8 [h, w, 3] images of one size (csrc/tr_texels.h), by the function the library itself calls, on the host (no
    GPU needed)."""
    if len(textures) != 4:
        raise ValueError("four textures are required (texture, normal_map, normal_map_tangent, specular_map)")
    keep = [np.ascontiguousarray(t, np.uint8) for t in textures]
    if any(t.ndim != 3 or t.shape[2] != 3 for t in keep):
        raise ValueError("texel_set_host: textures are uint8 [h, w, 3] arrays")
    imgs = (_lib.ImageRgb8 * 4)(*[_lib.ImageRgb8(t.ctypes.data_as(C.POINTER(C.c_uint8)), t.shape[1], t.shape[0]) for t in keep])
    h, w = keep[0].shape[:2]
    cap = ((w + 3) // 4) * ((h + 1) // 2) * 32 + ((w + 7) // 8) * ((h + 3) // 4) * 32   # (either block shape fits)
    words = np.zeros(cap, np.uint32)
    bpr = C.c_uint32()
    n = check(load_library().tr_texel_set_host(pipeline_name.encode(), imgs, words.ctypes.data, cap, C.byref(bpr)))
    return words[:n].copy(), int(bpr.value)


class Scene:
    """Scene::new(width, height, obj, texture, normal_map, normal_map_tangent, specular_map,
    shader_pipeline_name) -- scene.rs:47-56.

    mesh: dict of float32 pos[n,3], tex[n,3], nrm[n,3] and uint32 idx[n_tri,9]
          (p0,t0,n0,p1,t1,n1,p2,t2,n2 -- obj::raw::RawObj as the path reads it).
    textures: uint8 [h,w,3] arrays in Scene::new's order.
    Extra keyword options are the tr_options of include/tiny_renderer.h.
    instances: optional [n, 4] float32 instance table (set_instances) drawn from the first frame on.
    instance_transforms: optional [n, 24] float32 transform table (set_instance_transforms) instead; a scene has one
          table, so giving both is a ValueError.
    """

    def __init__(self, width, height, mesh, textures, shader_pipeline_name, *, device=-1,
                 winner_tap=False, tile_stamps=False, band_rows=None, stream=None, frame_buffer_device=None,
                 bin_capacity=0, tile_waves=0, tile_mode=0, frames_per_launch=0, auto_group=True,
                 trust_frame_buffers=False, max_frame_slots=0, store_depth=False, instances=None,
                 instance_transforms=None):
        if instances is not None and instance_transforms is not None:
            raise ValueError("a scene draws one table: instances= or instance_transforms=, not both")
        L = load_library()
        self.width, self.height = int(width), int(height)
        keep = []
        m = _mesh_struct(mesh, keep)
        imgs = (_lib.ImageRgb8 * 4)()
        if len(textures) != 4:
            raise ValueError("four textures are required (texture, normal_map, normal_map_tangent, specular_map)")
        for k, t in enumerate(textures):
            t = np.ascontiguousarray(t, np.uint8)
            keep.append(t)
            imgs[k] = _lib.ImageRgb8(t.ctypes.data_as(C.POINTER(C.c_uint8)), t.shape[1], t.shape[0])
        self._tex_shapes = [tuple(t.shape) for t in keep[-4:]]
        o = _lib.Options()
        o.struct_size = C.sizeof(_lib.Options)
        o.device = device
        o.flags = ((_lib.TR_OPT_WINNER_TAP if winner_tap else 0) | (_lib.TR_OPT_TILE_STAMPS if tile_stamps else 0)
                   | (0 if auto_group else _lib.TR_OPT_NO_AUTO_GROUP)
                   | (_lib.TR_OPT_TRUST_FRAME_BUFFERS if trust_frame_buffers else 0)
                   | (_lib.TR_OPT_STORE_DEPTH if store_depth else 0))
        if band_rows is not None:
            o.band_row0, o.band_row1 = int(band_rows[0]), int(band_rows[1])
        o.stream = stream
        o.frame_buffer_device = frame_buffer_device
        o.bin_capacity = int(bin_capacity)
        o.tile_waves = int(tile_waves)
        o.tile_mode = int(tile_mode)
        o.frames_per_launch = int(frames_per_launch)
        o.max_frame_slots = int(max_frame_slots)
        h = C.c_void_p()
        self._h = None
        self._pinned = []
        check(L.tr_scene_create(self.width, self.height, C.byref(m), imgs,
                                shader_pipeline_name.encode(), C.byref(o), C.byref(h)))
        self._h = h
        self.pipeline = shader_pipeline_name
        self._mesh_shape = {"pos": np.empty((m.n_pos, 3), np.float32), "nrm": np.empty((m.n_nrm, 3), np.float32)}
        self.n_morph_targets = 0
        self.n_bones = 0
        if instances is not None:
            self.set_instances(instances)
        if instance_transforms is not None:
            self.set_instance_transforms(instance_transforms)

    def close(self):
        if getattr(self, "_h", None):
            load_library().tr_scene_destroy(self._h)   # waits for queued work, pending read-backs included
            self._h = None
            for p in getattr(self, "_pinned", []):
                load_library().tr_host_free(p)
            self._pinned = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # --- the reference's methods -------------------------------------------------------------
    def clear(self):
        check(load_library().tr_scene_clear(self._h))

    def set_light_direction(self, light_direction):
        check(load_library().tr_scene_set_light_direction(self._h, _f3(light_direction)))
        self._light = tuple(float(v) for v in light_direction)

    def set_camera(self, look_from, look_at, up):
        check(load_library().tr_scene_set_camera(self._h, _f3(look_from), _f3(look_at), _f3(up)))
        self._camera = tuple(tuple(float(v) for v in a) for a in (look_from, look_at, up))   # (for project)

    def render(self):
        check(load_library().tr_scene_render(self._h))

    def set_auto_group(self, on):
        """Whether render() may hold cleared frames back to fuse them (default on; tr_scene_set_auto_group)."""
        check(load_library().tr_scene_set_auto_group(self._h, 1 if on else 0))

    def _dropped(self, fn, value, n_arrays=1):
        """The setters' opening: None or an empty `value` calls setter `fn` with a count of zero and null arrays; was it so?"""
        if value is None or len(value) == 0:
            check(getattr(load_library(), fn)(self._h, 0, *[None] * n_arrays))
            return True
        return False

    def set_instances(self, instances):
        """tr_scene_set_instances: draw the mesh once per row of the [n, 4] float32 table (offset x, y, z, scale),
        positions p * scale + offset, instance-major polygon order; None or an empty table: the mesh itself."""
        if self._dropped("tr_scene_set_instances", instances):
            return
        a = _instance_table(instances)
        check(load_library().tr_scene_set_instances(self._h, a.shape[0], a.ctypes.data))

    def set_instance_transforms(self, table):
        """tr_scene_set_instance_transforms: draw the mesh once per row of the [n, 24] float32 table (instance_transforms
        builds one: a 3 x 4 for positions, a 3 x 3 for vertex normals), replacing a table of either kind; None or an
        empty table: the mesh itself."""
        if self._dropped("tr_scene_set_instance_transforms", table):
            return
        a = _transform_table(table)
        check(load_library().tr_scene_set_instance_transforms(self._h, a.shape[0], a.ctypes.data))

    def set_morph_targets(self, dpos, dnrm=None):
        """tr_scene_set_morph_targets: T morph targets as deltas dpos [T, n_pos, 3] and dnrm [T, n_nrm, 3] float32
        (morph_deltas builds one from a second mesh); None or no targets: drops them.  Leaves the scene without a pose."""
        if self._dropped("tr_scene_set_morph_targets", dpos, 2):
            self.n_morph_targets = 0
            return
        if dnrm is None:
            raise ValueError("morph targets need dnrm beside dpos")
        dp, dn = _morph_deltas(self._mesh_shape, dpos, dnrm)
        check(load_library().tr_scene_set_morph_targets(self._h, dp.shape[0], dp.ctypes.data, dn.ctypes.data))
        self.n_morph_targets = dp.shape[0]

    def set_morph_weights(self, weights):
        """tr_scene_set_morph_weights: the pose drawn from now on, [T] float32; None or empty: the mesh itself."""
        if self._dropped("tr_scene_set_morph_weights", weights):
            return
        w = _morph_weights(weights, self.n_morph_targets)
        check(load_library().tr_scene_set_morph_weights(self._h, w.shape[0], w.ctypes.data))

    def set_skin(self, bones, weights=None, n_bones=None):
        """tr_scene_set_skin: four influences per position index -- bones [n_pos, 4] uint32, weights [n_pos, 4] float32;
        n_bones: the palette's size (default: the largest index + 1).  None: drops the skin.  Leaves the scene without a
        palette."""
        L = load_library()
        if bones is None:
            check(L.tr_scene_set_skin(self._h, 0, None, None))
            self.n_bones = 0
            return
        if weights is None:
            raise ValueError("a skin needs weights beside bones")
        b, w = _skin(self._mesh_shape, bones, weights)
        n = int(n_bones) if n_bones is not None else (int(b.max()) + 1 if b.size else 1)
        if n < 1 or n > _lib.TR_SKIN_MAX_BONES:
            raise ValueError("a skin has 1 .. %d bones" % _lib.TR_SKIN_MAX_BONES)
        if b.size and int(b.max()) >= n:
            raise ValueError("bone index %d beyond the skin's %d bones" % (int(b.max()), n))
        check(L.tr_scene_set_skin(self._h, n, b.ctypes.data, w.ctypes.data))
        self.n_bones = n

    def set_bone_palette(self, palette):
        """tr_scene_set_bone_palette: the palette drawn from now on, [n_bones, 24] float32 (instance_transforms builds
        one); None or empty: no palette -- the morph pose's rows or the mesh's own."""
        if self._dropped("tr_scene_set_bone_palette", palette):
            return
        a = _palette(palette, self.n_bones)
        check(load_library().tr_scene_set_bone_palette(self._h, a.shape[0], a.ctypes.data))

    def debug_morph_rows(self):
        """tr_scene_debug_morph_rows: sets of posed rows the scene has on the device now (held and free)."""
        return check(load_library().tr_scene_debug_morph_rows(self._h))

    def render_frames(self, frames, frame_buffers_device=None, instances=None, instance_transforms=None, morph_weights=None,
                      bone_palettes=None):
        """tr_scene_render_frames: `frames` is an [n, 12] float32 array (or a list of (light, look_from,
        look_at, up) tuples): per frame light direction, look_from, look_at, up.  Frame i is what
        clear(); set_light_direction; set_camera; render() produces; the frames of a group are rendered by
        one launch per kernel.  frame_buffers_device: optional list of n device pointers (colour targets).
        instances: optional [n, n_instances, 4] float32 -- frame i draws table instances[i] (what set_instances
        before its render would do; tr_scene_render_frames_instanced); None: the current table in every frame.
        instance_transforms: the same with transform tables, [n, n_instances, 24] float32
        (tr_scene_render_frames_transformed); at most one of the two.
        morph_weights: [n, T] float32 -- frame i draws the pose morph_weights[i] (what set_morph_weights before its
        render would do; tr_scene_render_frames_morphed) under the scene's current table; not together with a table per
        frame.
        bone_palettes: [n, n_bones, 24] float32 -- frame i draws the palette bone_palettes[i] (what set_bone_palette
        before its render would do; tr_scene_render_frames_skinned) under the scene's current morph pose and table; not
        together with morph_weights= or a table per frame."""
        if bone_palettes is not None and (morph_weights is not None or instances is not None or instance_transforms is not None):
            raise ValueError("bone_palettes= draws the scene's current pose and table: nothing else per frame beside it")
        if instances is not None and instance_transforms is not None:
            raise ValueError("one table per frame: instances= or instance_transforms=, not both")
        if morph_weights is not None and (instances is not None or instance_transforms is not None):
            raise ValueError("morph_weights= draws the scene's current table: no table per frame beside it")
        if not isinstance(frames, np.ndarray):
            frames = np.asarray([np.concatenate([np.asarray(v, np.float32).reshape(3) for v in f]) for f in frames],
                                np.float32)
        frames = np.ascontiguousarray(frames, np.float32).reshape(-1, 12)
        fbs = None
        if frame_buffers_device is not None:
            if len(frame_buffers_device) != len(frames):
                raise ValueError("one frame buffer per frame")
            fbs = (C.c_void_p * len(frames))(*[int(q) for q in frame_buffers_device])
        # The per-frame input, at most one (above): its converter and what that takes beside the array, the call, what the
        # ValueError for a wrong number of frames calls it, whether an array without elements still goes as a pointer
        kinds = ((bone_palettes, _palette, (self.n_bones,), "tr_scene_render_frames_skinned", "palette", True),
                 (morph_weights, _morph_weights, (self.n_morph_targets,), "tr_scene_render_frames_morphed", "pose", False),
                 (instance_transforms, _transform_table, (), "tr_scene_render_frames_transformed", "instance transform table", False),
                 (instances, _instance_table, (), "tr_scene_render_frames_instanced", "instance table", False))
        for value, convert, args, fn, what, always_pointer in kinds:
            if value is not None:
                a = convert(value, *args, per_frame=True)
                if a.shape[0] != len(frames):
                    raise ValueError("one %s per frame" % what)
                check(getattr(load_library(), fn)(self._h, len(frames), frames.ctypes.data, a.shape[1],
                                                  a.ctypes.data if a.size or always_pointer else None, fbs))
                return
        check(load_library().tr_scene_render_frames(self._h, len(frames), frames.ctypes.data, fbs))

    @property
    def frames_per_launch(self):
        return check(load_library().tr_scene_frames_per_launch(self._h))

    def interior_tiles(self):
        """Did the newest fused tile launches run the kernels compiled for frames made of whole tiles only?"""
        return bool(check(load_library().tr_scene_interior_tiles(self._h)))

    def frames_kept(self):
        return check(load_library().tr_scene_frames_kept(self._h))

    def select_frame(self, back):
        """Makes the frame `back` frames before the last one of the last render_frames call current."""
        check(load_library().tr_scene_select_frame(self._h, int(back)))

    def _image(self, fn, strict, *args, out=None):
        """What getter `fn`(scene, *args, rgb) delivers, in `out` (default: a new [H, W, 3] uint8 array); its status goes to
        last_status, and through check() when strict."""
        if out is None:
            out = np.empty((self.height, self.width, 3), np.uint8)
        code = getattr(load_library(), fn)(self._h, *args, out.ctypes.data)
        if strict:
            check(code)
        self.last_status = code
        return out

    def _pinned_array(self, shape):
        """A page-locked uint8 array of `shape` from tr_host_alloc (freed with the scene)."""
        n = int(np.prod(shape))
        p = load_library().tr_host_alloc(n)
        if not p:
            raise MemoryError("tr_host_alloc(%d)" % n)
        self._pinned.append(p)
        return np.ctypeslib.as_array((C.c_uint8 * n).from_address(p)).reshape(shape)

    def _out_pointer(self, out, name="out", shape="[H, W, 3]", source="pinned_frame", nbytes=None):
        """`out` of a stage as the library takes it: None stays None (in place), an array of `nbytes` (default: a frame's)
        contiguous bytes gives its address, any other array a ValueError in the caller's words; anything else is a device
        pointer (int)."""
        if out is None:
            return None
        if isinstance(out, np.ndarray):
            if out.nbytes != (self.width * self.height * 3 if nbytes is None else nbytes) or not out.flags["C_CONTIGUOUS"]:
                text = "%s must be a contiguous %s uint8 array (%s)" % (name, shape, source)
                raise ValueError(text)
            return out.ctypes.data
        return int(out)

    def _target_pointer(self, out, tensor_text, name="out", shape="[H, W, 3]", source="pinned_frame", nbytes=None):
        """_out_pointer of a stage that takes a torch tensor too: one of at least `nbytes` contiguous bytes gives its
        address, any other tensor a ValueError of tensor_text."""
        if hasattr(out, "data_ptr"):
            if out.numel() * out.element_size() < (self.width * self.height * 3 if nbytes is None else nbytes) or not out.is_contiguous():
                raise ValueError(tensor_text)
            return out.data_ptr()
        return self._out_pointer(out, name, shape, source, nbytes)

    def get_frame_buffer(self, strict=True):
        return self._image("tr_scene_get_frame_buffer", strict)

    def pinned_frame(self):
        """A page-locked [H, W, 3] uint8 array for get_frame_buffer_async (freed with the scene)."""
        return self._pinned_array((self.height, self.width, 3))

    def get_frame_buffer_async(self, out):
        """Enqueue the read-back of the frame into `out` (see pinned_frame); valid after sync()."""
        if out.nbytes != self.width * self.height * 3 or not out.flags["C_CONTIGUOUS"]:
            raise ValueError("out must be a contiguous [H, W, 3] uint8 array")
        check(load_library().tr_scene_get_frame_buffer_async(self._h, out.ctypes.data))
        return out

    # --- supersampled output (tr_scene_resolve / tr_scene_get_resolved) ------------------------
    def _resolved_shape(self, factor):
        """(H / f, W / f, 3) of the frame resolved by `factor`; ValueError for what the host alone can rule out."""
        f = int(factor)
        if f != factor or f not in (2, 4, 8):
            raise ValueError("resolve factor must be 2, 4 or 8, not %r" % (factor,))
        if self.width % f or self.height % f:
            raise ValueError("a %d x %d frame cannot be resolved by %d: width and height must be multiples of it"
                             % (self.width, self.height, f))
        return self.height // f, self.width // f, 3

    def resolve(self, factor, out=None, strict=True):
        """The current frame box-filtered by `factor` (2, 4 or 8) on the device: an [H / f, W / f, 3] uint8 array,
        out[Y, X, c] = (sum of the f x f block of get_frame_buffer() + f * f / 2) // (f * f).  Synchronizes."""
        shape = self._resolved_shape(factor)
        if out is None:
            out = np.empty(shape, np.uint8)
        elif out.dtype != np.uint8 or out.nbytes != shape[0] * shape[1] * 3 or not out.flags["C_CONTIGUOUS"]:
            raise ValueError("out must be a contiguous [H / f, W / f, 3] uint8 array")
        return self._image("tr_scene_get_resolved", strict, int(factor), out=out)

    def pinned_resolved(self, factor):
        """A page-locked [H / f, W / f, 3] uint8 array for resolve_into (freed with the scene)."""
        return self._pinned_array(self._resolved_shape(factor))

    def resolve_into(self, factor, target):
        """Enqueue the resolve of the current frame behind the renders issued so far (tr_scene_resolve); the result is
        there after sync().  `target`: a device pointer (int) to 3 * (W / f) * (H / f) bytes, or an array from
        pinned_resolved.  A band scene writes output rows [band_row0 / f, band_row1 / f) only."""
        shape = self._resolved_shape(factor)
        ptr = self._out_pointer(target, "target", "[H / f, W / f, 3]", "pinned_resolved", shape[0] * shape[1] * 3)
        check(load_library().tr_scene_resolve(self._h, int(factor), ptr))
        return target

    def composite(self, src, winner_base=0):
        """tr_scene_composite: merges the current frame of scene `src` into this scene's on the device -- src wins a
        pixel where it drew one and is strictly nearer (the reference's depth test; ties keep this scene's pixel), taking
        colour, z and, with winner taps, src's winner + winner_base.  Asynchronous; both scenes must have the same size
        and band, and be on one device.  store_depth=True on both scenes avoids the depth-only repeat of their passes."""
        if src is self:
            raise ValueError("composite: src is this scene")
        if not isinstance(src, Scene):
            raise ValueError("composite: src must be a Scene")
        if (src.width, src.height) != (self.width, self.height):
            raise ValueError("composite: src is %d x %d, this scene %d x %d" % (src.width, src.height, self.width, self.height))
        check(load_library().tr_scene_composite(self._h, src._h, int(winner_base) & 0xFFFFFFFF))

    # --- shared shadows (tr_scene_render_shadow_pass / _colour_pass, tr_scene_shadow_merge) ----------
    def _two_pass(self, who):
        if getattr(self, "pipeline", None) not in TWO_PASS_PIPELINES:
            raise ValueError("%s: pipeline %r has one pass (shadow and occlusion have two)" % (who, getattr(self, "pipeline", None)))

    def render_shadow_pass(self):
        """tr_scene_render_shadow_pass: the light-space depth pass of `shadow` / `occlusion` alone, into the current
        frame's shadow buffer; consumes a pending shadow clear, a pending clear of z and colour stays pending."""
        self._two_pass("render_shadow_pass")
        check(load_library().tr_scene_render_shadow_pass(self._h))

    def render_colour_pass(self):
        """tr_scene_render_colour_pass: the colour pass of `shadow` / `occlusion` alone, against the shadow buffer as it
        stands (the scene's own, or one merged with another scene's).  clear(); render_shadow_pass(); render_colour_pass()
        is render() after clear() in every byte."""
        self._two_pass("render_colour_pass")
        check(load_library().tr_scene_render_colour_pass(self._h))

    def shadow_merge(self, src):
        """tr_scene_shadow_merge: merges the shadow buffer of scene `src` into this scene's on the device, per pixel
        `if (zs >= zd) zd = zs` -- the buffer of the two meshes concatenated, when both shadow passes ran under one
        light and camera.  Asynchronous; both scenes on `shadow` or `occlusion`, of one size and on one device; bands
        need not match.  src is not written."""
        if src is self:
            raise ValueError("shadow_merge: src is this scene")
        if not isinstance(src, Scene):
            raise ValueError("shadow_merge: src must be a Scene")
        if (src.width, src.height) != (self.width, self.height):
            raise ValueError("shadow_merge: src is %d x %d, this scene %d x %d" % (src.width, src.height, self.width, self.height))
        self._two_pass("shadow_merge")
        src._two_pass("shadow_merge (src)")
        check(load_library().tr_scene_shadow_merge(self._h, src._h))

    def ambient_occlusion(self, radius=8, rings=1, threshold=1.0, falloff=20.0, grey=False):
        """tr_scene_ambient_occlusion: darkens the current frame in place on the device from its own z buffer -- `rings`
        rings of sixteen samples out to `radius` pixels, a sample occludes where it is nearer by more than `threshold`,
        by (zq - z0) / falloff, at most 1, a sixteenth (per ring) each; grey=True writes the occlusion alone (white to
        black).  Asynchronous; every later consumer sees the shaded frame, and calling it twice shades twice.  Band
        scenes are refused.  store_depth=True avoids the depth-only repeat of the frame's pass."""
        p = ao_params(radius, rings, threshold, falloff, grey)
        check(load_library().tr_scene_ambient_occlusion(self._h, C.addressof(p)))

    # --- frame accumulation (tr_scene_accumulate / tr_scene_get_accumulated) -----------------------
    def accumulate(self, n_frames, weights=None, strict=True):
        """The last `n_frames` frames of the last render_frames call -- frame k is what select_frame(k) makes current --
        averaged on the device under integer weights (0..255, None: all 1): an [H, W, 3] uint8 array,
        (sum of w_k * F_k + D // 2) // D on the stored bytes with D = sum of w_k.  Synchronizes; no frame is changed."""
        n, w = accumulate_weights(n_frames, weights)
        return self._image("tr_scene_get_accumulated", strict, n, w.ctypes.data if w is not None else None)

    def accumulate_into(self, n_frames, target, weights=None):
        """Enqueue the average behind the renders issued so far (tr_scene_accumulate); the result is there after sync().
        `target`: a device pointer (int) to 3 * W * H bytes that overlaps no frame buffer of the scene, or an array from
        pinned_frame.  A band scene writes its band's rows only."""
        n, w = accumulate_weights(n_frames, weights)
        if target is None:
            raise ValueError("accumulate_into: no target (accumulate_in_place averages into the current frame)")
        ptr = self._out_pointer(target, "target")
        check(load_library().tr_scene_accumulate(self._h, n, w.ctypes.data if w is not None else None, ptr))
        return target

    def accumulate_in_place(self, n_frames, weights=None):
        """tr_scene_accumulate with out = NULL: the average replaces the current frame, which must be one of the
        n_frames frames; every later consumer (the getters, resolve, the sparse read-back, composite) sees it, the other
        kept frames, z, winner words and the shadow buffer stay.  Asynchronous; calling it twice averages twice."""
        n, w = accumulate_weights(n_frames, weights)
        check(load_library().tr_scene_accumulate(self._h, n, w.ctypes.data if w is not None else None, None))

    # --- depth of field (tr_scene_depth_of_field / tr_scene_get_depth_of_field) ----------------------
    def depth_of_field(self, params, out=None):
        """tr_scene_depth_of_field: blurs the current frame by its own z buffer on the device (params from dof_params).
        out=None: in place -- every later consumer (the getters, resolve, the sparse read-back, composite) sees the
        blurred frame, z, winner words and the shadow buffer stay, calling it twice blurs twice.  Otherwise `out` is a
        device pointer (int) to 3 * W * H bytes that overlaps no frame buffer of the scene, or an array from
        pinned_frame, and the scene's frame stays as it is.  Asynchronous: the result is there after sync().  Band
        scenes are refused.  store_depth=True avoids the depth-only repeat of the frame's pass."""
        _check_params(params, DofParams, "depth_of_field", "dof_params")
        ptr = self._out_pointer(out)
        check(load_library().tr_scene_depth_of_field(self._h, C.addressof(params), ptr))
        return out

    def get_depth_of_field(self, params, strict=True):
        """tr_scene_get_depth_of_field: the current frame blurred on the device, as an [H, W, 3] uint8 array.
        Synchronizes; the scene's frame stays unblurred."""
        _check_params(params, DofParams, "get_depth_of_field", "dof_params")
        return self._image("tr_scene_get_depth_of_field", strict, C.addressof(params))

    # --- bloom (tr_scene_bloom / tr_scene_get_bloom) -------------------------------------------------
    def bloom(self, params, out=None):
        """tr_scene_bloom: keys the current frame's highlights, blurs them by a tent and adds them back on the device
        (params from bloom_params).  out=None: in place -- every later consumer (the getters, resolve, the sparse
        read-back, composite, set_texture_from_frame) sees the bloomed frame, z, winner words and the shadow buffer stay,
        calling it twice blooms twice.  Otherwise `out` is a device pointer (int) to 3 * W * H bytes that overlaps no frame
        buffer of the scene, or an array from pinned_frame, and the scene's frame stays as it is.  Asynchronous: the
        result is there after sync().  Band scenes are refused.  No depth is needed."""
        _check_params(params, BloomParams, "bloom", "bloom_params")
        ptr = self._out_pointer(out)
        check(load_library().tr_scene_bloom(self._h, C.addressof(params), ptr))
        return out

    def get_bloom(self, params, strict=True):
        """tr_scene_get_bloom: the current frame bloomed on the device, as an [H, W, 3] uint8 array.  Synchronizes; the
        scene's frame stays unbloomed."""
        _check_params(params, BloomParams, "get_bloom", "bloom_params")
        return self._image("tr_scene_get_bloom", strict, C.addressof(params))

    # --- colour grading (tr_scene_set_lut / tr_scene_grade / tr_scene_get_graded) ---------------------
    def set_lut(self, lut):
        """tr_scene_set_lut: the scene's colour lookup table, uint8 [n, n, n, 3] indexed [b][g][r], n = 2..33 (lut_identity,
        lut_from_function, load_cube); None drops it.  Waits for the scene's queued work."""
        if lut is None:
            check(load_library().tr_scene_set_lut(self._h, 0, None))
            return
        table = _lut_array(lut, "set_lut")
        check(load_library().tr_scene_set_lut(self._h, table.shape[0], table.ctypes.data))

    def grade(self, out=None):
        """tr_scene_grade: maps the current frame through the scene's table on the device.  out=None: in place -- every
        later consumer sees the graded frame, z, winner words and the shadow buffer stay, calling it twice grades twice.
        Otherwise `out` is a device pointer (int) to 3 * W * H bytes apart from every frame buffer of the scene, or an
        array from pinned_frame, and the scene's frame stays as it is.  Asynchronous: the result is there after sync().
        Band scenes write their band's rows only.  No depth is needed."""
        ptr = self._out_pointer(out)
        check(load_library().tr_scene_grade(self._h, ptr))
        return out

    def get_graded(self, strict=True):
        """tr_scene_get_graded: the current frame graded on the device, as an [H, W, 3] uint8 array.  Synchronizes; the
        scene's frame stays ungraded."""
        return self._image("tr_scene_get_graded", strict)

    def debug_grade_grid(self, cap=0):
        """tr_scene_debug_grade_grid: every later k_grade launch of the scene starts at most `cap` workgroups (0: no cap, the
        default), so that each walks more tiles; the result does not change.  Returns the number of workgroups of the
        scene's most recent k_grade launch, 0 if there has been none."""
        if isinstance(cap, bool) or not isinstance(cap, (int, np.integer)) or not 0 <= cap <= 0xFFFFFFFF:
            raise ValueError("debug_grade_grid: cap must be an integer 0..2^32 - 1")
        return check(load_library().tr_scene_debug_grade_grid(self._h, int(cap)))

    # --- outlines (tr_scene_outline / tr_scene_get_outlined) ------------------------------------------
    def outline(self, params, out=None):
        """tr_scene_outline: inks the current frame's silhouettes, depth steps and folds from its own z buffer on the
        device (params from outline_params).  out=None: in place, by the kernel itself -- every later consumer (the
        getters, resolve, the sparse read-back, composite) sees the outlined frame, z, winner words and the shadow buffer
        stay, calling it twice outlines twice.  Otherwise `out` is a device pointer (int) to 3 * W * H bytes apart from
        every frame buffer of the scene, or an array from pinned_frame, and the scene's frame stays as it is.
        Asynchronous: the result is there after sync().  Band scenes are refused.  store_depth=True avoids the
        depth-only repeat of the frame's pass."""
        _check_params(params, OutlineParams, "outline", "outline_params")
        ptr = self._out_pointer(out)
        check(load_library().tr_scene_outline(self._h, C.addressof(params), ptr))
        return out

    def get_outlined(self, params, strict=True):
        """tr_scene_get_outlined: the current frame outlined on the device, as an [H, W, 3] uint8 array.  Synchronizes;
        the scene's frame stays as it is."""
        _check_params(params, OutlineParams, "get_outlined", "outline_params")
        return self._image("tr_scene_get_outlined", strict, C.addressof(params))

    # --- edge anti-aliasing (tr_scene_antialias / tr_scene_get_antialiased) ---------------------------
    def antialias(self, params, out=None):
        """tr_scene_antialias: smooths the current frame's stair-steps on the device by a luma-driven edge filter (params
        from aa_params), at the frame's own size.  out=None: in place (through a scratch frame of the scene's) -- every
        later consumer sees the filtered frame, z, winner words and the shadow buffer stay, calling it twice filters
        twice.  Otherwise `out` is a device pointer (int) to 3 * W * H bytes apart from every frame buffer of the scene,
        or an array from pinned_frame, and the scene's frame stays as it is.  Asynchronous: the result is there after
        sync().  Band scenes are refused.  No depth is read."""
        _check_params(params, AaParams, "antialias", "aa_params")
        ptr = self._out_pointer(out)
        check(load_library().tr_scene_antialias(self._h, C.addressof(params), ptr))
        return out

    def get_antialiased(self, params, strict=True):
        """tr_scene_get_antialiased: the current frame filtered on the device, as an [H, W, 3] uint8 array.  Synchronizes;
        the scene's frame stays as it is."""
        _check_params(params, AaParams, "get_antialiased", "aa_params")
        return self._image("tr_scene_get_antialiased", strict, C.addressof(params))

    # --- resize (tr_scene_resize / tr_scene_get_resized) -----------------------------------------------
    def resize(self, width, height, filter="area", strict=True):
        """tr_scene_get_resized: the current frame scaled on the device to width x height (each 1..8192 and at least an
        eighth of the frame's) by the "area" or the "bilinear" filter: a [height, width, 3] uint8 array, equal to
        resize_host(get_frame_buffer(), width, height, filter) in every byte.  Synchronizes; the scene's frame stays."""
        p = resize_params(self.width, self.height, width, height, filter, "tr_scene_get_resized")
        return self._image("tr_scene_get_resized", strict, C.addressof(p), out=np.empty((p.height, p.width, 3), np.uint8))

    def pinned_resized(self, width, height):
        """A page-locked [height, width, 3] uint8 array for resize_into (freed with the scene)."""
        return self._pinned_array((int(height), int(width), 3))

    def resize_into(self, out, width, height, filter="area"):
        """tr_scene_resize: enqueue the resize of the current frame behind the renders issued so far; the result is there
        after sync().  `out`: a torch tensor on the scene's device or a device pointer (int) to 3 * width * height bytes,
        or an array from pinned_resized; every byte of it is written.  Band scenes are refused; there is no in-place
        form.  No depth is read."""
        p = resize_params(self.width, self.height, width, height, filter, "tr_scene_resize")
        if out is None:
            raise ValueError("tr_scene_resize: out == NULL (the output is no frame of the scene: there is no in-place form)")
        ptr = self._target_pointer(out, "out must be a contiguous tensor of at least 3 * width * height bytes", "out", "[height, width, 3]", "pinned_resized", p.width * p.height * 3)
        check(load_library().tr_scene_resize(self._h, C.addressof(p), ptr))
        return out

    # --- warp (tr_scene_set_warp / tr_scene_warp / tr_scene_get_warped) -------------------------------
    def set_warp(self, grid, width, height):
        """tr_scene_set_warp: the scene's grid of source coordinates for an output of width x height (each 1..8192): int32
        [gh, gw, 2], or [3, gh, gw, 2] for a grid a channel (warp_params(per_channel=True)), (gh, gw) = warp_grid_shape,
        nodes (sx, sy) in 1/256 source pixel (warp_grid_identity, warp_grid_from_function, warp_grid_rotate, warp_grid_lens,
        warp_grid_homography, warp_grid_chromatic).  Uploaded in stream order: work already issued keeps the old grid."""
        g = _warp_grid(grid, width, height, "tr_scene_set_warp")
        check(load_library().tr_scene_set_warp(self._h, int(width), int(height), g.shape[0], g.ctypes.data))
        self._warp_size = (int(width), int(height))

    def pinned_warped(self, width, height):
        """A page-locked [height, width, 3] uint8 array for warp (freed with the scene)."""
        return self._pinned_array((int(height), int(width), 3))

    def warp(self, params, out=None):
        """tr_scene_warp: resamples the current frame through the scene's grid on the device (params from warp_params).
        out=None: in place, allowed where the grid's size is the frame's -- every later consumer (the getters, resize,
        resolve, the sparse read-back) sees the warped frame, z and the shadow buffer stay.  Otherwise `out` is a torch
        tensor on the scene's device or a device pointer (int) to 3 * width * height bytes (the grid's size) apart from
        every frame buffer of the scene, or an array from pinned_warped; every byte of it is written and the scene's frame
        stays.  Asynchronous: the result is there after sync().  Band scenes are refused.  No depth is needed."""
        _check_params(params, WarpParams, "warp", "warp_params")
        w, h = getattr(self, "_warp_size", (self.width, self.height))
        ptr = self._target_pointer(out, "out must be a contiguous tensor of at least 3 * width * height bytes", "out", "[height, width, 3]", "pinned_warped", w * h * 3)
        check(load_library().tr_scene_warp(self._h, C.addressof(params), ptr))
        return out

    def get_warped(self, params, strict=True):
        """tr_scene_get_warped: the current frame warped on the device, as a [height, width, 3] uint8 array of the grid's
        size, equal to warp_host(get_frame_buffer(), grid, width, height, params) in every byte.  Synchronizes; the scene's
        frame stays."""
        _check_params(params, WarpParams, "get_warped", "warp_params")
        w, h = getattr(self, "_warp_size", (self.width, self.height))
        return self._image("tr_scene_get_warped", strict, C.addressof(params), out=np.empty((h, w, 3), np.uint8))

    # --- convolve (tr_scene_convolve / tr_scene_get_convolved) -----------------------------------------
    def convolve(self, params, out=None):
        """tr_scene_convolve: filters the current frame through a kernel of integer weights on the device (params from
        convolve_params; kernel_gaussian, kernel_box, kernel_tent, kernel_sobel, kernel_laplacian, kernel_emboss and
        kernel_motion build the usual ones).  out=None: in place -- every later consumer (the getters, resize, resolve,
        the sparse read-back) sees the filtered frame, z, winner words and the shadow buffer stay, calling it twice
        filters twice.  Otherwise `out` is a torch tensor on the scene's device or a device pointer (int) to 3 * W * H
        bytes that overlaps no frame buffer of the scene, or an array from pinned_frame, and the scene's frame stays as it
        is.  Asynchronous: the result is there after sync().  Band scenes are refused.  No depth is needed."""
        _check_params(params, ConvolveParams, "convolve", "convolve_params")
        ptr = self._target_pointer(out, "out must be a contiguous tensor of at least 3 * width * height bytes")
        check(load_library().tr_scene_convolve(self._h, C.addressof(params), ptr))
        return out

    def get_convolved(self, params, strict=True):
        """tr_scene_get_convolved: the current frame filtered on the device, as an [H, W, 3] uint8 array equal to
        convolve_host(get_frame_buffer(), params) in every byte.  Synchronizes; the scene's frame stays."""
        _check_params(params, ConvolveParams, "get_convolved", "convolve_params")
        return self._image("tr_scene_get_convolved", strict, C.addressof(params))

    # --- rank (tr_scene_rank / tr_scene_get_ranked) ----------------------------------------------------
    def rank(self, params, out=None):
        """tr_scene_rank: the current frame through an order-statistic filter on the device -- median, erode, dilate,
        morphological gradient, despeckle (params from rank_params; footprint_rect, footprint_disc, footprint_cross and
        footprint_line build the usual footprints).  out=None: in place -- every later consumer (the getters, resize,
        resolve, the sparse read-back) sees the filtered frame, z, winner words and the shadow buffer stay, calling it
        twice filters twice (open is erode then dilate).  Otherwise `out` is a torch tensor on the scene's device or a
        device pointer (int) to 3 * W * H bytes that overlaps no frame buffer of the scene, or an array from
        pinned_frame, and the scene's frame stays as it is.  Asynchronous: the result is there after sync().  Band scenes
        are refused.  No depth is needed."""
        _check_params(params, RankParams, "rank", "rank_params")
        ptr = self._target_pointer(out, "out must be a contiguous tensor of at least 3 * width * height bytes")
        check(load_library().tr_scene_rank(self._h, C.addressof(params), ptr))
        return out

    def get_ranked(self, params, strict=True):
        """tr_scene_get_ranked: the current frame filtered on the device, as an [H, W, 3] uint8 array equal to
        rank_host(get_frame_buffer(), params) in every byte.  Synchronizes; the scene's frame stays."""
        _check_params(params, RankParams, "get_ranked", "rank_params")
        return self._image("tr_scene_get_ranked", strict, C.addressof(params))

    # --- bilateral (tr_scene_bilateral / tr_scene_get_bilateral) ----------------------------------------
    def bilateral(self, params, out=None):
        """tr_scene_bilateral: the current frame through an edge-preserving weighted mean on the device, guided by colour
        or by the frame's own depth (params from bilateral_params; spatial_box, spatial_gaussian, range_gaussian and
        range_step build the usual tables).  out=None: in place -- every later consumer (the getters, resize, resolve, the
        sparse read-back) sees the filtered frame, z, winner words and the shadow buffer stay, calling it twice filters
        twice.  Otherwise `out` is a torch tensor on the scene's device or a device pointer (int) to 3 * W * H bytes that
        overlaps no frame buffer of the scene, or an array from pinned_frame, and the scene's frame stays as it is.
        Asynchronous: the result is there after sync().  Band scenes are refused.  The colour guide needs no depth; the
        depth guide makes a depth left on the chip real."""
        _check_params(params, BilateralParams, "bilateral", "bilateral_params")
        ptr = self._target_pointer(out, "out must be a contiguous tensor of at least 3 * width * height bytes")
        check(load_library().tr_scene_bilateral(self._h, C.addressof(params), ptr))
        return out

    def get_bilateral(self, params, strict=True):
        """tr_scene_get_bilateral: the current frame filtered on the device, as an [H, W, 3] uint8 array equal to
        bilateral_host(get_frame_buffer(), params, read_z_f32()) in every byte.  Synchronizes; the scene's frame stays."""
        _check_params(params, BilateralParams, "get_bilateral", "bilateral_params")
        return self._image("tr_scene_get_bilateral", strict, C.addressof(params))

    # --- YUV output (tr_scene_to_yuv / tr_scene_to_yuv_from / tr_scene_get_yuv) ------------------------
    def to_yuv(self, layout="i420", matrix="bt709", range="limited", strict=True):
        """tr_scene_get_yuv: the current frame as YCbCr planes, converted on the device: the tuple yuv_planes gives (NV12's
        second plane [ch, cw, 2]), equal to yuv_host(get_frame_buffer(), ...) in every byte.  Synchronizes."""
        p = yuv_params(layout, matrix, range, "tr_scene_get_yuv")
        flat = self._image("tr_scene_get_yuv", strict, C.addressof(p), out=np.empty(yuv_bytes(self.width, self.height, p.layout), np.uint8))
        return yuv_planes(flat, self.width, self.height, p.layout)

    def pinned_yuv(self, layout="i420", width=None, height=None):
        """A page-locked flat uint8 array of yuv_bytes bytes for to_yuv_into / to_yuv_from (freed with the scene); of the
        frame's size, or of width x height."""
        w, h = (self.width if width is None else width), (self.height if height is None else height)
        return self._pinned_array((yuv_bytes(w, h, layout),))

    def _yuv_target(self, target, nbytes, who):
        if target is None:
            raise ValueError("%s: out == NULL (there is no in-place form)" % who)
        text = "%s: target must be a contiguous tensor of at least yuv_bytes bytes" % who
        return self._target_pointer(target, text, "target", "flat yuv_bytes", "pinned_yuv", nbytes)

    def to_yuv_into(self, target, layout="i420", matrix="bt709", range="limited"):
        """tr_scene_to_yuv: enqueue the conversion of the current frame behind the renders issued so far; the planes are
        there after sync() (yuv_planes splits them).  `target`: a torch uint8 tensor on the scene's device, a device
        address (int, any alignment) of yuv_bytes bytes, or an array from pinned_yuv; every byte of it is written.  Band
        scenes are refused; there is no in-place form.  No depth is read."""
        p = yuv_params(layout, matrix, range, "tr_scene_to_yuv")
        ptr = self._yuv_target(target, yuv_bytes(self.width, self.height, p.layout), "tr_scene_to_yuv")
        check(load_library().tr_scene_to_yuv(self._h, C.addressof(p), ptr))
        return target

    def to_yuv_from(self, image, layout="i420", matrix="bt709", range="limited", target=None, width=None, height=None):
        """tr_scene_to_yuv_from: the planes of any tightly packed rgb8 image on the device -- what resize_into,
        resolve_into or warp wrote --, enqueued on the scene's stream behind everything issued so far.  `image`: a
        torch uint8 tensor [h, w, 3] on the scene's device, a page-locked [h, w, 3] array of the scene's, or a device
        address (int) with width and height.  `target` as for to_yuv_into, and the call is asynchronous; without one
        the call synchronizes and returns the tuple of planes."""
        p = yuv_params(layout, matrix, range, "tr_scene_to_yuv_from")
        if hasattr(image, "data_ptr") or isinstance(image, np.ndarray):
            shape = tuple(image.shape)
            contiguous = image.is_contiguous() if hasattr(image, "data_ptr") else image.flags["C_CONTIGUOUS"]
            if len(shape) != 3 or shape[2] != 3 or not contiguous or (image.element_size() if hasattr(image, "data_ptr") else image.itemsize) != 1:
                raise ValueError("tr_scene_to_yuv_from: image must be a contiguous [h, w, 3] uint8 tensor or page-locked array")
            h, w = shape[0], shape[1]
            src = image.data_ptr() if hasattr(image, "data_ptr") else image.ctypes.data
        else:
            w, h, src = width, height, int(image)
        w, h = _yuv_size(w, h, "tr_scene_to_yuv_from")
        nbytes = yuv_bytes(w, h, p.layout)
        own = target is None
        if own:
            cache = self.__dict__.setdefault("_yuv_blocks", {})
            target = cache.get(nbytes)
            if target is None:
                target = cache[nbytes] = self._pinned_array((nbytes,))
        ptr = self._yuv_target(target, nbytes, "tr_scene_to_yuv_from")
        check(load_library().tr_scene_to_yuv_from(self._h, src, w, h, C.addressof(p), ptr))
        if not own:
            return target
        self.sync()
        return yuv_planes(target.copy(), w, h, p.layout)

    # --- layers (tr_scene_layer / tr_scene_layer_from_scene / tr_scene_get_layered) ------------------
    def _layer_source(self, image, who, width, height, format, stride):
        """(address, format, width, height, stride, keep-alive) of `image`: a torch uint8 tensor [h, w, 3 | 4] on the scene's
        device or a page-locked array of the scene's (rows at any stride), or a device address (int) with width,
        height, format and stride."""
        if hasattr(image, "data_ptr") or isinstance(image, np.ndarray):
            fmt, w, h, st = _layer_array(image, who)
            return (image.data_ptr() if hasattr(image, "data_ptr") else image.ctypes.data), fmt, w, h, st
        if width is None or height is None:
            raise ValueError("%s: a device address needs width and height" % who)
        return int(image), format, width, height, stride

    def layer(self, image, x=0, y=0, mode="normal", opacity=256, where=None, key=None, out=None, width=None, height=None, format="rgb8", stride=0):
        """tr_scene_layer: blends a second image into the current frame on the device with its top-left pixel on frame
        pixel (x, y) (signed; row 0 = top; it may hang over any edge): a backdrop (where="undrawn"), a tint of the
        model (where="drawn"), a watermark or picture-in-picture, a vignette (mode="multiply"), a cross-fade (opacity).
        `image`: a torch uint8 tensor [h, w, 3] or [h, w, 4] on the scene's device -- a non-contiguous row stride is
        passed on as the stride --, a page-locked array of the scene's (pinned_layer), or a device address (int) with
        width, height, format and stride.  out=None: in place, by the kernel itself -- every later consumer sees the
        layered frame, z, winner words and the shadow buffer stay, calling it twice blends twice.  Otherwise `out` is a
        device pointer (int) to 3 * W * H bytes apart from every frame buffer of the scene, or an array from
        pinned_frame, and the scene's frame stays as it is.  Asynchronous: the result is there after sync() -- keep
        `image` alive until then.  Band scenes are refused.  Depth is read only with `where`.  layer_host is the rule."""
        src, fmt, w, h, st = self._layer_source(image, "tr_scene_layer", width, height, format, stride)
        p = layer_params(w, h, x, y, mode, fmt, opacity, where, key, st, "tr_scene_layer")
        check(load_library().tr_scene_layer(self._h, C.addressof(p), src, self._out_pointer(out)))
        return out

    def layer_from(self, other, x=0, y=0, mode="normal", opacity=256, where=None, key=None, out=None):
        """tr_scene_layer_from_scene: the same with the CURRENT frame of the scene `other` (any size) as the layer, read
        on the device behind its fast-clear flags; ordered behind other's renders issued so far.  other is only read."""
        if not isinstance(other, Scene):
            raise ValueError("tr_scene_layer_from_scene: other must be a Scene")
        p = layer_params(0, 0, x, y, mode, "rgb8", opacity, where, key, 0, "tr_scene_layer_from_scene")
        check(load_library().tr_scene_layer_from_scene(self._h, C.addressof(p), other._h, self._out_pointer(out)))
        return out

    def get_layered(self, image, x=0, y=0, mode="normal", opacity=256, where=None, key=None, strict=True, width=None, height=None,
                    format="rgb8", stride=0):
        """tr_scene_get_layered: the current frame with `image` blended in on the device (arguments as for layer), as an
        [H, W, 3] uint8 array.  Synchronizes; the scene's frame stays as it is."""
        src, fmt, w, h, st = self._layer_source(image, "tr_scene_get_layered", width, height, format, stride)
        p = layer_params(w, h, x, y, mode, fmt, opacity, where, key, st, "tr_scene_get_layered")
        return self._image("tr_scene_get_layered", strict, C.addressof(p), src)

    def pinned_layer(self, width, height, channels=3):
        """A page-locked [height, width, channels] uint8 array for layer / get_layered (freed with the scene)."""
        if channels not in (3, 4):
            raise ValueError("pinned_layer: channels must be 3 or 4")
        w, h = _layer_size(width, height, "pinned_layer")
        return self._pinned_array((h, w, channels))

    # --- depth ramp (tr_scene_set_ramp / tr_scene_ramp / tr_scene_get_ramped) -------------------------
    def set_ramp(self, table):
        """tr_scene_set_ramp: the scene's ramp table, uint8 [n, 4] of (r, g, b, a), n = 2..1024 (ramp_fog, ramp_grey,
        ramp_false_colour, ramp_contours, ramp_slice); None drops it.  Waits for the scene's queued work."""
        if table is None:
            check(load_library().tr_scene_set_ramp(self._h, 0, None))
            return
        tab = _ramp_table(table, "set_ramp")
        check(load_library().tr_scene_set_ramp(self._h, tab.shape[0], tab.ctypes.data))

    def ramp(self, z0, scale, mode="normal", opacity=256, undrawn=(0, 0, 0, 0), repeat=False, out=None, params=None):
        """tr_scene_ramp: blends the entry of the scene's ramp table that each pixel's own depth chooses into the current
        frame on the device (arguments: ramp_params, or params built by it with z0 and scale None).  out=None: in place,
        by the kernel itself -- every later consumer sees the ramped frame, z, winner words and the shadow buffer stay,
        calling it twice ramps twice.  Otherwise `out` is a device pointer (int) or tensor of 3 * W * H bytes apart from
        every frame buffer of the scene, or an array from pinned_frame, and the scene's frame stays as it is.
        Asynchronous: the result is there after sync().  Band scenes are refused.  store_depth=True avoids the depth-only
        repeat of the frame's pass.  ramp_host is the rule."""
        p = self._ramp_params("tr_scene_ramp", z0, scale, mode, opacity, undrawn, repeat, params)
        ptr = self._target_pointer(out, "out must be a contiguous tensor of at least 3 * width * height bytes")
        check(load_library().tr_scene_ramp(self._h, C.addressof(p), ptr))
        return out

    def get_ramped(self, z0, scale, mode="normal", opacity=256, undrawn=(0, 0, 0, 0), repeat=False, strict=True, params=None):
        """tr_scene_get_ramped: the current frame ramped on the device (arguments as for ramp), as an [H, W, 3] uint8
        array.  Synchronizes; the scene's frame stays as it is."""
        p = self._ramp_params("tr_scene_get_ramped", z0, scale, mode, opacity, undrawn, repeat, params)
        return self._image("tr_scene_get_ramped", strict, C.addressof(p))

    @staticmethod
    def _ramp_params(who, z0, scale, mode, opacity, undrawn, repeat, params):
        if params is None:
            return ramp_params(z0, scale, mode, opacity, undrawn, repeat, who)
        _check_params(params, RampParams, who, "ramp_params")
        return params

    def debug_ramp_grid(self, cap=0):
        """tr_scene_debug_ramp_grid: every later k_ramp launch of the scene starts at most `cap` workgroups (0: no cap, the
        default), so that each walks more tiles; the result does not change.  Returns the number of workgroups of the
        scene's most recent k_ramp launch, 0 if there has been none."""
        if isinstance(cap, bool) or not isinstance(cap, (int, np.integer)) or not 0 <= cap <= 0xFFFFFFFF:
            raise ValueError("debug_ramp_grid: cap must be an integer 0..2^32 - 1")
        return check(load_library().tr_scene_debug_ramp_grid(self._h, int(cap)))

    # --- lines (tr_scene_set_lines / tr_scene_lines / tr_scene_get_lined) -----------------------------
    def set_lines(self, lines):
        """tr_scene_set_lines: the scene's table of segments, a LINE_DTYPE array of up to 2^20 records in raster
        coordinates (lines_table, wireframe_lines); None or an empty table drops it.  Validates every segment and bins the
        table into the frame's tiles on the host; waits for the scene's queued work."""
        if lines is None or len(lines) == 0:
            check(load_library().tr_scene_set_lines(self._h, 0, None))
            return
        tab = _lines_table(lines, "set_lines")
        check(load_library().tr_scene_set_lines(self._h, tab.shape[0], tab.ctypes.data))

    def lines(self, width=1, opacity=256, depth_test=True, painter=False, depth_bias=0.0, out=None, params=None):
        """tr_scene_lines: draws the scene's table of segments into the current frame on the device, depth-tested against
        the frame's own z (arguments: lines_params, or params built by it).  out=None: in place, by the kernel itself --
        every later consumer sees the lines; z, winner words and the shadow buffer stay.  Otherwise `out` is a device
        pointer (int) or tensor of 3 * W * H bytes apart from every frame buffer of the scene, or an array from
        pinned_frame, and the scene's frame stays as it is.  Asynchronous: the result is there after sync().  Band scenes
        are refused.  lines_host is the rule."""
        p = self._lines_params("tr_scene_lines", width, opacity, depth_test, painter, depth_bias, params)
        ptr = self._target_pointer(out, "out must be a contiguous tensor of at least 3 * width * height bytes")
        check(load_library().tr_scene_lines(self._h, C.addressof(p), ptr))
        return out

    def get_lined(self, width=1, opacity=256, depth_test=True, painter=False, depth_bias=0.0, strict=True, params=None):
        """tr_scene_get_lined: the current frame with the lines drawn on the device (arguments as for lines), as an
        [H, W, 3] uint8 array.  Synchronizes; the scene's frame stays as it is."""
        p = self._lines_params("tr_scene_get_lined", width, opacity, depth_test, painter, depth_bias, params)
        return self._image("tr_scene_get_lined", strict, C.addressof(p))

    @staticmethod
    def _lines_params(who, width, opacity, depth_test, painter, depth_bias, params):
        if params is None:
            return lines_params(width, opacity, depth_test, painter, depth_bias, who)
        _check_params(params, LinesParams, who, "lines_params")
        return params

    def debug_line_bins(self):
        """tr_scene_debug_line_bins: (non-empty tiles, list entries) of the scene's table of lines."""
        nt, ne = C.c_uint32(), C.c_uint64()
        check(load_library().tr_scene_debug_line_bins(self._h, C.byref(nt), C.byref(ne)))
        return int(nt.value), int(ne.value)

    # --- projector (tr_scene_projector / tr_scene_get_projector) --------------------------------------
    def _projector_args(self, who, params, image, occluder, mode, opacity, soft, depth_bias, width, height, format, stride):
        """(params, image address, stride, occluder handle) of a projector call.  `params`: ProjectorParams, or the matrix
        m, completed here from the image's shape, the keywords and whether there is an occluder."""
        src, fmt, w, h, st = self._layer_source(image, who, width, height, format, stride)
        ch = 4 if fmt == "rgba8" else 3
        if occluder is not None and not isinstance(occluder, Scene):
            raise ValueError("%s: occluder must be a Scene" % who)
        if isinstance(params, ProjectorParams):
            if (params.pw, params.ph, params.channels) != (w, h, ch):
                raise ValueError("%s: image must be [ph, pw, channels] of the params" % who)
            p = params
        else:
            p = projector_params(params, w, h, ch, mode, opacity, occluder is not None, soft, depth_bias, who)
        return p, src, (st if st else w * ch), (occluder._h if occluder is not None else None)

    def projector(self, params, image, occluder=None, out=None, mode="add", opacity=256, soft=False, depth_bias=0.0, width=None, height=None,
                  format="rgb8", stride=0):
        """tr_scene_projector: casts `image` onto the drawn pixels of the current frame on the device from a second camera
        -- a slide projector, a decal, a light cookie; with `occluder`, a Scene of the image's size rendered from the
        projector's camera (store_depth=True spares a depth-only repeat; it may be this scene), its depth shadows the
        light.  `params`: projector_params(..), or just the matrix m (projector_matrix) with mode, opacity, soft and
        depth_bias given here.  `image` as for layer: a torch uint8 tensor [ph, pw, 3 | 4] on the scene's device, a
        page-locked array of the scene's (pinned_layer), or a device address (int) with width, height, format and
        stride.  out=None: in place, by the kernel itself -- every later consumer sees the result; z, winner words and
        the shadow buffer stay.  Otherwise `out` is a device pointer (int) or tensor of 3 * W * H bytes apart from every
        frame buffer of the scene, or an array from pinned_frame, and the scene's frame stays as it is.  Asynchronous:
        the result is there after sync() -- keep `image` alive until then.  Band scenes are refused.
        projector_host is the rule."""
        p, src, st, occ = self._projector_args("tr_scene_projector", params, image, occluder, mode, opacity, soft, depth_bias, width, height, format, stride)
        ptr = self._target_pointer(out, "out must be a contiguous tensor of at least 3 * width * height bytes")
        check(load_library().tr_scene_projector(self._h, C.addressof(p), src, st, occ, ptr))
        return out

    def get_projector(self, params, image, occluder=None, strict=True, mode="add", opacity=256, soft=False, depth_bias=0.0, width=None, height=None,
                      format="rgb8", stride=0):
        """tr_scene_get_projector: the current frame with `image` cast on it on the device (arguments as for projector), as
        an [H, W, 3] uint8 array.  Synchronizes; the scene's frame stays as it is."""
        p, src, st, occ = self._projector_args("tr_scene_get_projector", params, image, occluder, mode, opacity, soft, depth_bias, width, height, format,
                                               stride)
        return self._image("tr_scene_get_projector", strict, C.addressof(p), src, st, occ)

    def debug_projector_launches(self):
        """tr_scene_debug_projector_launches: the k_projector launches this scene has enqueued so far (the kernel has no
        entry in profile_read)."""
        return check(load_library().tr_scene_debug_projector_launches(self._h))

    # --- relight (tr_scene_relight / tr_scene_get_relit) ----------------------------------------------
    def relight(self, params, lights=(), out=None):
        """tr_scene_relight: lays up to 8 coloured lights (light_directional, light_point, light_spot) with their
        highlights on the drawn pixels of the current frame on the device, from normals recovered out of the frame's own
        depth.  params: relight_params(uniforms of prepare_uniforms(2, ..) for the frame's camera, eye, ..).  out=None:
        in place, by the kernel itself -- every later consumer sees the result; z, winner words and the shadow buffer
        stay.  Otherwise `out` is a device pointer (int) or tensor of 3 * W * H bytes apart from every frame buffer of
        the scene, or an array from pinned_frame, and the scene's frame stays as it is.  Asynchronous: the result is there
        after sync().  Band scenes are refused.  relight_host is the rule."""
        _check_params(params, RelightParams, "tr_scene_relight", "relight_params")
        table, n = _light_table(lights, "tr_scene_relight")
        ptr = self._target_pointer(out, "out must be a contiguous tensor of at least 3 * width * height bytes")
        check(load_library().tr_scene_relight(self._h, C.addressof(params), table, n, ptr))
        return out

    def get_relit(self, params, lights=(), strict=True):
        """tr_scene_get_relit: the current frame with the lights laid on it on the device (arguments as for relight), as an
        [H, W, 3] uint8 array.  Synchronizes; the scene's frame stays as it is."""
        _check_params(params, RelightParams, "tr_scene_get_relit", "relight_params")
        table, n = _light_table(lights, "tr_scene_get_relit")
        return self._image("tr_scene_get_relit", strict, C.addressof(params), table, n)

    def debug_relight_launches(self):
        """tr_scene_debug_relight_launches: the k_relight launches this scene has enqueued so far (the kernel has no
        entry in profile_read)."""
        return check(load_library().tr_scene_debug_relight_launches(self._h))

    def project(self, points):
        """Model-space points [n, 3] as the scene's last camera (set_camera) places them: project_points under
        prepare_uniforms(0, ..) of the scene's size.  Returns (xy, z, ok)."""
        cam = getattr(self, "_camera", None)
        if cam is None:
            raise ValueError("project: the scene has no camera yet (set_camera)")
        st, u = prepare_uniforms(0, self.width, self.height, getattr(self, "_light", (0.0, 0.0, 1.0)), *cam)
        check(st)
        return project_points(u, points)

    # --- distance field (tr_scene_distance / tr_scene_get_distance / tr_scene_distance_ramp / ..._ramped) ---
    def pinned_field(self):
        """A page-locked [H, W] uint16 array for distance (freed with the scene)."""
        return self._pinned_array((self.height, self.width, 2)).view(np.uint16).reshape(self.height, self.width)

    def distance(self, out, radius=None, seed="drawn", threshold=0, invert=False, params=None):
        """tr_scene_distance: the squared distance of every pixel of the current frame to its nearest seed (arguments:
        distance_params, or params built by it), computed on the device into `out`: a device pointer (int) at an even
        address or a tensor of 2 * W * H bytes apart from every frame buffer of the scene, or an array from pinned_field.
        uint16, index x + row * W with row 0 = top; DIST_FAR beyond the radius.  Asynchronous: the result is there after
        sync().  The frame stays as it is.  Band scenes are refused.  distance_host is the rule."""
        p = self._distance_params("tr_scene_distance", radius, seed, threshold, invert, params)
        if out is None:
            raise ValueError("distance: out must not be None (get_distance returns an array)")
        ptr = self._target_pointer(out, "out must be a contiguous tensor of at least 2 * width * height bytes", shape="[H, W]",
                                   source="pinned_field", nbytes=self.width * self.height * 2)
        check(load_library().tr_scene_distance(self._h, C.addressof(p), ptr))
        return out

    def get_distance(self, radius=None, seed="drawn", threshold=0, invert=False, strict=True, params=None):
        """tr_scene_get_distance: the field of the current frame (arguments as for distance) as an [H, W] uint16 array,
        row 0 = top.  Synchronizes; the scene's frame stays as it is."""
        p = self._distance_params("tr_scene_get_distance", radius, seed, threshold, invert, params)
        return self._image("tr_scene_get_distance", strict, C.addressof(p), out=np.empty((self.height, self.width), np.uint16))

    def distance_ramp(self, radius=None, step=256, seed="drawn", threshold=0, invert=False, mode="normal", opacity=256, far=(0, 0, 0, 0), repeat=False,
                      keep_seeds=False, out=None, params=None):
        """tr_scene_distance_ramp: blends the entry of the scene's ramp table (set_ramp; ramp_glow, ramp_stroke, ramp_rings)
        that each pixel's distance to the nearest seed chooses into the current frame on the device (arguments:
        distance_ramp_params, or params built by it).  out=None: in place, by the kernel itself; otherwise as for ramp.
        Asynchronous: the result is there after sync().  Band scenes are refused.  distance_ramp_host is the rule."""
        p = self._distance_ramp_params("tr_scene_distance_ramp", radius, step, seed, threshold, invert, mode, opacity, far, repeat, keep_seeds, params)
        ptr = self._target_pointer(out, "out must be a contiguous tensor of at least 3 * width * height bytes")
        check(load_library().tr_scene_distance_ramp(self._h, C.addressof(p), ptr))
        return out

    def get_distance_ramped(self, radius=None, step=256, seed="drawn", threshold=0, invert=False, mode="normal", opacity=256, far=(0, 0, 0, 0),
                            repeat=False, keep_seeds=False, strict=True, params=None):
        """tr_scene_get_distance_ramped: the current frame ramped by its distance field on the device (arguments as for
        distance_ramp), as an [H, W, 3] uint8 array.  Synchronizes; the scene's frame stays as it is."""
        p = self._distance_ramp_params("tr_scene_get_distance_ramped", radius, step, seed, threshold, invert, mode, opacity, far, repeat, keep_seeds,
                                       params)
        return self._image("tr_scene_get_distance_ramped", strict, C.addressof(p))

    @staticmethod
    def _distance_params(who, radius, seed, threshold, invert, params):
        if params is None:
            return distance_params(radius, seed, threshold, invert, who)
        _check_params(params, DistanceParams, who, "distance_params")
        return params

    @staticmethod
    def _distance_ramp_params(who, radius, step, seed, threshold, invert, mode, opacity, far, repeat, keep_seeds, params):
        if params is None:
            return distance_ramp_params(radius, step, seed, threshold, invert, mode, opacity, far, repeat, keep_seeds, who)
        _check_params(params, DistanceRampParams, who, "distance_ramp_params")
        return params

    # --- frame statistics (tr_scene_frame_stats / tr_scene_get_frame_stats) ---------------------------
    def pinned_stats(self):
        """A page-locked uint8 array of one tr_frame_stats record for frame_stats (freed with the scene); FrameStats(array)
        reads it after sync()."""
        return self._pinned_array((FRAME_STATS_BYTES,))

    def frame_stats(self, window=None, depth=False, z_lo=0.0, z_scale=1.0, out=None):
        """tr_scene_frame_stats: enqueue the reduction of the current frame to one record behind everything issued so far;
        the result is there after sync().  window, depth, z_lo, z_scale: stats_params.  `out`: a device pointer (int) to
        6192 bytes, or an array from pinned_stats; None takes a page-locked array of the scene's own (one, reused by every
        such call).  Returns `out` -- FrameStats(out) after sync() for an array.  Nothing of the scene is written; without
        depth no depth is read.  Band scenes give the record of their band's rows (frame_stats_merge joins them)."""
        p = stats_params(window, depth, z_lo, z_scale)
        if out is None:
            if getattr(self, "_stats_out", None) is None:
                self._stats_out = self.pinned_stats()
            out = self._stats_out
        ptr = self._out_pointer(out, "out", "6192-byte", "pinned_stats", FRAME_STATS_BYTES)
        check(load_library().tr_scene_frame_stats(self._h, C.addressof(p), ptr))
        return out

    def get_frame_stats(self, window=None, depth=False, z_lo=0.0, z_scale=1.0, strict=True):
        """tr_scene_get_frame_stats: the record of the current frame as a FrameStats.  Synchronizes."""
        p = stats_params(window, depth, z_lo, z_scale)
        out = np.zeros(FRAME_STATS_BYTES, np.uint8)
        code = load_library().tr_scene_get_frame_stats(self._h, C.addressof(p), out.ctypes.data)
        if strict:
            check(code)
        self.last_status = code
        return FrameStats(out)

    def debug_stats_grid(self, cap=0):
        """tr_scene_debug_stats_grid: every later k_stats launch of the scene starts at most `cap` workgroups (0: no cap, the
        default), so that each walks more tiles and k_stats_finish sums fewer slots; the record does not change.  Returns
        the number of workgroups of the scene's most recent k_stats launch, 0 if there has been none."""
        if isinstance(cap, bool) or not isinstance(cap, (int, np.integer)) or not 0 <= cap <= 0xFFFFFFFF:
            raise ValueError("debug_stats_grid: cap must be an integer 0..2^32 - 1")
        return check(load_library().tr_scene_debug_stats_grid(self._h, int(cap)))

    # --- dynamic textures (tr_scene_set_texture*) ---------------------------------------------------
    def _texture_shape(self, which):
        if isinstance(which, bool) or not isinstance(which, (int, np.integer)) or not 0 <= which <= 3:
            raise ValueError("which must be 0..3 (texture, normal_map, normal_map_tangent, specular_map)")
        return self._tex_shapes[int(which)]

    def set_texture(self, which, image):
        """tr_scene_set_texture: image `which` (0..3 in the constructor's order) becomes the uint8 [h, w, 3] array `image`,
        which must have the size of the image it replaces.  Renders issued from now on draw what a scene created with that
        image draws; frames issued earlier (held-back ones too) keep the old one.  Asynchronous; the array is copied."""
        shape = self._texture_shape(which)
        a = np.ascontiguousarray(image, np.uint8)
        if a.shape != shape:
            raise ValueError("set_texture: the image is %r, texture %d is %r (a texture keeps its size)" % (a.shape, which, shape))
        img = _lib.ImageRgb8(a.ctypes.data_as(C.POINTER(C.c_uint8)), a.shape[1], a.shape[0])
        check(load_library().tr_scene_set_texture(self._h, int(which), C.byref(img)))

    def set_texture_device(self, which, ptr, w, h, producer=None):
        """tr_scene_set_texture_device: the same from 3 * w * h bytes of device memory at `ptr` (int), e.g. the target of
        resolve_into / accumulate_into / depth_of_field(out=...).  producer: the Scene whose stream wrote it (the repack is
        ordered behind its work); None: the caller guarantees the memory is complete with respect to this scene's stream."""
        self._texture_shape(which)
        if producer is not None and not isinstance(producer, Scene):
            raise ValueError("set_texture_device: producer must be a Scene or None")
        check(load_library().tr_scene_set_texture_device(self._h, int(which), int(ptr) if ptr is not None else None, int(w), int(h),
                                                         producer._h if producer is not None else None))

    def set_texture_from(self, src, which=0):
        """tr_scene_set_texture_from_frame: the current frame of scene `src` (this scene itself is allowed: feedback) becomes
        image `which`; src's frame size must be the texture's size.  Nothing leaves the device."""
        self._texture_shape(which)
        if not isinstance(src, Scene):
            raise ValueError("set_texture_from: src must be a Scene")
        check(load_library().tr_scene_set_texture_from_frame(self._h, int(which), src._h))

    def read_texture(self, which):
        """tr_scene_read_texture: image `which` as the scene holds it now, uint8 [h, w, 3].  Synchronizes."""
        out = np.empty(self._texture_shape(which), np.uint8)
        check(load_library().tr_scene_read_texture(self._h, int(which), out.ctypes.data))
        return out

    def debug_texel_set(self):
        """tr_scene_debug_texel_set: the scene's texel set as uint32 words (empty: the scene has none).  Synchronizes."""
        h, w = self._tex_shapes[0][:2]
        cap = ((w + 3) // 4) * ((h + 1) // 2) * 32 + ((w + 7) // 8) * ((h + 3) // 4) * 32
        words = np.zeros(cap, np.uint32)
        n = check(load_library().tr_scene_debug_texel_set(self._h, words.ctypes.data, cap))
        return words[:n].copy()

    def host_buffer_written(self, out):
        """Tells the scene that the caller has written into a pinned_frame() array (it then assumes nothing about
        the array's content at the next get_frame_buffer_async)."""
        check(load_library().tr_scene_host_buffer_written(self._h, out.ctypes.data))

    def get_z_buffer(self, strict=True):
        return self._image("tr_scene_get_z_buffer", strict)

    def get_shadow_buffer(self, strict=True):
        return self._image("tr_scene_get_shadow_buffer", strict)

    # --- parity taps / device-resident access -------------------------------------------------
    def _raw(self, fn, dtype):
        out = np.empty((self.height, self.width), dtype)
        check(getattr(load_library(), fn)(self._h, out.ctypes.data))
        return out

    def read_z_f32(self):
        return self._raw("tr_scene_read_z_f32", np.float32)

    def read_shadow_f32(self):
        return self._raw("tr_scene_read_shadow_f32", np.float32)

    def read_winner_u32(self):
        return self._raw("tr_scene_read_winner_u32", np.uint32)

    def sync(self):
        return check(load_library().tr_scene_sync(self._h))

    def flush(self):
        """Hand every render issued so far to the device without waiting (renders may be held back in batches)."""
        return check(load_library().tr_scene_flush(self._h))

    def frame_buffer_device(self):
        return load_library().tr_scene_frame_buffer_device(self._h)

    def set_frame_buffer_device(self, ptr):
        """Renders issued from now on write the device buffer at `ptr` (None: the library's own)."""
        check(load_library().tr_scene_set_frame_buffer_device(self._h, ptr))

    def set_stream(self, stream):
        check(load_library().tr_scene_set_stream(self._h, stream))

    def debug_tile_stamps(self):
        """[n_tiles, 8] uint64: start, end (100 MHz ticks), polygons in the bin, hardware id, bin staged, coverage done."""
        cap = ((self.width + 127) // 128) * ((self.height + 7) // 8)
        out = np.zeros((cap, 8), np.uint64)
        n = check(load_library().tr_scene_debug_tile_stamps(self._h, out.ctypes.data, cap))
        return out[:n]

    def band_tiles(self, frame_buffer_device=None):
        """tr_scene_band_tiles: the tiles of one of the frame buffers this scene has rendered into (None: the current
        one) with their cleared-colour flags -- what PeerExchange.all_gather_tiles sends by."""
        out = _lib.BandTiles()
        check(load_library().tr_scene_band_tiles(self._h, frame_buffer_device, C.byref(out)))
        return out

    def profile_enable(self, on=True):
        check(load_library().tr_scene_profile_enable(self._h, 1 if on else 0))

    def profile_read(self):
        buf = (_lib.KernelTime * 32)()
        n = check(load_library().tr_scene_profile_read(self._h, buf, 32))
        return {buf[i].name.decode(): {"launches": int(buf[i].launches), "total_ms": float(buf[i].total_ms),
                                       "frames": int(buf[i].frames)}
                for i in range(n)}


def _frame_intervals(self, cap=1 << 16):
    """Microseconds between the completions of consecutive profiled frames (float32 array)."""
    out = np.zeros(cap, np.float32)
    n = check(load_library().tr_scene_profile_frame_intervals(self._h, out.ctypes.data, cap))
    return out[:n]


Scene.profile_frame_intervals = _frame_intervals


def band_rows(height, n_ranks, rank):
    """Output rows [row0, row1) rank `rank` of `n_ranks` renders (tr_band_rows, include/tiny_renderer.h)."""
    r0, r1 = C.c_uint32(), C.c_uint32()
    check(load_library().tr_band_rows(height, n_ranks, rank, C.byref(r0), C.byref(r1)))
    return int(r0.value), int(r1.value)


def prepare_uniforms(kind, width, height, light, look_from, look_at, up, uniforms=None):
    """shader.rs:183-279 on the host (no GPU needed).  Returns (status, Uniforms)."""
    u = uniforms if uniforms is not None else _lib.Uniforms()
    st = load_library().tr_prepare_uniforms(kind, C.byref(u), width, height, _f3(light),
                                            _f3(look_from), _f3(look_at), _f3(up))
    return st, u
