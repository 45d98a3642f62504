"""The two ways tr_scene.cpp draws a frame -- run_pass (one pass of one frame, arguments by value) and run_group (g frames
times the pipeline's passes, arguments in a device table) -- fill the same SetupArgs / TileArgs and queue the same chain
k_lit, k_setup, k_order, k_bin.  These cases pin what that shared code decides and the other suites reach only in
passing: the paths agree frame for frame, every launch leaves the profile record it should, an empty mesh ends its chain
with k_order, a depth-only repeat on a lit scene runs the pass's own closure without k_lit, an accumulating render after
a group depth-tests against real z, the tile stamps reach both paths, and a pose's rows are the ones both paths draw.

Small frames only (256x64: whole tiles; 250x70: a ragged edge in x and y), the 576-polygon sphere, everything
np.array_equal against the CPU oracle.  The specular closure's colour is compared with the oracle where the device powf
is the host's (tr_specular_exact), and between the paths always."""
import numpy as np
import pytest

from tests import helpers as H

pytestmark = pytest.mark.gpu

SIZES = ((256, 64), (250, 70))
PIPES = ("default", "phong", "normal_map", "specular", "darboux", "shadow", "occlusion")
TWO_PASS = ("shadow", "occlusion")
N = 3
F32_MIN_BITS = 0xFF7FFFFF
NO_WINNER = 0xFFFFFFFF


def views(n=N, cam0=0.2, light0=-0.4):
    """[n, 12]: light, look_from, look_at, up per frame; every frame differs from its neighbours."""
    p = np.zeros((n, 12), np.float32)
    for i in range(n):
        p[i, 0:3] = H.light(light0 + 0.3 * i)
        p[i, 3:6], p[i, 6:9], p[i, 9:12] = H.camera(cam0 + 0.45 * i)
    return p


def colour_is_exact(pipe):
    import tiny_renderer_amd as T
    return pipe != "specular" or bool(T.load_library().tr_specular_exact())


_ORACLE = {}


def oracle_frames(key, W, Hh, mesh, texs, pipe, p):
    """Per frame (rgb, z bits, shadow bits or None, winner words) of the per-frame protocol on the oracle; computed once
    per `key` and shared, never written."""
    k = (key, W, Hh, pipe, p.tobytes())
    if k not in _ORACLE:
        from oracle import oracle as O
        cpu = O.Scene(W, Hh, mesh, texs, pipe)
        out = []
        for q in p:
            cpu.clear()
            cpu.set_light_direction(q[0:3])
            cpu.set_camera(q[3:6], q[6:9], q[9:12])
            assert cpu.render() == 0
            out.append((cpu.get_frame_buffer(), cpu.z_f32().view(np.uint32),
                        cpu.shadow_f32().view(np.uint32) if pipe in TWO_PASS else None, cpu.winner_u32()))
            assert out[-1][0].any(), "an empty frame proves nothing"
        cpu.close()
        _ORACLE[k] = out
    return _ORACLE[k]


def frame(s, q, clear=True):
    if clear:
        s.clear()
    s.set_light_direction(q[0:3])
    s.set_camera(q[3:6], q[6:9], q[9:12])
    s.render()


def read(gpu, pipe, winner=False):
    """(rgb, z bits, shadow bits or None, winner words or None) of the scene's current frame."""
    return (gpu.get_frame_buffer(), gpu.read_z_f32().view(np.uint32),
            gpu.read_shadow_f32().view(np.uint32) if pipe in TWO_PASS else None, gpu.read_winner_u32() if winner else None)


def same(got, want, pipe, what, winner=False, colour=True):
    """`got` (read) against `want` (read, or an oracle frame): bit for bit."""
    assert np.array_equal(got[1], want[1]), "%s: z bits differ at %d pixels" % (what, int((got[1] != want[1]).sum()))
    if pipe in TWO_PASS:
        assert np.array_equal(got[2], want[2]), "%s: shadow bits differ at %d pixels" % (what, int((got[2] != want[2]).sum()))
    if winner:
        assert np.array_equal(got[3], want[3]), "%s: winner words differ at %d pixels" % (what, int((got[3] != want[3]).sum()))
    if colour:
        assert np.array_equal(got[0], want[0]), "%s: rgb differs at %d pixels" % (what, int((got[0] != want[0]).any(-1).sum()))


def kept_frames(gpu, pipe, n, winner=False):
    """The frames a render_frames call of n frames left behind, oldest first: [(index in the call, read)]."""
    kept = gpu.frames_kept()
    assert kept == min(n, gpu.frames_per_launch)
    out = []
    for back in range(kept - 1, -1, -1):
        gpu.select_frame(back)
        out.append((n - 1 - back, read(gpu, pipe, winner)))
    gpu.select_frame(0)
    return out


# --- agreement of the paths ---------------------------------------------------------------------

@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("pipe", PIPES)
def test_the_four_ways_agree(small_synthetic, pipe, size):
    """The same three frames by per-frame render() calls with automatic groups off (run_pass, a read after every frame)
    and on (the frames are held back and fused: run_group through flush_deferred; only the last can be seen), by
    render_frames (run_group, transient depth) and by render_frames on a scene that stores its depth."""
    import tiny_renderer_amd as T
    mesh, texs = small_synthetic
    W, Hh = size
    p = views()
    want = oracle_frames("sphere", W, Hh, mesh, texs, pipe, p)
    exact = colour_is_exact(pipe)

    one = T.Scene(W, Hh, mesh, texs, pipe, auto_group=False)
    per_frame = []
    for i in range(N):
        frame(one, p[i])
        per_frame.append(read(one, pipe))
        same(per_frame[i], want[i], pipe, "render(), frame %d, against the oracle" % i, colour=exact)
    assert one.sync() == 0
    one.close()

    held = T.Scene(W, Hh, mesh, texs, pipe, frames_per_launch=4)
    for i in range(N):
        frame(held, p[i])
    last = read(held, pipe)
    assert held.sync() == 0
    held.close()
    same(last, want[N - 1], pipe, "render() held back, last frame, against the oracle", colour=exact)
    same(last, per_frame[N - 1], pipe, "render() held back against render()")

    for store_depth in (False, True):
        grp = T.Scene(W, Hh, mesh, texs, pipe, frames_per_launch=4, store_depth=store_depth)
        grp.render_frames(p)
        assert grp.sync() == 0
        got = kept_frames(grp, pipe, N)
        assert [i for i, _ in got] == list(range(N))
        for i, f in got:
            what = "render_frames%s, frame %d" % (" storing depth" if store_depth else "", i)
            same(f, want[i], pipe, what + ", against the oracle", colour=exact)
            same(f, per_frame[i], pipe, what + ", against render()")
        grp.close()


@pytest.mark.parametrize("pipe", PIPES)
def test_winner_words_agree(small_synthetic, pipe):
    """With the winner tap both render() and render_frames go frame by frame through run_pass (the tap is a single
    buffer); a group never has one.  Winner words, z, shadow buffer and colour, 250x70."""
    import tiny_renderer_amd as T
    mesh, texs = small_synthetic
    W, Hh = SIZES[1]
    p = views()
    want = oracle_frames("sphere", W, Hh, mesh, texs, pipe, p)
    exact = colour_is_exact(pipe)
    assert len(np.unique(want[0][3][want[0][3] != NO_WINNER])) > 10
    one = T.Scene(W, Hh, mesh, texs, pipe, winner_tap=True, auto_group=False)
    per_frame = []
    for i in range(N):
        frame(one, p[i])
        per_frame.append(read(one, pipe, True))
        same(per_frame[i], want[i], pipe, "render(), frame %d, against the oracle" % i, winner=True, colour=exact)
    one.close()
    call = T.Scene(W, Hh, mesh, texs, pipe, winner_tap=True)
    call.render_frames(p)
    assert call.sync() == 0
    got = read(call, pipe, True)   # (one buffer: the last frame's words)
    same(got, want[N - 1], pipe, "render_frames, last frame, against the oracle", winner=True, colour=exact)
    same(got, per_frame[N - 1], pipe, "render_frames against render()", winner=True)
    call.close()


# --- profile records ------------------------------------------------------------------------------

def records(prof):
    return {k: (v["launches"], v["frames"]) for k, v in prof.items()}


# {kernel: (launches, frames)} of three frames: pass by pass on the per-frame path, one launch per kernel and pass for
# the group.  k_lit only under TR_LIT=1, once per frame; the depth pass's tile kernel has an entry of its own.
PER_FRAME = {
    "phong": {"k_setup": (3, 3), "k_order": (3, 3), "k_bin": (3, 3), "k_tile": (3, 3)},
    "shadow": {"k_setup": (6, 6), "k_order": (6, 6), "k_bin": (6, 6), "k_tile": (3, 3), "k_tile_depth": (3, 3)},
    "normal_map": {"k_lit": (3, 3), "k_setup": (3, 3), "k_order": (3, 3), "k_bin": (3, 3), "k_tile": (3, 3)},
}
GROUP = {
    "phong": {"k_setup": (1, 3), "k_order": (1, 3), "k_bin": (1, 3), "k_tile": (1, 3)},
    "shadow": {"k_setup": (2, 6), "k_order": (2, 6), "k_bin": (2, 6), "k_tile": (1, 3), "k_tile_depth": (1, 3)},
    "normal_map": {"k_lit": (1, 3), "k_setup": (1, 3), "k_order": (1, 3), "k_bin": (1, 3), "k_tile": (1, 3)},
}


@pytest.mark.parametrize("pipe", ["phong", "shadow", "normal_map"])
def test_profile_records_of_each_path(small_synthetic, monkeypatch, pipe):
    """Kernel kinds, launches and frames of three frames under profiling, per path.  Every frame is checked as well: the
    profiling arms queue the same work."""
    import tiny_renderer_amd as T
    monkeypatch.setenv("TR_LIT", "1")   # (read when a scene is made)
    mesh, texs = small_synthetic
    W, Hh = SIZES[1]
    p = views()
    want = oracle_frames("sphere", W, Hh, mesh, texs, pipe, p)

    one = T.Scene(W, Hh, mesh, texs, pipe, auto_group=False)
    one.profile_enable(True)
    for i in range(N):
        frame(one, p[i])
    assert one.sync() == 0
    got = records(one.profile_read())
    print("per-frame", pipe, got)
    assert got == PER_FRAME[pipe]
    same(read(one, pipe), want[N - 1], pipe, "render() under profiling")
    one.close()

    held = T.Scene(W, Hh, mesh, texs, pipe, frames_per_launch=4)
    held.profile_enable(True)
    for i in range(N):
        frame(held, p[i])
    assert held.sync() == 0
    got = records(held.profile_read())
    print("held back", pipe, got)
    assert got == GROUP[pipe]
    same(read(held, pipe), want[N - 1], pipe, "render() held back under profiling")
    held.close()

    for store_depth in (False, True):
        grp = T.Scene(W, Hh, mesh, texs, pipe, frames_per_launch=4, store_depth=store_depth)
        grp.profile_enable(True)
        grp.render_frames(p)
        assert grp.sync() == 0
        got = records(grp.profile_read())
        print("group, store_depth", store_depth, pipe, got)
        assert got == GROUP[pipe]
        for i, f in kept_frames(grp, pipe, N):
            same(f, want[i], pipe, "render_frames under profiling, frame %d" % i)
        grp.close()


# --- empty mesh -------------------------------------------------------------------------------------

@pytest.mark.parametrize("profiling", [False, True], ids=["plain", "profiling"])
@pytest.mark.parametrize("pipe", ["phong", "shadow"])
def test_empty_mesh_on_both_paths(small_synthetic, pipe, profiling):
    """No polygons: the chain ends with k_order (k_bin has nothing to launch, so the chain's completion rides on k_order),
    the frame is the cleared frame, sync() is OK and the profile has no k_bin record."""
    import tiny_renderer_amd as T
    mesh, texs = small_synthetic
    empty = dict(mesh, idx=np.zeros((0, 9), np.uint32))
    W, Hh = SIZES[1]
    p = views()

    def cleared(s, what):
        fb, z, sh, _ = read(s, pipe)
        assert not fb.any(), what
        assert (z == F32_MIN_BITS).all(), what
        assert sh is None or (sh == F32_MIN_BITS).all(), what

    def no_k_bin(s, launches, what):
        if not profiling:
            return
        got = records(s.profile_read())
        print(what, pipe, got)
        n_passes = 2 if pipe in TWO_PASS else 1
        assert "k_bin" not in got, what
        assert got["k_setup"] == (launches * n_passes, N * n_passes) and got["k_order"] == got["k_setup"], what

    one = T.Scene(W, Hh, empty, texs, pipe, auto_group=False)
    one.profile_enable(profiling)
    for i in range(N):
        frame(one, p[i])
    assert one.sync() == 0
    no_k_bin(one, N, "render()")   # (before anybody reads z: that would repeat a pass for its depth)
    cleared(one, "render()")
    assert one.sync() == 0
    one.close()

    grp = T.Scene(W, Hh, empty, texs, pipe, frames_per_launch=4)
    grp.profile_enable(profiling)
    grp.render_frames(p)
    assert grp.sync() == 0
    no_k_bin(grp, 1, "render_frames")
    assert grp.frames_kept() == N
    for back in range(N):
        grp.select_frame(back)
        cleared(grp, "render_frames, frame -%d" % back)
    assert grp.sync() == 0
    grp.close()


# --- depth on demand on a lit scene ---------------------------------------------------------------------

@pytest.mark.parametrize("pipe", ["normal_map", "specular"])
def test_depth_on_demand_on_a_lit_scene(small_synthetic, monkeypatch, pipe):
    """A cleared frame leaves its depth on the chip; read_z_f32 repeats the colour pass for the depth alone.  On a scene
    whose closure runs per texel (k_lit) the repeat runs the pass's own closure, gets no lit arguments and launches no
    k_lit; colour and its fast-clear flags are as they were.  Once after a lone frame (fused_single), once after a group."""
    import tiny_renderer_amd as T
    monkeypatch.setenv("TR_LIT", "1")
    mesh, texs = small_synthetic
    W, Hh = SIZES[1]
    p = views()
    want = oracle_frames("sphere", W, Hh, mesh, texs, pipe, p)
    exact = colour_is_exact(pipe)

    one = T.Scene(W, Hh, mesh, texs, pipe, auto_group=False)
    one.profile_enable(True)
    frame(one, p[0])
    before = one.get_frame_buffer()
    z = one.read_z_f32().view(np.uint32)
    assert np.array_equal(z, want[0][1]), "lone frame: z bits differ at %d pixels" % int((z != want[0][1]).sum())
    after = one.get_frame_buffer()
    assert np.array_equal(after, before), "lone frame: the depth-only repeat changed the colour"
    if exact:
        assert np.array_equal(after, want[0][0])
    got = records(one.profile_read())
    print("lone", pipe, got)
    assert got["k_lit"] == (1, 1) and got["k_tile"] == (2, 2) and got["k_setup"] == (2, 2)   # (the frame, then its repeat)
    # the flags still describe the colour: the next cleared frame, which trusts them, is right
    frame(one, p[1])
    same(read(one, pipe), want[1], pipe, "the frame after the repeat", colour=exact)
    one.close()

    grp = T.Scene(W, Hh, mesh, texs, pipe, frames_per_launch=4)
    grp.profile_enable(True)
    grp.render_frames(p)
    assert grp.sync() == 0
    for back in range(N):
        grp.select_frame(back)
        before = grp.get_frame_buffer()
        z = grp.read_z_f32().view(np.uint32)
        assert np.array_equal(z, want[N - 1 - back][1]), "group, frame -%d: z bits differ at %d pixels" % (back, int((z != want[N - 1 - back][1]).sum()))
        after = grp.get_frame_buffer()
        assert np.array_equal(after, before), "group, frame -%d: the depth-only repeat changed the colour" % back
        if exact:
            assert np.array_equal(after, want[N - 1 - back][0])
    got = records(grp.profile_read())
    print("group", pipe, got)
    assert got["k_lit"] == (1, 3) and got["k_tile"] == (4, 6) and got["k_setup"] == (4, 6)   # (the group, then three repeats)
    grp.close()


# --- accumulating render after a group ---------------------------------------------------------------------

@pytest.mark.parametrize("pipe", ["phong", "shadow"])
def test_render_without_clear_onto_a_groups_last_frame(small_synthetic, pipe):
    """fresh = 0 through run_pass: the group's last frame has its depth made real first, then the render depth-tests
    against it and keeps the frame's colour where it loses."""
    import tiny_renderer_amd as T
    from oracle import oracle as O
    mesh, texs = small_synthetic
    W, Hh = SIZES[1]
    p = views()
    q = views(1, cam0=2.4, light0=0.8)[0]
    cpu = O.Scene(W, Hh, mesh, texs, pipe)
    frame(cpu, p[N - 1])
    frame(cpu, q, clear=False)
    want = (cpu.get_frame_buffer(), cpu.z_f32().view(np.uint32), cpu.shadow_f32().view(np.uint32) if pipe in TWO_PASS else None, None)
    first = oracle_frames("sphere", W, Hh, mesh, texs, pipe, p)[N - 1]
    assert (want[0] != first[0]).any() and (want[1] != first[1]).any(), "the second render changes nothing: no test"
    cpu.close()
    gpu = T.Scene(W, Hh, mesh, texs, pipe, frames_per_launch=4)
    gpu.render_frames(p)
    frame(gpu, q, clear=False)
    assert gpu.sync() == 0
    same(read(gpu, pipe), want, pipe, "render() without clear() after render_frames")
    gpu.close()


# --- tile stamps ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_tile_stamps_reach_both_paths(small_synthetic, size):
    """TileArgs::stamps on render() and on an explicit render_frames: every tile of the colour grid is stamped.  The kernel
    stamps tiles that hold polygons, so the sphere is scaled to reach every tile (checked on the oracle's frames)."""
    import tiny_renderer_amd as T
    mesh, texs = small_synthetic
    mesh = dict(mesh, pos=(mesh["pos"] * np.float32(1.5)).astype(np.float32))
    W, Hh = size
    p = views()
    want = oracle_frames("sphere x1.5", W, Hh, mesh, texs, "phong", p)
    ntx, nty = (W + H.TILE_W - 1) // H.TILE_W, (Hh + H.TILE_H - 1) // H.TILE_H
    for f in want:   # (z rows and tile rows both count from the bottom)
        drawn = f[1] != F32_MIN_BITS
        assert all(drawn[ty * H.TILE_H:(ty + 1) * H.TILE_H, tx * H.TILE_W:(tx + 1) * H.TILE_W].any()
                   for ty in range(nty) for tx in range(ntx)), "a tile without a drawn pixel: no test"

    def stamped(s, what):
        st = s.debug_tile_stamps()
        assert st.shape[0] == ntx * nty
        assert (st[:, 0] != 0).all() and (st[:, 1] != 0).all() and (st[:, 2] != 0).all(), (what, st[:, :3])

    one = T.Scene(W, Hh, mesh, texs, "phong", tile_stamps=True)
    frame(one, p[0])
    assert one.sync() == 0
    stamped(one, "render()")
    same(read(one, "phong"), want[0], "phong", "render() with stamps")
    one.close()
    grp = T.Scene(W, Hh, mesh, texs, "phong", tile_stamps=True)
    grp.render_frames(p)   # (one group; its first frame's workgroups write the stamps)
    assert grp.sync() == 0
    stamped(grp, "render_frames")
    same(read(grp, "phong"), want[N - 1], "phong", "render_frames with stamps")
    grp.close()


# --- posed frames --------------------------------------------------------------------------------------------

def morph_targets(mesh):
    """Two targets: an inflation, and a sine displacement along x by height with normal deltas of its own."""
    pos = np.asarray(mesh["pos"], np.float32).reshape(-1, 3)
    nrm = np.asarray(mesh["nrm"], np.float32).reshape(-1, 3)
    dp = np.zeros((2,) + pos.shape, np.float32)
    dn = np.zeros((2,) + nrm.shape, np.float32)
    dp[0] = pos * np.float32(0.2)
    dp[1, :, 0] = np.float32(0.12) * np.sin(np.float32(7.0) * pos[:, 1])
    dn[1, :, 1] = np.float32(-0.4) * np.cos(np.float32(7.0) * nrm[:, 1]) * nrm[:, 0]
    return dp, dn


POSES = np.array([[1.25, -0.6], [0.0, 1.0], [0.5, 0.5]], np.float32)


@pytest.mark.parametrize("pipe", ["phong", "shadow"])
def test_posed_frames_on_both_paths(small_synthetic, pipe):
    """A pose on a single frame (run_pass swaps the mesh's rows for the pose's behind blend_poses) and a pose per frame in a
    group of three (run_group takes the rows before it builds the frame's mesh): what scenes of the host-deformed mesh
    (tr_morph_mesh) render."""
    import tiny_renderer_amd as T
    mesh, texs = small_synthetic
    W, Hh = SIZES[1]
    p = views()
    dp, dn = morph_targets(mesh)
    want = []
    for i in range(N):
        pos, nrm = T.morph_mesh(mesh, dp, dn, POSES[i])
        want.append(oracle_frames("pose %d" % i, W, Hh, dict(mesh, pos=pos, nrm=nrm), texs, pipe, p[i:i + 1])[0])
    assert (want[0][1] != oracle_frames("sphere", W, Hh, mesh, texs, pipe, p)[0][1]).any(), "the pose changes nothing: no test"

    one = T.Scene(W, Hh, mesh, texs, pipe, auto_group=False)
    one.set_morph_targets(dp, dn)
    one.set_morph_weights(POSES[0])
    frame(one, p[0])
    same(read(one, pipe), want[0], pipe, "render() under a pose")
    one.close()

    grp = T.Scene(W, Hh, mesh, texs, pipe, frames_per_launch=4)
    grp.set_morph_targets(dp, dn)
    grp.render_frames(p, morph_weights=POSES)
    assert grp.sync() == 0
    for i, f in kept_frames(grp, pipe, N):
        same(f, want[i], pipe, "render_frames, a pose per frame, frame %d" % i)
    grp.close()
