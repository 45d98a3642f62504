"""tr_texel_set_host -- the texel set tr_scene_create builds (csrc/tr_texels.h), on the host -- against a numpy
restatement of the layout written from that header's comments:
  * words per texel: 4 for the closures that read a normal map (specular, normal_map, darboux), else 1;
  * blocks of 128 bytes: 8 x 4 texels (one word) or 4 x 2 (four words), row-major inside a block, blocks row-major;
  * word 0 = r | g << 8 | b << 16 of image 0, with image 3's first byte in bits 24..31 under `specular` alone;
  * words 1..3 = the f32 normal decoded from image 1 (darboux: image 2): channel / 255 - 0.5, normalised -- every
    operation rounded once in f32, the dot product as (x*x + y*y) + z*z;
  * padding texels of partial blocks are zero.
No GPU is needed."""
import ctypes as C

import numpy as np
import pytest

SIZES = [(1, 1), (7, 5), (8, 4), (9, 3), (130, 17)]   # (w, h)
PIPES = ["phong", "specular", "normal_map", "darboux"]
FOUR_WORDS = ("specular", "normal_map", "darboux")


def images(w, h, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(4)]


def numpy_set(pipe, texs):
    h, w = texs[0].shape[:2]
    K = 4 if pipe in FOUR_WORDS else 1
    bw, bh = (4, 2) if K == 4 else (8, 4)
    bpr, rows = -(-w // bw), -(-h // bh)
    out = np.zeros(bpr * rows * bw * bh * K, np.uint32)
    cy, cx = np.mgrid[0:h, 0:w]
    at = (((cy // bh) * bpr + cx // bw) * (bw * bh) + (cy % bh) * bw + cx % bw) * K
    t = [x.astype(np.uint32) for x in texs]
    word0 = t[0][..., 0] | (t[0][..., 1] << 8) | (t[0][..., 2] << 16)
    if pipe == "specular":
        word0 = word0 | (t[3][..., 0] << 24)
    out[at] = word0
    if K == 4:
        src = texs[2 if pipe == "darboux" else 1].astype(np.float32)
        f = np.float32
        n = src / f(255.0) - f(0.5)
        x, y, z = n[..., 0], n[..., 1], n[..., 2]
        length = np.sqrt((x * x + y * y) + z * z).astype(np.float32)
        with np.errstate(divide="ignore", invalid="ignore"):
            for k, c in enumerate((x, y, z)):
                out[at + 1 + k] = (c / length).astype(np.float32).view(np.uint32)
    return out, bpr


def set_host(pipe, texs, cap=None):
    """(status or word count, words, blocks_per_row) of a direct call."""
    import tiny_renderer_amd as T
    from tiny_renderer_amd import _lib
    L = T.load_library()
    keep = [np.ascontiguousarray(t) for t in texs]
    imgs = (_lib.ImageRgb8 * 4)(*[_lib.ImageRgb8(t.ctypes.data_as(C.POINTER(C.c_uint8)), t.shape[1], t.shape[0]) for t in keep])
    n_want = numpy_set(pipe, texs)[0].size
    cap = n_want if cap is None else cap
    words = np.full(max(cap, 1), 0xDEADBEEF, np.uint32)
    bpr = C.c_uint32(0xFFFFFFFF)
    n = L.tr_texel_set_host(pipe.encode(), imgs, words.ctypes.data, cap, C.byref(bpr))
    return n, words, bpr.value


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("pipe", PIPES)
def test_texel_set_host_matches_the_documented_layout(built, pipe, size):
    w, h = size
    texs = images(w, h, 7 * w + h)
    want, bpr_want = numpy_set(pipe, texs)
    n, words, bpr = set_host(pipe, texs)
    assert n == want.size          # an output array exactly as large as the set
    assert bpr == bpr_want
    assert np.array_equal(words[:n], want)
    # the wrapper returns the same words
    import tiny_renderer_amd as T
    got, bpr2 = T.texel_set_host(pipe, texs)
    assert bpr2 == bpr_want and np.array_equal(got, want)


@pytest.mark.parametrize("pipe", PIPES)
def test_texel_set_host_words_depend_on_the_right_images(built, pipe):
    """Word 0's top byte is the specular map's under `specular` alone; the normal words decode image 2 under `darboux` and
    image 1 under the others; nothing depends on an image the closure does not read; padding stays zero."""
    import tiny_renderer_amd as T
    w, h = 9, 3
    texs = images(w, h, 11)
    base, _ = T.texel_set_host(pipe, texs)
    K = 4 if pipe in FOUR_WORDS else 1
    rng = np.random.default_rng(5)
    for which in range(4):
        other = [t.copy() for t in texs]
        other[which] = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        other[which][..., 0] ^= 0x55   # (every texel's first byte differs)
        got, _ = T.texel_set_host(pipe, other)
        diff = (got != base).reshape(-1, K)
        changed = [bool(diff[:, k].any()) for k in range(K)]
        top = ((got.reshape(-1, K)[:, 0] ^ base.reshape(-1, K)[:, 0]) >> 24).any()
        low = ((got.reshape(-1, K)[:, 0] ^ base.reshape(-1, K)[:, 0]) & 0xFFFFFF).any()
        assert bool(low) == (which == 0)
        assert bool(top) == (which == 3 and pipe == "specular")
        if K == 4:
            nsrc = 2 if pipe == "darboux" else 1
            assert any(changed[1:]) == (which == nsrc)
    # padding: the words of texels outside the image are zero
    want, _ = numpy_set(pipe, texs)
    bw, bh = (4, 2) if K == 4 else (8, 4)
    bpr, rows = -(-w // bw), -(-h // bh)
    used = np.zeros(bpr * rows * bw * bh, bool)
    cy, cx = np.mgrid[0:h, 0:w]
    used[((cy // bh) * bpr + cx // bw) * (bw * bh) + (cy % bh) * bw + cx % bw] = True
    assert not base.reshape(-1, K)[~used].any() and (~used).any()
    assert np.array_equal(base, want)


def test_texel_set_host_errors(built):
    import tiny_renderer_amd as T
    L = T.load_library()
    texs = images(7, 5, 3)
    n_want = numpy_set("specular", texs)[0].size
    n, words, _ = set_host("specular", texs, cap=n_want - 1)
    assert n == -1 and L.tr_last_error()            # TR_E_INVALID: cap_words too small
    assert (words == 0xDEADBEEF).all()              # ... and nothing written
    n, _, _ = set_host("specular", texs, cap=0)
    assert n == -1
    uneven = [t.copy() for t in texs]
    uneven[2] = images(8, 5, 4)[0]
    with pytest.raises(T.TinyRendererError) as e:
        T.texel_set_host("specular", uneven)        # images of different sizes: such a scene has no set
    assert e.value.code == -1
    with pytest.raises(T.TinyRendererError) as e:
        T.texel_set_host("no_such_pipeline", texs)
    assert e.value.code == -2
