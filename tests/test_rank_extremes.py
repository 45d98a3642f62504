"""The rank stage at the two ends of the frame sizes, on the device: frames below one 128 x 16 tile, down to one pixel --
narrower and lower than the window, a single row, a single column --, and frames with a side of 32768.

The frames are tests/extreme_cases.py's: noise in a caller's guarded buffer, drawn into without a clear.  The expectation
is rank_host over the scene's own snapshot (tests/test_rank_host.py pins it to numpy).  Every comparison is
np.array_equal."""
import numpy as np
import pytest

from tests import extreme_cases as EC
from tests import rank_cases as RC
from tests import test_composite as TC
from tests import test_dense_frames as TD
from tests import test_outline as TO

SIZES = EC.SMALL + ((32768, 17), (20, 32768))
ALL = RC.everything()
SETS = ("15x15_rank112", "3x3_rank4", "disc3_erode", "despeckle_disc3")


def extreme_scene(ms, W, Hh):
    return TD.dense_scene(EC.model(ms, W, Hh), W, Hh, EC.KIND, table=EC.table, draws=EC.draws(W, Hh))


@pytest.mark.gpu
@pytest.mark.parametrize("W,Hh", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_out_of_place_and_the_getter(small_synthetic, W, Hh):
    import torch
    import tiny_renderer_amd as T
    s, buf, f = extreme_scene(small_synthetic, W, Hh)
    n = W * Hh * 3
    dev = TO.device_buffer(n + 64)
    changed = False
    for name in SETS:
        for edge, border in RC.EDGES:
            p = RC.params(ALL[name], edge, border)
            want = T.rank_host(f["fb"], p)
            changed = changed or not np.array_equal(want, f["fb"])
            dev[:] = 0x5A
            torch.cuda.synchronize()
            s.rank(p, dev.data_ptr())
            assert s.sync() == 0
            raw = dev.cpu().numpy()
            got = raw[:n].reshape(want.shape)
            assert np.array_equal(got, want), "%s %s %r: %d bytes differ" % (name, edge, border, int((got != want).sum()))
            assert (raw[n:] == 0x5A).all(), "bytes behind the result were written"
            assert np.array_equal(s.get_ranked(p), want), "getter %s %s %r" % (name, edge, border)
    assert changed, "every expectation is the input"
    TD.in_buffer(buf, f["fb"])
    assert np.array_equal(TC.bits(s.read_z_f32()), TC.bits(f["z"])), "z changed"
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("W,Hh", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_in_place(small_synthetic, W, Hh):
    import tiny_renderer_amd as T
    s, buf, f = extreme_scene(small_synthetic, W, Hh)
    p = RC.params(ALL["15x15_rank112"], "border", RC.PAPER)
    want = T.rank_host(f["fb"], p)
    assert not np.array_equal(want, f["fb"])
    assert s.rank(p) is None and s.sync() == 0
    TD.in_buffer(buf, want)
    assert np.array_equal(s.get_frame_buffer(), want)
    assert not (TC.clean_flags(s) & TC.tiles_any(want[::-1].any(-1))).any(), "a tile with colour in it is flagged clean"
    assert np.array_equal(TC.bits(s.read_z_f32()), TC.bits(f["z"])), "z changed"
    s.close()
