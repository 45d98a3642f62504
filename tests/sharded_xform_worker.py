"""Worker of tests/test_instance_transforms.py::test_sharded_transformed_two_ranks_one_gpu: one RANK of a two-rank
ShardedScene whose ranks share one GPU (started twice by torch.distributed.run; gloo carries the control messages, the
library's peer transport the bands).  Every rank draws the same transform tables -- set_instance_transforms with the
per-frame protocol, render_frames(instance_transforms=...) in groups, one rank with pools too small so that a group is
rendered again with its tables -- and compares the assembled frame with a single-GPU scene's frame, bit for bit.
    python -m torch.distributed.run --nproc-per-node 2 ... tests/sharded_xform_worker.py peer|peer-sparse"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

import tiny_renderer_amd as T  # noqa: E402
from tests import helpers as H  # noqa: E402
from tests.test_instance_transforms import _crowd, _table  # noqa: E402
from tiny_renderer_amd.sharded import ShardedScene  # noqa: E402


def main():
    exchange = sys.argv[1] if len(sys.argv) > 1 else "peer"
    torch.cuda.set_device(0)
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    assert world >= 2, "this worker is about a rank that HAS peers"
    mesh, texs = T.synthetic_scene(n_lat=12, n_lon=24, tex_size=256)
    W, Hh = 512, 384
    table = _table()

    def frames(n, c0):
        p = np.zeros((n, 12), np.float32)
        for i in range(n):
            p[i, 0:3] = H.light(0.2 + 0.1 * i)
            p[i, 3:6], p[i, 6:9], p[i, 9:12] = H.camera(c0 + 0.3 * i)
        return p

    def single(pipe, t, q):
        one = T.Scene(W, Hh, mesh, texs, pipe, instance_transforms=t)
        one.clear(), one.set_light_direction(q[0:3]), one.set_camera(q[3:6], q[6:9], q[9:12]), one.render()
        out = one.get_frame_buffer()
        one.close()
        return out

    def check(s, pipe, t, q, what):
        got = s.get_frame_buffer()    # collective; the WHOLE frame, all bands, on every rank
        want = single(pipe, t, q)
        assert want.any(), "empty frame"
        assert np.array_equal(got, want), "rank %d, %s %s: %d pixels differ (%s)" % (rank, exchange, pipe, int((got != want).any(-1).sum()), what)

    # caps (64, 0): only rank 0's pools are too small -- its group overflows and ALL ranks render it again, tables included
    for pipe, caps in (("phong", (0, 0)), ("shadow", (0, 0)), ("phong", (64, 0))):
        s = ShardedScene(W, Hh, mesh, texs, pipe, exchange=exchange, frames_per_launch=4, bin_capacity=caps[rank % 2])
        s.set_instance_transforms(table)
        p = frames(3, 0.0)
        for i in range(3):
            s.clear(), s.set_light_direction(p[i, 0:3]), s.set_camera(p[i, 3:6], p[i, 6:9], p[i, 9:12]), s.render()
        check(s, pipe, table, p[-1], "three per-frame renders")
        p = frames(9, 0.5)
        crowd = _crowd(9)
        s.render_frames(p, instance_transforms=crowd)       # groups of 4, 4, 1
        check(s, pipe, crowd[-1], p[-1], "after 9 frames in groups")
        s.clear(), s.set_light_direction(p[3, 0:3]), s.set_camera(p[3, 3:6], p[3, 6:9], p[3, 9:12]), s.render()
        check(s, pipe, crowd[-1], p[3], "per-frame render after a group call: the last table is current")
        s.close()
    dist.barrier()
    dist.destroy_process_group()
    print("rank %d OK" % rank)


try:
    main()
except BaseException:
    import traceback
    # (to STDOUT, with the rank: the launcher's own traceback buries a rank's stderr)
    print("RANK %s FAILED\n%s" % (os.environ.get("RANK", "?"), traceback.format_exc()), flush=True)
    raise
