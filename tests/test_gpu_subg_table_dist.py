"""dcor.dist.subg_table_distributed on the GPU: at world 1 over RCCL and as two gloo ranks sharing
cuda:0.  The gathered records equal one process's dcor.subgpanel.table_segments byte for byte."""
import os
import socket

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# (col_x, col_y, eps1, eps2, seed, rep_begin, reps): 14 replicates, so two ranks split inside a segment
RANK_SEGS = [(0, 1, 1.0, 1.0, 61, 0, 7), (2, 2, 0.2, 0.2, 62, 1001, 3), (1, 0, 2.0, 2.0, 63, 5, 0),
             (2, 0, 1.5, 0.5, 64, 2, 4)]
KW = dict(eta=(1.0, 0.5, 0.8), nsim=2000)


def _table(n=1003, p=3, seed=17):
    g = np.random.default_rng(seed)
    f = g.standard_normal(n)
    return np.asfortranarray(0.5 + 2.0 * (np.sqrt(0.5) * f[:, None] + np.sqrt(0.5) * g.standard_normal((n, p))))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_runs():
    from dcor.dist import subg_table_distributed
    D = _table()
    return [subg_table_distributed(D, RANK_SEGS, **KW).tobytes(),
            subg_table_distributed(D, [(1, 2, 1.0, 1.0, 65, 9, 1)], **KW).tobytes(),   # fewer items than ranks
            subg_table_distributed(D, []).tobytes()]


def _rank_expected():
    from dcor import subgpanel
    D = _table()
    return [subgpanel.table_segments(D, RANK_SEGS, **KW).tobytes(),
            subgpanel.table_segments(D, [(1, 2, 1.0, 1.0, 65, 9, 1)], **KW).tobytes(), b""]


def test_subg_table_distributed_rccl_world1():
    import torch
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()))
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        got = _rank_runs()
    finally:
        dist.destroy_process_group()
    want = _rank_expected()
    assert len(want[0]) == 14 * 48 and got == want


def _rank_worker(rank, world, port, q):
    import torch
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    q.put((rank, _rank_runs()))
    dist.destroy_process_group()


def test_subg_table_distributed_two_ranks_on_gpu():
    """Two gloo ranks sharing cuda:0: each runs its contiguous part of the flattened (segment,
    replicate) space in one native call; the gathered records are the one-process call's bytes."""
    import torch.multiprocessing as mp
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_rank_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=200) for _ in range(world))
    for p in procs:
        p.join(timeout=30)
        assert p.exitcode == 0
    want = _rank_expected()
    assert got[0] == want and got[1] == want
