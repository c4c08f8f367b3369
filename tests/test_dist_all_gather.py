"""dist.all_gather_dict / batch_dict_to_cuda (the reference's utils/dist.py:159-185) on CPU: two gloo ranks, and no process group."""
import os
import socket

import torch
import torch.distributed as dist
import torch.multiprocessing as mp


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _batch(rank):
    g = torch.Generator().manual_seed(40 + rank)
    return {"box_corners": torch.randn(2, 5, 8, 3, generator=g), "labels": torch.randint(0, 18, (2, 5), generator=g),
            "strided": torch.randn(3, 2, generator=g).t(), "scan_name": f"scene{rank}"}


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    from vdetr_amd.dist import all_gather_dict, init_distributed
    init_distributed("gloo")
    out = all_gather_dict(_batch(rank))
    # numpy (pickled by value): torch tensors would travel as shared-memory handles that die with the worker
    q.put((rank, {k: v.numpy().copy() if torch.is_tensor(v) else v for k, v in out.items()}))
    dist.barrier()
    dist.destroy_process_group()


def test_all_gather_dict_on_two_gloo_ranks():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    mine = [_batch(0), _batch(1)]
    for rank in (0, 1):
        assert list(res[rank]) == list(mine[0])
        for key in ("box_corners", "labels", "strided"):
            want = torch.cat((mine[0][key], mine[1][key]), dim=0)
            assert torch.equal(torch.from_numpy(res[rank][key]), want), (rank, key)
        assert res[rank]["scan_name"] == f"scene{rank}"       # not a tensor: passed through


def test_all_gather_dict_without_a_process_group_is_the_identity():
    from vdetr_amd.dist import all_gather_dict, batch_dict_to_cuda
    assert not dist.is_initialized()
    batch = _batch(0)
    out = all_gather_dict(batch)
    assert list(out) == list(batch) and all(out[k] is batch[k] for k in batch)
    moved = batch_dict_to_cuda({"a": torch.ones(2), "b": [torch.zeros(1), torch.zeros(2)], "c": [], "d": "name", "e": [1, 2]}, "cpu")
    assert torch.equal(moved["a"], torch.ones(2)) and [t.shape[0] for t in moved["b"]] == [1, 2]
    assert moved["c"] == [] and moved["d"] == "name" and moved["e"] == [1, 2]
