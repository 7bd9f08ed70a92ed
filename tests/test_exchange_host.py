"""GradBucketReducer.exchange() -- the staged gradient exchange of the two-graph data-parallel step -- on CPU tensors over gloo, two ranks.

The gradients lie in one flat buffer the way train.FlatAdamW lays them out; nothing fires the reducer's hooks' launches (enabled = False, as
under the captured step), so every all-reduce seen here comes from exchange().  Each rank records the collectives it issues by wrapping
torch.distributed.all_reduce and mapping the tensor's address to its bucket."""
import os
import socket

import torch
import torch.distributed as dist
import torch.multiprocessing as mp


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


SHAPES = [(32, 16), (32,), (7,), (33, 5), (32, 32), (1,), (2, 3, 5)]  # odd sizes: the 4-float padding of the flat layout is in play


def _grads(rank, rnd):
    g = torch.Generator().manual_seed(1000 * rnd + rank)
    return [torch.randn(s, generator=g) for s in SHAPES]


def _worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from vmg_amd.train import GradBucketReducer
    params = [torch.nn.Parameter(torch.zeros(s)) for s in SHAPES]
    offs, total = [], 0
    for p in params:
        offs.append(total)
        total += (p.numel() + 3) // 4 * 4
    gflat = torch.zeros(total)
    for p, o in zip(params, offs):
        p.grad = gflat[o:o + p.numel()].view_as(p)
    red = GradBucketReducer(params, bucket_bytes=512, flat_grad=gflat, offsets=offs)
    red.enabled = False
    order = []
    real = dist.all_reduce

    def logged(t, *a, **k):
        order.append([i for i, f in enumerate(red.flat) if f.data_ptr() == t.data_ptr() and f.numel() == t.numel()])
        return real(t, *a, **k)
    dist.all_reduce = logged
    outs, orders, states = [], [], []
    for rnd in range(2):  # the second round shows that the first left the reducer reset
        del order[:]
        gflat.zero_()
        for p, g in zip(params, _grads(rank, rnd)):
            p.grad.copy_(g)
        if rnd == 1 and rank == 1:
            red._on_grad(params[0])  # a hook that fires while disabled must not move any state
        red.exchange()
        outs.append([p.grad.numpy().copy() for p in params])
        orders.append(list(order))
        states.append((list(red.pending) == [len(b) for b in red.buckets], len(red.works), len(red._seen)))
    dist.all_reduce = real
    q.put((rank, outs, orders, states, len(red.buckets), float(gflat.sum())))
    dist.barrier()
    dist.destroy_process_group()


def test_exchange_reduces_every_bucket_in_index_order():
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=120) for _ in range(world)], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    nb = res[0][4]
    assert nb >= 3
    for rank, outs, orders, states, nb_r, _ in res:
        assert nb_r == nb
        for rnd in range(2):
            assert orders[rnd] == [[i] for i in range(nb)], f"rank {rank} round {rnd}: launch order {orders[rnd]}"
            assert states[rnd] == (True, 0, 0), f"rank {rank} round {rnd}: the reducer was not left reset"
            for i, s in enumerate(SHAPES):
                want = (_grads(0, rnd)[i] + _grads(1, rnd)[i]) / 2  # (SUM then one divide, in fp32: exactly this expression)
                assert torch.equal(torch.from_numpy(outs[rnd][i]), want), f"rank {rank} round {rnd}: tensor {i}"


def test_exchange_without_a_process_group_is_a_no_op_and_needs_the_flat_buffer():
    """A lone process (no process group) has nothing to exchange: the gradients stay, the state is reset.  A reducer whose gradients are not in
    one flat buffer refuses."""
    import pytest
    from vmg_amd.train import GradBucketReducer
    from vmg_amd.wgrad import DEFERRED
    saved = list(DEFERRED.callbacks)
    try:
        params = [torch.nn.Parameter(torch.zeros(s)) for s in SHAPES]
        offs, total = [], 0
        for p in params:
            offs.append(total)
            total += (p.numel() + 3) // 4 * 4
        gflat = torch.zeros(total)
        for p, o, g in zip(params, offs, _grads(0, 0)):
            p.grad = gflat[o:o + p.numel()].view_as(p)
            p.grad.copy_(g)
        red = GradBucketReducer(params, bucket_bytes=512, flat_grad=gflat, offsets=offs)
        red._on_grad(params[0])
        assert len(red._seen) == 1
        red.exchange()
        assert len(red._seen) == 0 and red.works == [] and red.pending == [len(b) for b in red.buckets]
        for p, g in zip(params, _grads(0, 0)):
            assert torch.equal(p.grad, g)
        with pytest.raises(RuntimeError, match="flat"):
            GradBucketReducer([torch.nn.Parameter(torch.zeros(3))], bucket_bytes=512).exchange()
    finally:
        DEFERRED.callbacks[:] = saved
