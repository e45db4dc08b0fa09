"""CPU: ring (context-parallel) attention with the float64 restatements as `ops`
(tests/merge_ref.py): what is checked here is the ring itself - which K/V shard meets which
queries under which mask, the zigzag layout, the merge per query half, the travelling dk / dv
accumulators and the autograd wiring - against the unsharded oracle within 1e-10.

* in-process, world 4: one thread per rank joined by queues (`ThreadRing`);
* world 2 over a gloo process group: the default `DistRing` (batch_isend_irecv);
* `zigzag_split` / `zigzag_gather` round trip, and the refusals of `ring_attention`.
"""
import os

import pytest
import torch
import torch.multiprocessing as mp

from tests import merge_ref as mr
from tests import sink_ref as sr
from tests.test_sharding import _free_port
from xf_flash_attention_cutlass_amd import sharding as sh

TOL = 1e-10
B, H, HK, D = 2, 4, 2, 16


def _split(x, world, rank, causal):
    if causal:
        return sh.zigzag_split(x, world, rank)
    n = x.shape[1] // world
    return x[:, rank * n:(rank + 1) * n]


def _gather(shards, causal):
    return sh.zigzag_gather(shards) if causal else torch.cat(shards, dim=1)


def _problem(world, c, seed=0):
    g = torch.Generator().manual_seed(seed)
    s = 2 * world * c
    q = torch.randn(B, s, H, D, generator=g, dtype=torch.float64)
    k = torch.randn(B, s, HK, D, generator=g, dtype=torch.float64)
    v = torch.randn(B, s, HK, D, generator=g, dtype=torch.float64)
    w = torch.randn(B, s, H, D, generator=g, dtype=torch.float64)
    return q, k, v, w


def _reference(q, k, v, w, sink, causal, softcap):
    leaves = [x.clone().requires_grad_(True) for x in (q, k, v)]
    if sink is not None:
        leaves.append(sink.clone().requires_grad_(True))
    out, _ = sr.sink_attention(leaves[0], leaves[1], leaves[2], leaves[3] if sink is not None else None,
                               causal=causal, softcap=softcap)
    return out.detach(), torch.autograd.grad(out, leaves, w)


def _rank_run(ring, world, q, k, v, w, sink, causal, softcap):
    """One rank's forward and backward through the autograd Function; returns its shards of
    (out, dq, dk, dv) and its share of dsink."""
    r = ring.rank
    leaves = [_split(x, world, r, causal).clone().requires_grad_(True) for x in (q, k, v)]
    s = None if sink is None else sink.clone().requires_grad_(True)
    out = sh.ring_attention(*leaves, causal=causal, softcap=softcap, sink=s, ops=mr.OracleOps, ring=ring)
    grads = torch.autograd.grad(out, leaves + ([s] if s is not None else []), _split(w, world, r, causal))
    return (out.detach(), *grads)


def _check(per_rank, ref_out, ref_grads, causal, has_sink):
    out = _gather([p[0] for p in per_rank], causal)
    assert (out - ref_out).abs().max().item() <= TOL
    for i, name in enumerate(("dq", "dk", "dv")):
        g = _gather([p[1 + i] for p in per_rank], causal)
        assert (g - ref_grads[i]).abs().max().item() <= TOL, name
    if has_sink:
        dsink = sum(p[4] for p in per_rank)               # the SUM all-reduce the docstring asks for
        assert (dsink - ref_grads[3]).abs().max().item() <= TOL


@pytest.mark.parametrize("c", [1, 5])
@pytest.mark.parametrize("feat", ["plain", "sink", "softcap"])
@pytest.mark.parametrize("causal", [False, True])
def test_ring_world4_in_process(causal, feat, c):
    world = 4
    q, k, v, w = _problem(world, c)
    sink = sr.sink_values(H, torch.float64) if feat == "sink" else None
    softcap = 3.0 if feat == "softcap" else 0.0
    ref_out, ref_grads = _reference(q, k, v, w, sink, causal, softcap)
    per_rank = mr.run_ranks(world, lambda ring: _rank_run(ring, world, q, k, v, w, sink, causal, softcap))
    _check(per_rank, ref_out, ref_grads, causal, sink is not None)


def test_ring_world1_with_ops_is_the_plain_problem():
    q, k, v, w = _problem(1, 3)
    sink = sr.sink_values(H, torch.float64)
    ref_out, ref_grads = _reference(q, k, v, w, sink, True, 0.0)
    per_rank = mr.run_ranks(1, lambda ring: _rank_run(ring, 1, q, k, v, w, sink, True, 0.0))
    _check(per_rank, ref_out, ref_grads, True, True)


def _gloo_worker(rank, world, port, causal, res):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        q, k, v, w = _problem(world, 3)                   # the same seed on every rank
        sink = sr.sink_values(H, torch.float64)
        mine = _rank_run(sh.DistRing(None), world, q, k, v, w, sink, causal, 0.0)
        dist.all_reduce(mine[4])                          # dsink: SUM over the ranks
        res.put((rank, [x.numpy() for x in mine]))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("causal", [False, True])
def test_ring_world2_gloo(causal):
    world = 2
    ctx = mp.get_context("spawn")
    res = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_gloo_worker, args=(r, world, port, causal, res)) for r in range(world)]
    for p in procs:
        p.start()
    got = dict(res.get(timeout=120) for _ in range(world))
    for p in procs:
        p.join(60)
    per_rank = [[torch.from_numpy(x) for x in got[r]] for r in range(world)]
    q, k, v, w = _problem(world, 3)
    sink = sr.sink_values(H, torch.float64)
    ref_out, ref_grads = _reference(q, k, v, w, sink, causal, 0.0)
    _check([p[:4] for p in per_rank], ref_out, ref_grads, causal, False)
    for p in per_rank:                                    # every rank holds the reduced dsink
        assert (p[4] - ref_grads[3]).abs().max().item() <= TOL


@pytest.mark.parametrize("world", [1, 2, 4])
@pytest.mark.parametrize("dim", [0, 1])
def test_zigzag_round_trip(world, dim):
    x = torch.arange(2 * world * 3 * 5).view(2 * world * 3, 5) if dim == 0 else \
        torch.arange(2 * 2 * world * 3).view(2, 2 * world * 3)
    shards = [sh.zigzag_split(x, world, r, dim) for r in range(world)]
    assert all(s.shape[dim] == 6 for s in shards)
    assert torch.equal(sh.zigzag_gather(shards, dim), x)
    c = 3                                                 # rank r: chunks r and 2W - 1 - r
    assert torch.equal(shards[0].narrow(dim, c, c), x.narrow(dim, (2 * world - 1) * c, c))
    with pytest.raises(ValueError, match="multiple of 2 \\* world"):
        sh.zigzag_split(torch.zeros(2, 2 * world + 1), world, 0)


class _FakeRing:
    def __init__(self, world):
        self.rank, self.world = 0, world


@pytest.mark.parametrize("kw,exc,needle", [
    (dict(window_size=(8, 0)), NotImplementedError, "sliding windows"),
    (dict(alibi_slopes=torch.zeros(H)), NotImplementedError, "ALiBi"),
    (dict(dropout_p=0.1), NotImplementedError, "dropout"),
    (dict(ring=_FakeRing(17)), NotImplementedError, "at most 16 ranks"),
    (dict(causal=True, odd=True), ValueError, "even s_local"),
    (dict(fp8=True), NotImplementedError, "fp8"),
    (dict(sink=torch.zeros(H + 1)), ValueError, "sink must have shape"),
])
def test_ring_refusals(kw, exc, needle):
    kw = dict(kw)
    s = 5 if kw.pop("odd", False) else 4
    q, k, v = torch.zeros(1, s, H, D), torch.zeros(1, s, HK, D), torch.zeros(1, s, HK, D)
    if kw.pop("fp8", False):
        q = q.to(torch.float8_e4m3fn)
    kw.setdefault("ring", _FakeRing(2))
    with pytest.raises(exc, match=needle):
        sh.ring_attention(q, k, v, ops=mr.OracleOps, **kw)


def test_docstrings_state_the_sum_all_reduce():
    for fn in (sh.ring_attention, sh.all_gather_dim, sh.sharded_attention, sh.sharded_varlen):
        assert "SUM all-reduce" in fn.__doc__, fn.__name__
