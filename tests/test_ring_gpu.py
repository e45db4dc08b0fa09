"""GPU: ring (context-parallel) attention on the real kernels.  One process plays all W ranks:
one thread per rank joined by queues (`merge_ref.ThreadRing`), every rank running
`sharding.ring_forward` / `ring_backward` with the default `KernelOps` on the one GPU.  (The
autograd Function's forward runs in the rank threads too; its backward is driven here by calling
`ring_backward` directly, because autograd runs the backward of CUDA tensors on one engine thread
per device, where W ranks that wait for each other cannot make progress.  The Function's backward
wiring is covered on CPU, tests/test_ring_cpu.py.)

Forward: `sink_ref.check_fwd` with second_rounding=True (the per-step partials are rounded to the
dtype, then the merge rounds once more) against the float64 oracle on the gathered problem.
Gradients: `bwd_util.check_grads` unchanged (mult 3, no block factor); dsink (the sum of the
ranks' shares) by the rule of tests/test_sink_bwd_gpu.py.  W = 1 through a one-rank RCCL group is
`flash_attn_func` itself, bit for bit."""
import os

import pytest
import torch

from tests import bwd_util as bu
from tests import merge_ref as mr
from tests import sink_ref as sr
from tests.test_sharding import _free_port

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, FP = torch.bfloat16, torch.float16
B, H, HK = 2, 4, 2


@pytest.fixture(scope="module")
def sh():
    from xf_flash_attention_cutlass_amd import sharding
    return sharding


def _inputs(s, d, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, s, H, d, generator=g).to(dtype)
    k = torch.randn(B, s, HK, d, generator=g).to(dtype)
    v = torch.randn(B, s, HK, d, generator=g).to(dtype)
    go = torch.randn(B, s, H, d, generator=g).to(dtype)
    return q, k, v, go


def _ref(q, k, v, go, sink, cast, reorder, **kw):
    leaves = [cast(x).clone().requires_grad_(True) for x in (q, k, v)]
    if sink is not None:
        leaves.append(cast(sink).clone().requires_grad_(True))
    out, lse = sr.sink_attention(leaves[0], leaves[1], leaves[2], leaves[3] if sink is not None else None,
                                 reorder_ops=reorder, **kw)
    return torch.autograd.grad(out, leaves, cast(go)), out.detach(), lse.detach()


def _all_refs(q, k, v, go, sink, dtype, **kw):
    g64, o64, l64 = _ref(q, k, v, go, sink, lambda x: x.double(), False, **kw)
    g32, _, _ = _ref(q, k, v, go, sink, lambda x: x.float(), False, **kw)
    gpt, opt, _ = _ref(q, k, v, go, sink, lambda x: x.to(dtype), True, **kw)
    grads = bu.Refs(g64[:3], tuple(x.to(dtype) for x in g32[:3]), gpt[:3])
    return sr.FwdRefs(o64, l64, opt), grads, g64, gpt


def _split(sh, x, world, rank, causal):
    if causal:
        return sh.zigzag_split(x, world, rank)
    n = x.shape[1] // world
    return x[:, rank * n:(rank + 1) * n]


def _run_ring(sh, world, q, k, v, go, sink, causal, softcap, deterministic):
    """Every rank's (out, lse, dq, dk, dv, dsink) on the CPU, gathered to the whole problem."""
    scale = q.shape[-1] ** -0.5
    s32 = None if sink is None else sink.to(DEV)

    def body(ring):
        ql, kl, vl, gl = (_split(sh, x, world, ring.rank, causal).contiguous().to(DEV) for x in (q, k, v, go))
        kw = dict(causal=causal, softmax_scale=scale, softcap=softcap, sink=s32, ops=sh.KernelOps, ring=ring)
        out, lse = sh.ring_forward(ql, kl, vl, **kw)
        out_f = sh.ring_attention(ql, kl, vl, causal=causal, softcap=softcap, sink=s32, ring=ring)
        grads = sh.ring_backward(gl, ql, kl, vl, out, lse, deterministic=deterministic, **kw)
        torch.cuda.synchronize()
        assert torch.equal(out_f.view(torch.int16), out.view(torch.int16)), "Function forward != ring_forward"
        return [x.cpu() for x in (out, lse, *grads[:3])] + [None if grads[3] is None else grads[3].cpu()]
    per_rank = mr.run_ranks(world, body)
    gather = (lambda xs, dim=1: sh.zigzag_gather(xs, dim)) if causal else (lambda xs, dim=1: torch.cat(xs, dim))
    out, dq, dk, dv = (gather([p[i] for p in per_rank]) for i in (0, 2, 3, 4))
    lse = gather([p[1] for p in per_rank], 2)
    dsink = None if sink is None else sum(p[5] for p in per_rank)
    return out, lse, (dq, dk, dv), dsink


CASES = {}
for _w in (2, 4):
    for _c in (1, 48):
        for _causal in (False, True):
            CASES[f"w{_w}_c{_c}_{'causal' if _causal else 'full'}"] = dict(
                world=_w, c=_c, causal=_causal, d=64 if (_w == 2) == (_c == 1) else 128)
CASES["fp16_w2_c48_causal"] = dict(world=2, c=48, causal=True, d=128, dtype=FP)
CASES["softcap_w4_c48_causal"] = dict(world=4, c=48, causal=True, d=64, softcap=15.0)
CASES["sink_w4_c48_causal"] = dict(world=4, c=48, causal=True, d=128, sink=True)
CASES["sink_w2_c48_full"] = dict(world=2, c=48, causal=False, d=64, sink=True)


@pytest.mark.parametrize("case", list(CASES))
def test_ring_matches_oracle(sh, parity_report, case):
    cfg = dict(dtype=BF, softcap=0.0, sink=False)
    cfg.update(CASES[case])
    world, c, causal, d, dtype = cfg["world"], cfg["c"], cfg["causal"], cfg["d"], cfg["dtype"]
    q, k, v, go = _inputs(2 * world * c, d, dtype, 300 + d + world + c)
    sink = sr.sink_values(H) if cfg["sink"] else None
    frefs, grefs, g64, gpt = _all_refs(q, k, v, go, sink, dtype, causal=causal, softcap=cfg["softcap"])
    out, lse, grads, dsink = _run_ring(sh, world, q, k, v, go, sink, causal, cfg["softcap"], False)
    name = f"ring {case}"
    sr.check_fwd(name, out, lse, frefs, dtype, parity_report, second_rounding=True)
    bu.check_grads(name, grads, grefs, dtype, parity_report)
    if sink is not None:
        # the rule of tests/test_sink_bwd_gpu.py: 3 |pt - ref| + eps / 2 sum exp(s - LSE) sum |dO O| + 1e-5
        w = torch.exp(sink.double().view(1, -1, 1) - frefs.lse64)
        a = (go.double() * frefs.ref64).abs().sum(-1).permute(0, 2, 1)
        term = 0.5 * bu.EPS[dtype] * (w * a).sum((0, 2))
        err = (dsink.double() - g64[3]).abs()
        bound = 3.0 * (gpt[3].double() - g64[3]).abs() + term + 1e-5
        i = int((err / bound).argmax())
        parity_report(dict(case=name, metric="dsink", err=err[i].item(), bound=bound[i].item(), head=i))
        assert bool((err <= bound).all()), f"{name}: dsink err {err.tolist()} > bound {bound.tolist()}"


def test_ring_deterministic_twice_same_bits(sh):
    q, k, v, go = _inputs(2 * 2 * 48, 128, BF, 41)
    a = _run_ring(sh, 2, q, k, v, go, None, True, 0.0, True)
    b = _run_ring(sh, 2, q, k, v, go, None, True, 0.0, True)
    assert torch.equal(a[0].view(torch.int16), b[0].view(torch.int16))
    assert torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
    for x, y, nm in zip(a[2], b[2], bu.NAMES):
        assert torch.equal(x.view(torch.int16), y.view(torch.int16)), nm


@pytest.fixture(scope="module")
def pg():
    import torch.distributed as dist
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ["MASTER_PORT"] = str(_free_port())
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device(DEV, 0))
    yield dist
    dist.destroy_process_group()


@pytest.mark.parametrize("with_sink", [False, True])
def test_world1_is_flash_attn_func(sh, pg, with_sink):
    """A one-rank RCCL group: no merge, no ring - `flash_attn_func` itself, forward and (with the
    deterministic backward, whose bits do not depend on atomics' order) backward bit for bit."""
    import xf_flash_attention_cutlass_amd as xfa
    q, k, v, go = (x.to(DEV) for x in _inputs(96, 128, BF, 43))
    res = []
    for fn in (lambda a, b_, c, s: sh.ring_attention(a, b_, c, causal=True, deterministic=True, sink=s),
               lambda a, b_, c, s: xfa.flash_attn_func(a, b_, c, causal=True, deterministic=True, sink=s)):
        leaves = [x.clone().requires_grad_(True) for x in (q, k, v)]
        s = sr.sink_values(H).to(DEV).requires_grad_(True) if with_sink else None
        out = fn(*leaves, s)
        grads = torch.autograd.grad(out, leaves + ([s] if with_sink else []), go)
        res.append((out.detach(), *grads))
    for x, y in zip(*res):
        assert x.dtype == y.dtype and torch.equal(x.view(torch.int32 if x.dtype == torch.float32 else torch.int16),
                                                  y.view(torch.int32 if y.dtype == torch.float32 else torch.int16))
