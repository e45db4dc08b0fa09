"""GPU: the backward of the attention-sink forward through the Python interface
(`flash_attn_func` / `flash_attn_varlen_func` with sink=): dq / dk / dv from the unchanged
backward kernels (given the sink forward's O and LSE they are the sink softmax's), dsink from
fmha_bwd_sink_kernel.

dq / dk / dv: `bwd_util.check_grads` (global and block rules) against the float64 gradients of
tests/sink_ref.py.  dsink, per head:
    |dsink - ref64| <= 3 |dsink_pt - ref64| + eps / 2 * sum_rows exp(s - LSE) sum_d |dO O| + 1e-5
The middle term is derived, not tuned: dsink = -sum exp(s - LSE) rowsum(dO * O) reads the O the
forward stored, each element of which is off by at most eps / 2 |O| from its rounding to the
dtype (the same rounding the backward's D carries)."""
import itertools

import pytest
import torch

from tests import bwd_util as bu
from tests import sink_ref as sr

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16


@pytest.fixture(scope="module")
def xfa():
    import xf_flash_attention_cutlass_amd as m
    return m


def _inputs(b, s, h, hk, d, seed):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(b, s, h, d, generator=g).to(BF)
    k = torch.randn(b, s, hk, d, generator=g).to(BF)
    v = torch.randn(b, s, hk, d, generator=g).to(BF)
    go = torch.randn(b, s, h, d, generator=g).to(BF)
    return q, k, v, go


DENSE = {"d64_causal": (64, dict(causal=True)), "d128_window100_0": (128, dict(window=(100, 0)))}


@pytest.mark.parametrize("deterministic", [False, True], ids=["atomic", "deterministic"])
@pytest.mark.parametrize("case", list(DENSE))
def test_dense_backward_with_sink(xfa, parity_report, case, deterministic):
    d, mask = DENSE[case]
    q, k, v, go = _inputs(2, 130, 4, 2, d, 71 + d)
    sink = sr.sink_values(4)
    fn = lambda a, b_, c, s, reorder_ops: sr.sink_attention(a, b_, c, s, reorder_ops=reorder_ops, **mask)
    refs, ds64, dspt, o64, l64 = sr.grad_refs(fn, q, k, v, go, sink)
    qd, kd, vd = (x.to(DEV).requires_grad_(True) for x in (q, k, v))
    sd = sink.to(DEV).requires_grad_(True)
    kw = dict(causal=mask.get("causal", False), window_size=mask.get("window", (-1, -1)))
    out = xfa.flash_attn_func(qd, kd, vd, deterministic=deterministic, sink=sd, **kw)
    dq, dk, dv, dsink = torch.autograd.grad(out, (qd, kd, vd, sd), go.to(DEV), retain_graph=True)
    (dsink2,) = torch.autograd.grad(out, (sd,), go.to(DEV))
    name = f"sink bwd {case} det={deterministic}"
    bu.check_grads(name, (dq, dk, dv), refs, BF, parity_report)
    term = sum(sr.dsink_term(sink, l64[i], go[i], o64[i]) for i in range(q.shape[0]))
    sr.check_dsink(name, dsink, ds64, dspt, term, parity_report)
    assert dsink.dtype == sink.dtype and torch.equal(dsink.view(torch.int32), dsink2.view(torch.int32))


@pytest.mark.parametrize("deterministic", [False, True], ids=["atomic", "deterministic"])
def test_varlen_backward_with_sink(xfa, parity_report, deterministic):
    lens = (1, 33, 130)
    q, k, v, go = (x[0] for x in _inputs(1, sum(lens), 4, 2, 128, 75))
    sink = sr.sink_values(4)
    fn = lambda a, b_, c, s, reorder_ops: sr.sink_attention_varlen(a, b_, c, s, lens, lens, causal=True,
                                                                   reorder_ops=reorder_ops)
    refs, ds64, dspt, o64, l64 = sr.grad_refs(fn, q, k, v, go, sink)
    cu = torch.tensor([0] + list(itertools.accumulate(lens)), dtype=torch.int32, device=DEV)
    qd, kd, vd = (x.to(DEV).requires_grad_(True) for x in (q, k, v))
    sd = sink.to(DEV).requires_grad_(True)
    out = xfa.flash_attn_varlen_func(qd, kd, vd, cu, cu, max(lens), max(lens), causal=True,
                                     deterministic=deterministic, sink=sd)
    dq, dk, dv, dsink = torch.autograd.grad(out, (qd, kd, vd, sd), go.to(DEV), retain_graph=True)
    (dsink2,) = torch.autograd.grad(out, (sd,), go.to(DEV))
    name = f"sink bwd varlen d128 causal det={deterministic}"
    worst = bu.WorstRows()
    for sl in bu.seq_slices(cu.cpu()):
        seq = bu.Refs(*(tuple(x[sl][None] for x in r) for r in refs))
        bu.check_grads(name, tuple(x[sl][None] for x in (dq, dk, dv)), seq, BF, worst)
    worst.flush(parity_report)
    sr.check_dsink(name, dsink, ds64, dspt, sr.dsink_term(sink, l64, go, o64), parity_report)
    assert torch.equal(dsink.view(torch.int32), dsink2.view(torch.int32))


def test_minus_inf_sink_backward_is_the_sink_free_backward(xfa):
    """sink = -inf on every head: dq / dk / dv bit-identical to the sink-free backward and
    dsink = 0.  In the deterministic mode: the default mode adds dQ with float atomics, whose
    order (and so whose bits) differs between any two runs, with or without a sink."""
    q, k, v, go = _inputs(2, 130, 4, 2, 64, 77)
    sink = torch.full((4,), float("-inf"), device=DEV, requires_grad=True)
    res = []
    for s in (None, sink):
        qd, kd, vd = (x.to(DEV).requires_grad_(True) for x in (q, k, v))
        out = xfa.flash_attn_func(qd, kd, vd, causal=True, deterministic=True, sink=s)
        res.append((out,) + torch.autograd.grad(out, (qd, kd, vd) + ((s,) if s is not None else ()),
                                                go.to(DEV)))
    for a, b_ in zip(res[0], res[1][:4]):
        assert torch.equal(a.view(torch.int16), b_.view(torch.int16))
    assert torch.equal(res[1][4], torch.zeros(4, device=DEV))


def test_sink_dtype_round_trip(xfa):
    """A bf16 sink is cast to fp32 for the call and its gradient comes back in bf16."""
    q, k, v, go = _inputs(1, 64, 4, 2, 64, 78)
    qd, kd, vd = (x.to(DEV) for x in (q, k, v))
    sd = torch.linspace(-1, 1, 4).to(BF).to(DEV).requires_grad_(True)
    out = xfa.flash_attn_func(qd, kd, vd, causal=True, sink=sd)
    (dsink,) = torch.autograd.grad(out, (sd,), go.to(DEV))
    assert dsink.dtype == BF and dsink.shape == (4,) and bool(torch.isfinite(dsink.float()).all())
