"""Shared helpers of the attention-sink tests (not a conftest: imported explicitly).

The reference is the explicit form: the scores from the oracle's own pieces
(`orc.local_mask`, `orc.expand_kv`), one extra column that holds `sink[h]`, a softmax over
keys + column, the column dropped, then times V.  It computes in the dtype of its inputs: float64
inputs give the reference, bf16 / fp16 inputs (with `reorder_ops`) the low-precision estimate of
the project's pass rules.  Autograd through it gives the reference gradients.

* `sink_attention`: [b, s, h, d] inputs -> (out, lse [b, h, sq]).
* `sink_attention_varlen`: packed inputs, per sequence.
* `posthoc`: the same result from a sink-free (O0, L0): O = f O0, LSE = max + log1p(exp(-|.|)).
* `dsink_formula`: -sum exp(s - LSE) D.
* `sink_values`: per-head values that differ, with one head at +20 and one at -inf.
* `fwd_refs` / `check_fwd`: float64 reference, low-precision estimate and the forward rules.
* `grad_refs`, `dsink_term`, `check_dsink`: the reference gradients and the dsink rule of
  tests/test_sink_bwd_gpu.py (shared with tests/test_bwd_stress_gpu.py).
"""
from __future__ import annotations

import math
from collections import namedtuple

import torch

from oracle import attention_ref as orc

EPS = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
LSE_ATOL = 1e-3
INF = float("inf")


def sink_values(h, dtype=torch.float32):
    """linspace(-3, 3) over the heads, head 1 at +20 and head h - 2 at -inf: a GQA head mix-up
    changes the result."""
    s = torch.linspace(-3.0, 3.0, h)
    if h >= 4:
        s[1] = 20.0
        s[h - 2] = -INF
    return s.to(dtype)


def sink_attention(q, k, v, sink, causal=False, window=(-1, -1), softcap=0.0, reorder_ops=False):
    """q [b, sq, h, d], k / v [b, sk, hk, d], sink [h] (or None: no sink column) in one dtype.
    Returns (out [b, sq, h, d], lse [b, h, sq]); a row without a visible key has O = 0 and
    LSE = +inf (the library's convention), whatever its sink."""
    window = (int(window[0]), 0) if causal else (int(window[0]), int(window[1]))
    b, sq, h, d = q.shape
    sk = k.shape[1]
    if sk == 0:
        return torch.zeros_like(q), torch.full((b, h, sq), INF, dtype=q.dtype)
    k, v = orc.expand_kv(k, h), orc.expand_kv(v, h)
    if reorder_ops:
        s = torch.einsum("bthd,bshd->bhts", q, k / math.sqrt(d))
    else:
        s = torch.einsum("bthd,bshd->bhts", q / math.sqrt(d), k)
    if softcap > 0:
        s = torch.tanh(s / softcap) * softcap
    dead = None
    if window[0] >= 0 or window[1] >= 0:
        lm = orc.local_mask(sq, sk, window, device=q.device)
        s = s.masked_fill(lm, -INF)
        dead = lm.all(-1).view(1, 1, sq)
    ext = s
    if sink is not None:
        ext = torch.cat([s, sink.to(s.dtype).view(1, h, 1, 1).expand(b, h, sq, 1)], dim=-1)
    p = torch.softmax(ext, dim=-1)[..., :sk].to(v.dtype)
    lse = torch.logsumexp(ext, dim=-1)
    if dead is not None:
        p = p.masked_fill(dead.unsqueeze(-1), 0.0)
        lse = torch.where(dead, torch.full_like(lse, INF), lse)
    return torch.einsum("bhts,bshd->bthd", p, v), lse


def seq_slices(lens):
    cu = [0]
    for n in lens:
        cu.append(cu[-1] + n)
    return [slice(cu[i], cu[i + 1]) for i in range(len(lens))]


def sink_attention_varlen(q, k, v, sink, lens_q, lens_k, used_k=None, **kw):
    """Packed q [total_q, h, d], k / v [total_k, hk, d]; sequence i has lens_q[i] queries and the
    first used_k[i] (default lens_k[i]) keys of its lens_k[i]-row slot.  Returns (out
    [total_q, h, d], lse [h, total_q])."""
    used_k = lens_k if used_k is None else used_k
    outs, lses = [], []
    for sq_, sk_, n in zip(seq_slices(lens_q), seq_slices(lens_k), used_k):
        ks, vs = k[sk_][:n], v[sk_][:n]
        o, l = sink_attention(q[sq_][None], ks[None], vs[None], sink, **kw)
        outs.append(o[0])
        lses.append(l[0])
    return torch.cat(outs, 0), torch.cat(lses, 1)


def posthoc(o0, l0, sink):
    """(O, LSE) from the sink-free (o0 [b, sq, h, d], l0 [b, h, sq]): f = 1 / (1 + exp(s - L0)),
    O = f O0, LSE = max(L0, s) + log1p(exp(-|L0 - s|)); rows with L0 = +inf stay."""
    s = sink.to(l0.dtype).view(1, -1, 1)
    dead = torch.isinf(l0) & (l0 > 0)
    l0s = torch.where(dead, torch.zeros_like(l0), l0)
    f = 1.0 / (1.0 + torch.exp(s - l0s))
    delta = (l0s - s).abs()
    delta = torch.where(torch.isnan(delta), torch.zeros_like(delta), delta)
    lse = torch.maximum(l0s, s.expand_as(l0s)) + torch.log1p(torch.exp(-delta))
    f = torch.where(dead, torch.ones_like(f), f)
    lse = torch.where(dead, l0, lse)
    return o0 * f.permute(0, 2, 1).unsqueeze(-1), lse


def dsink_formula(sink, lse, dout, out):
    """dsink[h] = - sum_(b, row) exp(s_h - LSE) D, D = rowsum(dO * O); lse [b, h, sq], dout / out
    [b, sq, h, d].  Rows with LSE = +inf add 0."""
    dsum = (dout * out).sum(-1).permute(0, 2, 1)                   # [b, h, sq]
    w = torch.exp(sink.to(lse.dtype).view(1, -1, 1) - lse)         # exp(-inf) = 0 on dead rows
    return -(w * dsum).sum((0, 2))


FwdRefs = namedtuple("FwdRefs", "ref64 lse64 pt")


def fwd_refs(q, k, v, sink, **kw) -> FwdRefs:
    """float64 (out, lse) and the low-precision estimate (q's dtype, reordered scale) of a dense
    problem; sink fp32 [h]."""
    o64, l64 = sink_attention(q.double(), k.double(), v.double(), sink.double(), **kw)
    pt, _ = sink_attention(q, k, v, sink.to(q.dtype), reorder_ops=True, **kw)
    return FwdRefs(o64, l64, pt)


def fwd_refs_varlen(q, k, v, sink, lens_q, lens_k, used_k=None, **kw) -> FwdRefs:
    o64, l64 = sink_attention_varlen(q.double(), k.double(), v.double(), sink.double(), lens_q,
                                     lens_k, used_k, **kw)
    pt, _ = sink_attention_varlen(q, k, v, sink.to(q.dtype), lens_q, lens_k, used_k,
                                  reorder_ops=True, **kw)
    return FwdRefs(o64, l64, pt)


def check_fwd(name, o, lse, refs: FwdRefs, dtype, report=None, mult=2.0, atol=0.0, second_rounding=False):
    """The project's forward rules against the float64 reference: max|O - ref| <= mult *
    max|pt - ref| + atol (mult 2 forward / varlen; 3 and atol 1e-5 kvcache); the LSE's +inf
    pattern equal to the reference's and its finite values within 1e-3.  second_rounding (the
    post-pass launches, which round O to the dtype a second time): + eps / 2 * max|ref|, the most
    a second rounding to nearest adds."""
    o, lse = o.double().cpu(), lse.double().cpu()
    assert torch.isfinite(o).all(), f"{name}: O has non-finite values"
    assert not torch.isnan(lse).any(), f"{name}: LSE has NaN"
    err = (o - refs.ref64).abs().max().item()
    bound = mult * (refs.pt.double() - refs.ref64).abs().max().item() + atol
    if second_rounding:
        bound += 0.5 * EPS[dtype] * refs.ref64.abs().max().item()
    fin = torch.isfinite(refs.lse64)
    inf_ok = bool(torch.equal(torch.isinf(lse) & (lse > 0), ~fin))
    dl = (lse[fin] - refs.lse64[fin]).abs()
    lse_err = dl.max().item() if dl.numel() else 0.0
    print(f"{name}: o err {err:.3e} bound {bound:.3e}; lse err {lse_err:.3e} bound {LSE_ATOL:.0e}")
    if report is not None:
        report(dict(case=name, metric="o", err=err, bound=bound))
        report(dict(case=name, metric="lse", err=lse_err, bound=LSE_ATOL))
    assert err <= bound, f"{name}: max|O - ref| = {err:.3e} > {bound:.3e}"
    assert inf_ok, f"{name}: the LSE's +inf rows differ from the reference's"
    assert lse_err <= LSE_ATOL, f"{name}: LSE off by {lse_err:.3e}"


# ---------------------------------------------------------------- backward ---------------
def _ref_grads(fn, q, k, v, go, sink, cast, reorder):
    """Gradients (dq, dk, dv, dsink) and (out, lse) of `fn` (a sink_ref forward) over inputs cast
    by `cast`."""
    qq, kk, vv, ss = (cast(x).clone().requires_grad_(True) for x in (q, k, v, sink))
    out, lse = fn(qq, kk, vv, ss, reorder_ops=reorder)
    grads = torch.autograd.grad(out, (qq, kk, vv, ss), cast(go))
    return grads, out.detach(), lse.detach()


def grad_refs(fn, q, k, v, go, sink, dtype=torch.bfloat16):
    """(bwd_util.Refs of (dq, dk, dv), dsink ref64, dsink pt, out64, lse64) of `fn`, a sink_ref
    forward taking (q, k, v, sink, reorder_ops=)."""
    from tests.bwd_util import Refs
    g64, o64, l64 = _ref_grads(fn, q, k, v, go, sink, lambda x: x.double(), False)
    g32, _, _ = _ref_grads(fn, q, k, v, go, sink, lambda x: x.float(), False)
    gpt, _, _ = _ref_grads(fn, q, k, v, go, sink, lambda x: x.to(dtype), True)
    refs = Refs(g64[:3], tuple(x.to(dtype) for x in g32[:3]), gpt[:3])
    return refs, g64[3], gpt[3].double(), o64, l64


def dsink_term(sink, lse64, go, o64, dtype=torch.bfloat16):
    """eps / 2 * sum_rows exp(s - LSE) sum_d |dO O| per head; lse64 [h, rows], go / o64
    [rows, h, d]."""
    w = torch.exp(sink.double().view(-1, 1) - lse64)               # [h, rows]
    a = (go.double() * o64).abs().sum(-1)                          # [rows, h]
    return 0.5 * EPS[dtype] * (w * a.transpose(0, 1)).sum(1)


def check_dsink(name, dsink, ref64, pt, term, report):
    dsink = dsink.double().cpu()
    assert torch.isfinite(dsink).all(), f"{name}: dsink not finite"
    err = (dsink - ref64).abs()
    bound = 3.0 * (pt - ref64).abs() + term + 1e-5
    ratio = err / bound
    print(f"{name}: dsink {dsink.tolist()} ref {ref64.tolist()} ratios {[round(x, 3) for x in ratio.tolist()]}")
    i = int(ratio.argmax())
    report(dict(case=name, metric="dsink", err=err[i].item(), bound=bound[i].item(), head=i))
    assert bool((ratio <= 1.0).all()), f"{name}: dsink err {err.tolist()} > bound {bound.tolist()}"
