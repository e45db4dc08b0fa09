"""Shared helpers of the merge and ring-attention tests (not a conftest: imported explicitly).

* `merge_ref`: the merge of partial attention states in the dtype of its inputs;
  float64 inputs give the reference.  Includes the absent-part (LSE = +-inf) and all-absent rules.
* `bwd_from_lse`: the `bwd` contract restated: dq / dk / dv / D of one (queries, K/V chunk) pair
  from a GIVEN out and lse (the merged ones), in the dtype of its inputs.
* `OracleOps`: the `ops` of `sharding.ring_attention` on those restatements (CPU, any dtype).
* `ThreadRing` / `run_ranks`: an in-process ring, one thread per rank joined by queues, so one
  process plays all `world` ranks.
"""
from __future__ import annotations

import math
import queue
import threading

import torch

from oracle import attention_ref as orc

INF = float("inf")


def merge_ref(outs, lses, sink=None):
    """outs: n tensors [b, rows, h, d] (or packed [total, h, d]); lses: n tensors [b, h, rows]
    (or [h, total]); sink [h] or None.  Returns (out, lse).  A part with LSE = +inf or -inf is
    absent for that row (its O is selected away, never multiplied); no part present: O = 0,
    LSE = +inf whatever the sink."""
    packed = outs[0].dim() == 3
    if packed:
        outs, lses = [o[None] for o in outs], [l[None] for l in lses]
    dt = torch.promote_types(outs[0].dtype, lses[0].dtype)
    O = torch.stack([o.to(dt) for o in outs])                        # [n, b, rows, h, d]
    L = torch.stack([l.to(dt) for l in lses])                        # [n, b, h, rows]
    present = ~torch.isinf(L)
    anyp = present.any(0)
    m = torch.where(present, L, torch.full_like(L, -INF)).max(0).values
    m = torch.where(anyp, m, torch.zeros_like(m))
    w = torch.where(present, torch.exp(torch.where(present, L, m.expand_as(L)) - m), torch.zeros_like(L))
    den = torch.where(anyp, w.sum(0), torch.ones_like(m))
    wn = (w / den).permute(0, 1, 3, 2).unsqueeze(-1)                 # [n, b, rows, h, 1]
    sel = present.permute(0, 1, 3, 2).unsqueeze(-1)
    out = (wn * torch.where(sel, O, torch.zeros_like(O))).sum(0)
    lse = m + torch.log(den)
    if sink is not None:
        s = sink.to(dt).view(1, -1, 1)
        f = 1.0 / (1.0 + torch.exp(s - lse))
        delta = (lse - s).abs()
        lse = torch.maximum(lse, s.expand_as(lse)) + torch.log1p(torch.exp(-delta))
        out = out * f.permute(0, 2, 1).unsqueeze(-1)
    lse = torch.where(anyp, lse, torch.full_like(lse, INF))
    out = torch.where(anyp.permute(0, 2, 1).unsqueeze(-1), out, torch.zeros_like(out))
    out = out.to(outs[0].dtype)
    return (out[0], lse[0]) if packed else (out, lse)


def _masked_scores(q, k, scale, causal, softcap):
    """(capped, masked scores [b, h, sq, sk], visibility mask, raw scaled scores)"""
    kk = orc.expand_kv(k, q.shape[2])
    raw = torch.einsum("bthd,bshd->bhts", q, kk) * scale
    s = torch.tanh(raw / softcap) * softcap if softcap > 0 else raw
    vis = torch.ones(q.shape[1], k.shape[1], dtype=torch.bool)
    if causal:
        vis = ~orc.local_mask(q.shape[1], k.shape[1], (-1, 0))
    return s, vis, raw


def fwd_chunk(q, k, v, scale, causal=False, softcap=0.0):
    """(out, lse) of q against one K/V chunk; a row without a visible key has O = 0, LSE = +inf."""
    s, vis, _ = _masked_scores(q, k, scale, causal, softcap)
    s = s.masked_fill(~vis, -INF)
    lse = torch.logsumexp(s, dim=-1)
    dead = torch.isneginf(lse)
    lse = torch.where(dead, torch.full_like(lse, INF), lse)
    p = torch.exp(s - torch.where(dead, torch.zeros_like(lse), lse).unsqueeze(-1))
    p = p.masked_fill(dead.unsqueeze(-1), 0.0)
    return torch.einsum("bhts,bshd->bthd", p, orc.expand_kv(v, q.shape[2])), lse


def bwd_from_lse(dout, q, k, v, out, lse, scale, causal=False, softcap=0.0):
    """The `bwd` contract on one K/V chunk with a GIVEN out / lse: P = exp(S - lse), D =
    rowsum(dO * O), dV = P^T dO, dS = P (dO V^T - D) (times the softcap derivative), dQ = scale
    dS K, dK = scale dS^T Q, the GQA group summed.  With the merged out / lse of the whole key
    set this is the chunk's exact dK / dV and its additive share of dQ.  Returns (dq, dk, dv, D
    [b, h, sq])."""
    b, sq, h, d = q.shape
    sk, hk = k.shape[1], k.shape[2]
    s, vis, raw = _masked_scores(q, k, scale, causal, softcap)
    p = torch.exp(s - lse.unsqueeze(-1)).masked_fill(~vis, 0.0)     # lse = +inf: exp(-inf) = 0
    dsum = (dout * out).sum(-1).permute(0, 2, 1)
    kk, vv = orc.expand_kv(k, h), orc.expand_kv(v, h)
    dv = torch.einsum("bhts,bthd->bshd", p, dout)
    ds = p * (torch.einsum("bthd,bshd->bhts", dout, vv) - dsum.unsqueeze(-1))
    if softcap > 0:
        ds = ds * (1.0 - torch.tanh(raw / softcap) ** 2)
    dq = torch.einsum("bhts,bshd->bthd", ds, kk) * scale
    dk = torch.einsum("bhts,bthd->bshd", ds, q) * scale
    g = h // hk
    return dq, dk.view(b, sk, hk, g, d).sum(3), dv.view(b, sk, hk, g, d).sum(3), dsum


class OracleOps:
    """`ops` of `sharding.ring_attention` on the restatements above (see `sharding.KernelOps` for
    the contract)."""

    @staticmethod
    def fwd(q, k, v, scale, causal, softcap, out=None):
        o, lse = fwd_chunk(q, k, v, scale, causal, softcap)
        if out is not None:
            out.copy_(o)
            o = out
        return o, lse

    @staticmethod
    def bwd(dout, q, k, v, out, lse, scale, causal, softcap, deterministic):
        return bwd_from_lse(dout, q, k, v, out, lse, scale, causal, softcap)

    @staticmethod
    def merge(outs, lses, sink, out, lse_out):
        o, lse = merge_ref(list(outs), list(lses), sink)
        if out is None:
            return o, lse
        out.copy_(o)
        lse_out.copy_(lse)
        return out, lse_out

    @staticmethod
    def sink_bwd(lse, softmax_d, sink):
        w = torch.exp(sink.view(1, -1, 1) - lse)                    # exp(-inf) = 0 on dead rows
        return -(w * softmax_d).sum((0, 2))


def default_scale(q):
    return 1.0 / math.sqrt(q.shape[-1])


class ThreadRing:
    """The `ring` of `sharding.ring_attention` inside one process: rank r puts what it sends into
    rank r + 1's queue and takes what rank r - 1 sent from its own.  Each queue has one producer,
    so messages arrive in the order they were sent."""

    def __init__(self, rank, world, boxes):
        self.rank, self.world, self.boxes = rank, world, boxes

    def shift(self, tensors):
        self.boxes[(self.rank + 1) % self.world].put(list(tensors))
        return self.boxes[self.rank].get(timeout=120)


def run_ranks(world, fn):
    """fn(ring) on `world` threads, one per rank; returns the results by rank (re-raises the
    first failure)."""
    boxes = [queue.Queue() for _ in range(world)]
    res, err = [None] * world, [None] * world

    def body(r):
        try:
            res[r] = fn(ThreadRing(r, world, boxes))
        except BaseException as e:          # noqa: BLE001 (handed to the caller's thread)
            err[r] = e
            for bx in boxes:                # unblock the neighbours: they fail on the marker
                bx.put(None)
    ths = [threading.Thread(target=body, args=(r,)) for r in range(world)]
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    for e in err:
        if e is not None and not isinstance(e, TypeError):
            raise e
    for e in err:
        if e is not None:
            raise e
    return res
