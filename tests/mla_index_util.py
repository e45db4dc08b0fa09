"""Shared helpers of the MLA indexer tests (not a conftest: imported explicitly).

The index-key cache (include/paged_attn.h, 2.14): blocks of page * 132 bytes - page rows of 128
e4m3fn features, then page fp32 descales.  `quantize_ref` restates the append's quantiser (both
scale formats), `block_views` the layout, `logits_ref` the logits in float64 from the cache bytes,
with the magnitude sum A the error bound is stated in.
"""
from __future__ import annotations

import torch

F8 = torch.float8_e4m3fn
NEG_INF = float("-inf")


def quantize_ref(k, scale_fmt=None):
    """k [n, 128] (bf16 / fp16) -> (bytes uint8 [n, 128], descale fp32 [n]): amax = max |float(x)|,
    descale = amax / 448 in fp32 (1.0 where amax == 0) and, under "ue8m0", the smallest power of two
    >= that, at least 2^-126, on the exponent bits; byte = e4m3fn(clamp(float(x) * (1 / descale)))."""
    x = k.float()
    amax = x.abs().amax(-1)
    ds = torch.where(amax == 0, torch.ones_like(amax), amax / 448.0)
    if scale_fmt == "ue8m0":
        bits = ds.view(torch.int32)
        ds = (((bits >> 23) + ((bits & 0x7FFFFF) != 0).int()).clamp(min=1) << 23).view(torch.float32)
    else:
        assert scale_fmt is None
    return (x * (1 / ds)[:, None]).clamp(-448.0, 448.0).to(F8).view(torch.uint8), ds


def block_views(cache, page):
    """cache uint8 [num_blocks, page * 132] -> views (keys uint8 [num_blocks, page, 128], descales
    fp32 [num_blocks, page]) of the same storage."""
    return cache[:, :page * 128].unflatten(1, (page, 128)), cache[:, page * 128:].view(torch.float32)


def write_slots(cache, page, slots, b8, ds):
    """What the append writes: row slots[t] = (b8[t], ds[t]) for the slots inside the cache."""
    keys, dsv = block_views(cache, page)
    for t, s in enumerate(slots.tolist()):
        if 0 <= s < cache.shape[0] * page:
            keys[s // page, s % page] = b8[t]
            dsv[s // page, s % page] = ds[t]


def logits_ref(q8, weights, cache, page, table, lens, max_k):
    """float64 (logits, A) [b * sq, max_k] from the bytes: logits as the header defines them (-inf
    from vis on), A = descale * sum_h |w| sum_d |q k| (0 where the logit is -inf)."""
    b, sq, heads, _ = q8.shape
    keys, dsv = block_views(cache, page)
    out = torch.full((b * sq, max_k), NEG_INF, dtype=torch.float64)
    mag = torch.zeros(b * sq, max_k, dtype=torch.float64)
    for bi in range(b):
        n = min(int(lens[bi]), max_k)
        s = torch.arange(n)
        blk = table[bi, s // page].long()
        ok = (blk >= 0) & (blk < cache.shape[0])
        blk = torch.where(ok, blk, torch.zeros_like(blk))
        k = keys[blk, s % page].view(F8).double()
        d = dsv[blk, s % page].double()
        for i in range(sq):
            r = bi * sq + i
            vis = ok & (s < max(0, min(n - sq + i + 1, n)))
            q, w = q8[bi, i].view(F8).double(), weights[r].double()
            out[r, :n] = torch.where(vis, d * (w[:, None] * (q @ k.T).clamp(min=0)).sum(0), out[r, :n])
            mag[r, :n] = torch.where(vis, d * (w.abs()[:, None] * (q.abs() @ k.abs().T)).sum(0), mag[r, :n])
    return out, mag
