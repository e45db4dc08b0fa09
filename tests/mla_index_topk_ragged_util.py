"""Shared helper of the ragged MLA index top-k tests (not a conftest: imported explicitly): the exact
reference of fmha_mla_index_topk_ragged (include/paged_attn.h, 2.17) on the CPU.
"""
from __future__ import annotations

import torch


def topk_ragged_ref(logits, ks, ke, topk, slots=None):
    """int32 [rows, topk]: per row the selectable columns (not NaN, not -inf) of [lo, hi), -0.0 as
    +0.0, stably sorted descending (the lower column first among equals), the first topk of them in
    ascending column order, through `slots` (-1 in place where the entry is outside [0, 2^31)), then -1."""
    rows, n = logits.shape
    out = torch.full((rows, topk), -1, dtype=torch.int32)
    for r in range(rows):
        lo, hi = max(0, min(int(ks[r]), n)), max(0, min(int(ke[r]), n))
        x = logits[r, lo:max(lo, hi)].float()
        pos = (~x.isnan() & (x != float("-inf"))).nonzero()[:, 0]
        order = torch.sort(x[pos] + 0.0, descending=True, stable=True).indices
        sel = pos[order[:topk]].sort().values + lo
        ent = sel if slots is None else slots[sel]
        out[r, :len(sel)] = torch.where((ent >= 0) & (ent < 2 ** 31), ent, torch.full_like(ent, -1)).int()
    return out
