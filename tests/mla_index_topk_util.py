"""Shared helper of the MLA index top-k tests (not a conftest: imported explicitly): the exact
reference of fmha_mla_index_topk (include/paged_attn.h, 2.15) on the CPU.
"""
from __future__ import annotations

import torch

INT32_MAX = 2 ** 31 - 1


def topk_ref(logits, table, lens, topk, seqlen_q, page, num_blocks, max_k=None):
    """int32 [rows, topk]: per row the selectable columns (not NaN, not -inf) of [0, vis), -0.0 as
    +0.0, stably sorted descending (the lower position first among equals), the first topk of them
    in ascending position, through the block table (-1 in place where the entry is outside [0,
    num_blocks) or the slot beyond int32), then -1."""
    rows, width = logits.shape
    max_k = width if max_k is None else max_k
    out = torch.full((rows, topk), -1, dtype=torch.int32)
    for r in range(rows):
        b, i = divmod(r, seqlen_q)
        n = max(0, min(int(lens[b]), max_k))
        x = logits[r, :max(0, min(n - seqlen_q + i + 1, n))].float()
        pos = (~x.isnan() & (x != float("-inf"))).nonzero()[:, 0]
        order = torch.sort(x[pos] + 0.0, descending=True, stable=True).indices
        sel = pos[order[:topk]].sort().values
        blk = table[b, sel // page].long()
        slot = blk * page + sel % page
        ok = (blk >= 0) & (blk < num_blocks) & (slot <= INT32_MAX)
        out[r, :len(sel)] = torch.where(ok, slot, torch.full_like(slot, -1)).int()
    return out
