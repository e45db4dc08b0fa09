"""GPU: the MLA indexer's selection with rows split over workgroups (ABI 2.18) -
fmha_mla_index_topk_split against the exact CPU reference (torch.equal) over ragged, poisoned rows
of every value family, with lengths around the chunk length, a poisoned caller workspace and a
sentinel behind the output; against the one-workgroup kernel; a captured graph over pooled scratch.
"""
import pytest
import torch

import xf_flash_attention_cutlass_amd as xfa
from tests.test_mla_index_topk_gpu import DEV, SENTINEL, STAGE, _problem
from xf_flash_attention_cutlass_amd import capi

pytestmark = pytest.mark.gpu
LONGEST = 40001
FAMILIES = ["randn", "three", "equal", "dense", "mixed"]


def _chunk(max_k, splits):
    """L of include/paged_attn.h: ceil(max_seqlen_k / splits), rounded up to a multiple of 4"""
    return (-(-max_k // splits) + 3) // 4 * 4


def _lens(topk, splits):
    """Lengths around every boundary of the split; _problem's max_seqlen_k is the longest + 2.  (With
    2 splits no row is longer than 2 L: that length is the longest row.)"""
    L = _chunk(LONGEST + 2, splits)
    return [0, 1, topk - 1, topk + 1, L - 1, L, L + 1, min(2 * L + 1, LONGEST), STAGE + 1, LONGEST]


@pytest.mark.parametrize("topk,page,sq,family", [(t, 16, 3, f) for t in (1, 64, 2048) for f in FAMILIES] + [(64, 64, 1, "mixed")])
@pytest.mark.parametrize("splits", [2, 5, 16])
def test_split_equals_the_reference(splits, topk, page, sq, family):
    logits, table, lens, nblocks, max_k, ref = _problem(family, topk, page, sq, topk + page + sq + splits,
                                                        lens=_lens(topk, splits))
    assert max_k == LONGEST + 2 and splits * topk <= STAGE
    buf = torch.full((len(lens), sq, topk + 8), SENTINEL, dtype=torch.int32, device=DEV)
    ws = torch.full((capi.lib().fmha_mla_index_topk_split_workspace_size(len(lens) * sq, topk, splits),), 0x7E,
                    dtype=torch.uint8, device=DEV)
    got = xfa.paged_attn.mla_index_topk_split(logits.to(DEV)[:, :max_k], table.to(DEV), lens.to(DEV), topk, sq, page,
                                              max_k, nblocks, buf[..., :topk], splits, ws)
    torch.cuda.synchronize()
    assert got.data_ptr() == buf.data_ptr() and (buf[..., topk:] == SENTINEL).all()
    got = got.cpu()
    bad = (got != ref).any(-1).nonzero()
    assert torch.equal(got, ref), f"rows (batch, position) {bad.tolist()[:8]} of lengths {lens.tolist()} differ"


@pytest.mark.parametrize("splits", [2, 7])
def test_split_equals_one_workgroup(splits):
    """Forced splits against splits=1 on the same inputs, bit for bit; the launch record names the
    last launch, the merge kernel with one workgroup a row."""
    topk, page, sq = 512, 64, 2
    logits, table, lens, nblocks, max_k, ref = _problem("three", topk, page, sq, 7, lens=_lens(topk, splits))
    args = (logits.to(DEV)[:, :max_k], table.to(DEV), lens.to(DEV), topk)
    kw = dict(seqlen_q=sq, page_block_size=page, num_blocks=nblocks)
    one = xfa.mla_index_topk(*args, splits=1, **kw)
    assert capi.lib().fmha_last_kernel().decode().startswith("fmha_mla_index_topk_kernel ")
    got = xfa.mla_index_topk(*args, splits=splits, **kw)
    kern = capi.lib().fmha_last_kernel().decode()
    assert kern.startswith("fmha_mla_index_topk_merge_kernel ") and f"grid={len(lens) * sq}x1x1 block=" in kern, kern
    assert torch.equal(got, one) and torch.equal(got.cpu(), ref)


def test_captured_graph_over_pooled_scratch():
    """Captured once with the pool's scratch, replayed over logits changed in place: every replay
    equals the reference of the logits it ran on."""
    topk, page, sq, splits = 64, 16, 1, 4
    L = _chunk(33002, splits)
    lens = [L - 3, L + 5, 50, 3 * L + 1, 33000]
    logits, table, lens_t, nblocks, max_k, _ = _problem("randn", topk, page, sq, 2, lens=lens)
    ld, out = logits.to(DEV), torch.full((len(lens), sq, topk), SENTINEL, dtype=torch.int32, device=DEV)
    args = (ld[:, :max_k], table.to(DEV), lens_t.to(DEV), topk)
    kw = dict(seqlen_q=sq, page_block_size=page, num_blocks=nblocks, out=out, splits=splits)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        xfa.mla_index_topk(*args, **kw)                           # warm-up outside the capture: the pool's block
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        xfa.mla_index_topk(*args, **kw)
    for family, seed in (("three", 3), ("mixed", 4), ("dense", 5)):
        new = _problem(family, topk, page, sq, seed, lens=lens, table=table)
        ld.copy_(new[0])
        out.fill_(SENTINEL)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.cpu(), new[5]), family
