"""GPU: the MLA indexer's selection (ABI 2.15) - fmha_mla_index_topk against the
exact CPU reference (torch.equal: the result is a function of the inputs alone) over ragged,
poisoned rows of every value family; the launch record; a captured graph; the V3.2 decode step end
to end with the kernel in place of the torch glue.
"""
import pytest
import torch

import xf_flash_attention_cutlass_amd as xfa
from tests import mla_index_topk_util as tu
from tests import mla_util as mu
from xf_flash_attention_cutlass_amd import capi

pytestmark = pytest.mark.gpu
DEV = "cuda"
STAGE = xfa.paged_attn._mla_index_topk_stage     # rows up to this many visible keys stay in LDS
SWEEP = 1024 * 4                                 # columns of one workgroup step (16 waves x 64 lanes x 4)
SENTINEL = 0x7E7E7E7E
SPECIAL = [0.0, -0.0, float("inf"), float("-inf"), float("nan"), 1e-40, -1e-40]


def _values(family, rows, width, gen):
    if family == "randn":
        return torch.randn(rows, width, generator=gen)
    if family == "three":                        # the threshold falls among ties: positions decide
        return torch.tensor([-1.5, 0.25, 2.0])[torch.randint(0, 3, (rows, width), generator=gen)]
    if family == "equal":
        return torch.full((rows, width), 0.5)
    if family == "dense":                        # 1 + j 2^-23, permuted: the high digits are shared
        j = torch.stack([torch.randperm(width, generator=gen) for _ in range(rows)])
        return (j.double() * 2.0 ** -23 + 1.0).float()
    x = torch.randn(rows, width, generator=gen)  # "mixed": signs, both zeros, infinities, NaN, subnormals
    kind = torch.randint(0, 12, (rows, width), generator=gen)
    for i, v in enumerate(SPECIAL):
        x[kind == i] = v
    return x


def _problem(family, topk, page, sq, seed, lens=None, table=None):
    """Rows of several lengths in one batch, poison behind every row's visible columns, rows that
    start at every offset from a 16-byte boundary, a permuted block table with one entry equal to
    num_blocks under the longest sequence's first page."""
    gen = torch.Generator().manual_seed(seed)
    lens = lens or [0, 1, topk - 1, topk, topk + 1, SWEEP + 1, SWEEP + 3, STAGE - 1, STAGE, STAGE + 1, 40001]
    b, max_k = len(lens), max(lens) + 2
    width = -(-max_k // page)
    logits = torch.empty(b * sq, max_k + 3)                     # an odd row stride: every alignment
    logits[:, :max_k] = _values(family, b * sq, max_k, gen)
    for r in range(b * sq):
        n = lens[r // sq]
        vis = max(0, min(n - sq + r % sq + 1, n))
        logits[r, vis:] = torch.tensor([float("inf"), float("nan")]).repeat(max_k)[:max_k + 3 - vis]
    nblocks = b * width
    if table is None:
        table = torch.randperm(nblocks, generator=gen).int().view(b, width)
        assert not torch.equal(table.flatten().long(), torch.arange(nblocks))
        table[lens.index(max(lens)), 0] = nblocks
    ref = tu.topk_ref(logits[:, :max_k], table, lens, topk, sq, page, nblocks)
    return logits, table, torch.tensor(lens, dtype=torch.int32), nblocks, max_k, ref.view(b, sq, topk)


@pytest.mark.parametrize("family", ["randn", "three", "equal", "dense", "mixed"])
@pytest.mark.parametrize("sq", [1, 3])
@pytest.mark.parametrize("page", [16, 64])
@pytest.mark.parametrize("topk", [1, 64, 2048])
def test_topk_equals_the_reference(topk, page, sq, family):
    logits, table, lens, nblocks, max_k, ref = _problem(family, topk, page, sq, topk + page + sq)
    buf = torch.full((len(lens), sq, topk + 8), SENTINEL, dtype=torch.int32, device=DEV)
    got = xfa.mla_index_topk(logits.to(DEV)[:, :max_k], table.to(DEV), lens.to(DEV), topk, seqlen_q=sq,
                             page_block_size=page, num_blocks=nblocks, out=buf[..., :topk])
    torch.cuda.synchronize()
    assert got.data_ptr() == buf.data_ptr() and (buf[..., topk:] == SENTINEL).all()
    got = got.cpu()
    bad = (got != ref).any(-1).nonzero()
    assert torch.equal(got, ref), f"rows (batch, position) {bad.tolist()[:8]} of lengths {lens.tolist()} differ"


def test_launch_record_and_defaults():
    """fmha_last_kernel() names the kernel and one workgroup per row; max_seqlen_k defaults to the
    logits' width, num_blocks to "unknown", out to a new tensor."""
    logits, table, lens, nblocks, max_k, ref = _problem("randn", 8, 16, 2, 1, lens=[5, 40, 0])
    table[1, 0] = 7                                               # (no bad entry: num_blocks is unknown)
    ref = tu.topk_ref(logits[:, :max_k], table, lens, 8, 2, 16, nblocks).view(3, 2, 8)
    got = xfa.mla_index_topk(logits[:, :max_k].contiguous().to(DEV), table.to(DEV), lens.to(DEV), 8, seqlen_q=2,
                             page_block_size=16)
    kern = capi.lib().fmha_last_kernel().decode()
    assert kern.startswith("fmha_mla_index_topk_kernel ") and "grid=6x1x1 block=1024" in kern, kern
    assert got.dtype == torch.int32 and got.shape == (3, 2, 8) and torch.equal(got.cpu(), ref)


def test_captured_graph_follows_the_logits():
    """Captured once, replayed over logits changed in place: every replay equals the reference of
    the logits it ran on (no host-side state, no scratch)."""
    topk, page, sq, lens = 64, 16, 1, [SWEEP + 3, 50, STAGE + 1]
    logits, table, lens_t, nblocks, max_k, _ = _problem("randn", topk, page, sq, 2, lens=lens)
    ld, out = logits.to(DEV), torch.full((3, sq, topk), SENTINEL, dtype=torch.int32, device=DEV)
    args = (ld[:, :max_k], table.to(DEV), lens_t.to(DEV), topk)
    kw = dict(seqlen_q=sq, page_block_size=page, num_blocks=nblocks, out=out)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        xfa.mla_index_topk(*args, **kw)                           # warm-up outside the capture
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


def test_decode_step_end_to_end():
    """append -> mla_index_logits -> mla_index_topk (topk below one context, above the other) ->
    sparse decode: the indices are the reference selection on the kernel's own logits, and the
    decode equals attention over exactly the selected rows."""
    gen = torch.Generator().manual_seed(6)
    page, lens, heads, topk = 64, [100, 33], 16, 48
    table = torch.tensor([[3, 1], [0, 2]], dtype=torch.int32)
    slots = torch.cat([table[b, torch.arange(n) // page].long() * page + torch.arange(n) % page
                       for b, n in enumerate(lens)])
    latent = torch.randn(sum(lens), mu.D, generator=gen).bfloat16()
    kv = torch.zeros(4, page, 1, mu.D, dtype=torch.bfloat16)
    kv.view(-1, mu.D)[slots] = latent
    icache = torch.zeros(4, xfa.mla_index_cache_block_bytes(page), dtype=torch.uint8, device=DEV)
    xfa.mla_index_cache_append_fp8(torch.randn(sum(lens), 128, generator=gen).bfloat16().to(DEV), icache, slots.to(DEV), "ue8m0")
    q8 = torch.randn(2, 1, 64, 128, generator=gen).to(torch.float8_e4m3fn).to(DEV)
    w = (torch.randn(2, 64, generator=gen) / 8).to(DEV)
    lens_d = torch.tensor(lens, dtype=torch.int32, device=DEV)
    logits = xfa.mla_index_logits(q8, w, icache, table.to(DEV), lens_d, 2 * page)
    idx = xfa.mla_index_topk(logits, table.to(DEV), lens_d, topk, page_block_size=page, num_blocks=4)
    ref = tu.topk_ref(logits.cpu(), table, lens, topk, 1, page, 4)
    assert torch.equal(idx.cpu(), ref.view(2, 1, topk))
    assert (ref[0] >= 0).all() and (ref[1, :33] >= 0).all() and (ref[1, 33:] == -1).all()
    q = torch.randn(2, 1, heads, mu.D, generator=gen).bfloat16()
    sparse = xfa.flash_mla_with_kvcache(q.to(DEV), kv.to(DEV), None, None, indices=idx)
    rows = [kv.view(-1, mu.D)[r[r >= 0].long()].float() for r in ref]
    ora = mu.oracle(type("Rows", (), dict(kx=[r[:, None, :] for r in rows])), q)
    mu.assert_case("sparse over the kernel's indices", sparse[0].cpu(), sparse[1].cpu(), ora)
