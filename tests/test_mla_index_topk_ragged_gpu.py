"""GPU: the MLA indexer's selection for prefill rows (ABI 2.17) -
fmha_mla_index_topk_ragged against the exact CPU reference (torch.equal: the result is a function of
the inputs alone) over poisoned rows of every length and value family; against the decode selection
where both apply; the launch record; a captured graph; a packed prefill step end to end.
"""
import pytest
import torch

import xf_flash_attention_cutlass_amd as xfa
from tests import mla_index_topk_ragged_util as ru
from tests import mla_util as mu
from tests.test_mla_index_topk_gpu import _values
from xf_flash_attention_cutlass_amd import capi

pytestmark = pytest.mark.gpu
DEV = "cuda"
STAGE = xfa.paged_attn._mla_index_topk_ragged_stage   # a threshold bin up to this many keys stays in LDS
SWEEP = 256 * 4                                        # columns of one workgroup step (4 waves x 64 lanes x 4)
SENTINEL = 0x7E7E7E7E


def _problem(family, topk, seed, lens=None, with_slots=True):
    """Rows of every length in one launch, each over its own [ks, ke): lo at every residue mod 4, an
    odd row stride, +inf / NaN in every column outside the range; the last three rows have ks < 0,
    ke > N and ke < ks.  slots: a permutation with one entry negative and one >= 2^31, both under
    columns that rows of at most topk candidates select."""
    gen = torch.Generator().manual_seed(seed)
    lens = lens or [0, 1, topk - 1, topk, topk + 1, SWEEP - 1, SWEEP, SWEEP + 1, STAGE - 1, STAGE, STAGE + 1, 40001]
    ks = [12 * r + r % 4 for r in range(len(lens))]
    n = max(a + b for a, b in zip(ks, lens)) + 2
    ke = [a + b for a, b in zip(ks, lens)] + [topk + 7, n + 100, 10]
    ks = ks + [-5, n - topk - 9, 50]
    m = len(ks)
    logits = torch.empty(m, n + 3)                                  # an odd row stride: every alignment
    logits[:, :n] = _values(family, m, n, gen)
    poison = torch.tensor([float("inf"), float("nan")]).repeat(n)[:n + 3]
    for r in range(m):
        lo, hi = max(0, min(ks[r], n)), max(0, min(ke[r], n))
        logits[r, :lo] = poison[:lo]
        logits[r, max(lo, hi):] = poison[max(lo, hi):]
    slots = None
    if with_slots:
        slots = torch.randperm(n, generator=gen)
        slots[ks[1]], slots[ks[3]] = -3, 2 ** 31
    ks, ke = torch.tensor(ks, dtype=torch.int32), torch.tensor(ke, dtype=torch.int32)
    return logits, n, ks, ke, slots, ru.topk_ragged_ref(logits[:, :n], ks, ke, topk, slots)


@pytest.mark.parametrize("family", ["randn", "three", "equal", "dense", "mixed"])
@pytest.mark.parametrize("with_slots", [False, True])
@pytest.mark.parametrize("topk", [1, 64, 2048])
def test_topk_ragged_equals_the_reference(topk, with_slots, family):
    logits, n, ks, ke, slots, ref = _problem(family, topk, topk + with_slots, with_slots=with_slots)
    buf = torch.full((len(ks), topk + 8), SENTINEL, dtype=torch.int32, device=DEV)
    got = xfa.mla_index_topk_ragged(logits.to(DEV)[:, :n], ks.to(DEV), ke.to(DEV), topk,
                                    slots=slots.to(DEV) if with_slots else None, out=buf[:, :topk])
    torch.cuda.synchronize()
    assert got.data_ptr() == buf.data_ptr() and (buf[:, topk:] == SENTINEL).all()
    got = got.cpu()
    bad = (got != ref).any(-1).nonzero()[:, 0]
    assert torch.equal(got, ref), f"rows {bad.tolist()} of ranges {list(zip(ks.tolist(), ke.tolist()))} differ"


@pytest.mark.parametrize("family", ["randn", "three", "equal", "dense", "mixed"])
def test_agrees_with_the_decode_selection_on_one_causal_sequence(family):
    """ks = 0, ke = N - M + r + 1, slots = the block table expanded: bit-equal to mla_index_topk at
    batch 1, seqlen_q M."""
    gen = torch.Generator().manual_seed(7)
    m, n, page, topk = 5, STAGE + SWEEP + 37, 16, 64
    logits = _values(family, m, n, gen).to(DEV)
    table = torch.randperm(-(-n // page), generator=gen).int()[None]
    pos = torch.arange(n)
    slots = table[0, pos // page].long() * page + pos % page
    want = xfa.mla_index_topk(logits, table.to(DEV), torch.tensor([n], dtype=torch.int32, device=DEV), topk,
                              seqlen_q=m, page_block_size=page)
    ke = (torch.arange(m) + n - m + 1).int()
    got = xfa.mla_index_topk_ragged(logits, torch.zeros(m, dtype=torch.int32, device=DEV), ke.to(DEV), topk,
                                    slots=slots.to(DEV))
    assert torch.equal(got, want[0])


def test_launch_record_and_defaults():
    """fmha_last_kernel() names the kernel and one workgroup of 256 threads per row; out defaults
    to a new int32 [M, topk], slots to the column itself."""
    logits, n, ks, ke, _, ref = _problem("randn", 8, 1, lens=[5, 40, 0], with_slots=False)
    got = xfa.mla_index_topk_ragged(logits[:, :n].contiguous().to(DEV), ks.to(DEV), ke.to(DEV), 8)
    kern = capi.lib().fmha_last_kernel().decode()
    assert kern.startswith("fmha_mla_index_topk_ragged_kernel ") and "grid=6x1x1 block=256" in kern, kern
    assert got.dtype == torch.int32 and got.shape == (6, 8) and torch.equal(got.cpu(), ref)


def test_captured_graph_follows_logits_and_ranges():
    """Captured once, replayed over logits and ks / ke changed in place: every replay equals the
    reference of what it ran on (no host-side state, no scratch)."""
    topk, lens = 64, [SWEEP + 3, 50, STAGE + 1]
    logits, n, ks, ke, slots, _ = _problem("randn", topk, 2, lens=lens)
    ld, ksd, ked = logits.to(DEV), ks.to(DEV), ke.to(DEV)
    out = torch.full((len(ks), topk), SENTINEL, dtype=torch.int32, device=DEV)
    args, kw = (ld[:, :n], ksd, ked, topk), dict(slots=slots.to(DEV), out=out)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        xfa.mla_index_topk_ragged(*args, **kw)                        # warm-up outside the capture
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        xfa.mla_index_topk_ragged(*args, **kw)
    for family, seed, shift in (("three", 3, 0), ("mixed", 4, 5), ("dense", 5, -29)):
        new = _problem(family, topk, seed, lens=lens)[0]
        ld.copy_(new)
        ksd.copy_(ks + shift)
        ked.copy_(ke + 2 * shift)
        out.fill_(SENTINEL)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.cpu(), ru.topk_ragged_ref(new[:, :n], ks + shift, ke + 2 * shift, topk, slots)), family


def test_prefill_step_end_to_end():
    """Two packed sequences: append -> mla_index_logits_ragged -> mla_index_topk_ragged(slots =
    slot_mapping), topk below one length and above the other -> sparse attention at batch 1,
    seqlen_q M: the indices are the reference selection on the kernel's own logits, and the
    attention equals attention over exactly the selected rows."""
    gen = torch.Generator().manual_seed(6)
    page, lens, heads, topk = 64, [100, 33], 16, 48
    m = sum(lens)
    table = [[3, 1], [0]]
    slots = torch.cat([torch.tensor(table[b])[torch.arange(n) // page] * page + torch.arange(n) % page
                       for b, n in enumerate(lens)])
    latent = torch.randn(m, mu.D, generator=gen).bfloat16()
    kv = torch.zeros(4, page, 1, mu.D, dtype=torch.bfloat16)
    kv.view(-1, mu.D)[slots] = latent
    ipage = -(-m // 16) * 16
    icache = torch.zeros(1, xfa.mla_index_cache_block_bytes(ipage), dtype=torch.uint8, device=DEV)
    xfa.mla_index_cache_append_fp8(torch.randn(m, 128, generator=gen).bfloat16().to(DEV), icache, torch.arange(m, device=DEV), "ue8m0")
    k8, scale = icache[0, :m * 128].view(m, 128), icache[0, ipage * 128:].view(torch.float32)[:m]
    q8 = torch.randn(m, 64, 128, generator=gen).to(torch.float8_e4m3fn).to(DEV)
    w = (torch.randn(m, 64, generator=gen) / 8).to(DEV)
    start = torch.tensor([0] * lens[0] + [lens[0]] * lens[1], dtype=torch.int32)
    ks, ke = start.to(DEV), (torch.arange(m) + 1).int().to(DEV)
    logits = xfa.mla_index_logits_ragged(q8, w, k8, scale, ks, ke)
    idx = xfa.mla_index_topk_ragged(logits, ks, ke, topk, slots=slots.to(DEV))
    ref = ru.topk_ragged_ref(logits.cpu(), ks.cpu(), ke.cpu(), topk, slots)
    assert torch.equal(idx.cpu(), ref)
    assert (ref[lens[0] - 1] >= 0).all() and (ref[m - 1, :lens[1]] >= 0).all() and (ref[m - 1, lens[1]:] == -1).all()
    q = torch.randn(m, 1, heads, mu.D, generator=gen).bfloat16()
    o, lse = xfa.flash_mla_with_kvcache(q[:, 0][None].to(DEV), kv.to(DEV), None, None, indices=idx[None])
    rows = [kv.view(-1, mu.D)[r[r >= 0].long()].float() for r in ref]
    ora = mu.oracle(type("Rows", (), dict(kx=[r[:, None, :] for r in rows])), q)
    mu.assert_case("sparse prefill over the kernel's indices", o[0][:, None].cpu(), lse[0].t()[:, :, None].cpu(), ora)
