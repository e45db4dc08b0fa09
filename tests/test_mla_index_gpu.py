"""GPU: the MLA indexer - fmha_mla_index_logits against the float64 reference
over ragged, poisoned paged index caches; the index-key cache append byte for byte; and the V3.2
decode step end to end: append, logits, top-k slots, sparse decode = dense decode.
"""
import pytest
import torch

import xf_flash_attention_cutlass_amd as xfa
from tests import mla_index_util as iu
from tests import mla_util as mu
from xf_flash_attention_cutlass_amd import capi

pytestmark = pytest.mark.gpu
DEV = "cuda"
CHUNK = xfa.paged_attn._mla_index_chunk        # FMHA_MLA_INDEX_CHUNK: keys of one workgroup's item


def _keys(n, gen):
    """Rows whose neighbours' amax (hence descales) differ by >= 4x: a shifted descale shows."""
    k = torch.randn(n, 128, generator=gen)
    k = (k / k.abs().amax(-1, keepdim=True).clamp(min=1e-9) * (8.0 ** (torch.arange(n) % 3))[:, None]).bfloat16()
    a = k.float().abs().amax(-1)
    assert n < 2 or (torch.maximum(a[1:] / a[:-1], a[:-1] / a[1:]) >= 4).all()
    return k


@pytest.mark.parametrize("page", [16, 64])
@pytest.mark.parametrize("sq", [1, 2, 3])
@pytest.mark.parametrize("heads", [32, 64])
def test_logits_match_the_float64_reference(heads, sq, page):
    """One chunk plus 37 keys, 37 keys and no key; a tile straddling pages, a partial last tile, a
    chunk boundary, n < seqlen_q, poison (NaN bytes, NaN descales) behind everything past a
    sequence's end and one table entry equal to num_blocks there."""
    gen = torch.Generator().manual_seed(heads + 7 * sq + page)
    lens = [CHUNK + 37, 37, 0]
    max_k, width = CHUNK + 77, -(-(CHUNK + 77) // page)
    need = [-(-n // page) for n in lens]
    nblocks = sum(need) + 2
    cache = torch.full((nblocks, page * 132), 0xFF, dtype=torch.uint8)
    perm = torch.randperm(nblocks, generator=gen)
    poison = perm[-2:]                                               # never written: stay NaN
    table = poison[torch.randint(0, 2, (3, width), generator=gen)].int()
    table[1, need[1] + 1] = nblocks                                  # past the end: never dereferenced
    at = 0
    for bi, n in enumerate(lens):
        table[bi, :need[bi]] = perm[at:at + need[bi]].int()
        s = torch.arange(n)
        iu.write_slots(cache, page, table[bi, s // page].long() * page + s % page, *iu.quantize_ref(_keys(n, gen)))
        at += need[bi]
    assert not torch.equal(table[0, :need[0]].long(), torch.arange(need[0]))
    wide = torch.randn(3, sq, heads + 8, 128, generator=gen).to(iu.F8).view(torch.uint8)
    q8 = wide[:, :, 4:4 + heads]
    w = torch.randn(3 * sq, heads, generator=gen) * heads ** -0.5
    assert (w > 0).any() and (w < 0).any()
    ref, mag = iu.logits_ref(q8, w, cache, page, table, lens, max_k)

    buf = torch.full((3 * sq, max_k + 24), float("nan"), device=DEV)
    qd = wide.to(DEV)[:, :, 4:4 + heads]
    assert not qd.is_contiguous()
    got = xfa.mla_index_logits(qd, w.to(DEV), cache.to(DEV), table.to(DEV),
                               torch.tensor(lens, dtype=torch.int32, device=DEV), max_k, out=buf[:, :max_k])
    torch.cuda.synchronize()
    kern = capi.lib().fmha_last_kernel().decode()
    assert kern.startswith("fmha_mla_index_logits_kernel<%d>" % heads) and "grid=%dx1x1 block=256" % (3 * 2) in kern, kern
    assert got.data_ptr() == buf.data_ptr() and buf[:, max_k:].isnan().all()       # padding untouched
    got = got.cpu().double()
    dead = ref == iu.NEG_INF
    assert torch.equal(got == iu.NEG_INF, dead) and not got.isnan().any()
    err = torch.where(dead, torch.zeros_like(ref), (got - ref).abs())
    bound = (128 + heads + 8) * 2.0 ** -23 * mag
    worst = (err / bound.clamp(min=1e-300)).max()
    print(f"heads {heads} sq {sq} page {page}: worst err / bound {worst:.3f}, max err {err.max():.3e}")
    assert (err <= bound).all()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("fmt", [None, "ue8m0"])
def test_append_is_byte_exact(fmt, dtype):
    gen = torch.Generator().manual_seed(3)
    page, nblocks, n = 16, 5, 50
    k = _keys(n, gen).to(dtype)
    k[11] = 0
    slots = torch.randperm(nblocks * page, generator=gen)[:n]
    slots[3], slots[20], slots[31] = -1, nblocks * page, nblocks * page - 1
    want = torch.full((nblocks, page * 132), 0x7E, dtype=torch.uint8)
    b8, ds = iu.quantize_ref(k, fmt)
    iu.write_slots(want, page, slots, b8, ds)
    wide = torch.zeros(n, 256, dtype=dtype)
    wide[:, 64:192] = k
    cache = torch.full_like(want, 0x7E).to(DEV)
    xfa.mla_index_cache_append_fp8(wide.to(DEV)[:, 64:192], cache, slots.to(DEV), scale_fmt=fmt)
    assert torch.equal(cache.cpu(), want)                     # bytes, descales, every other byte 0x7E
    dsv = iu.block_views(cache.cpu(), page)[1]
    s = int(slots[11])
    assert dsv[s // page, s % page] == 1.0
    if fmt == "ue8m0":
        assert ((ds.view(torch.int32) & 0x7FFFFF) == 0).all()


def test_decode_step_end_to_end():
    """Index keys through the append, latent rows (the 16-bit cache has no append entry: written by
    slot) through the same slot mapping; logits, top-k slots with topk >= every length, then the
    sparse decode over them equals the dense decode: attention over a permutation of all keys."""
    gen = torch.Generator().manual_seed(5)
    page, lens, heads, topk = 64, [70, 33], 16, 96
    table = torch.tensor([[3, 1], [0, 2]], dtype=torch.int32)
    slots = torch.cat([table[b, torch.arange(n) // page].long() * page + torch.arange(n) % page
                       for b, n in enumerate(lens)])
    latent = torch.randn(sum(lens), mu.D, generator=gen).bfloat16()
    kv = torch.zeros(4, page, 1, mu.D, dtype=torch.bfloat16)
    kv.view(-1, mu.D)[slots] = latent
    icache = torch.zeros(4, xfa.mla_index_cache_block_bytes(page), dtype=torch.uint8, device=DEV)
    xfa.mla_index_cache_append_fp8(torch.randn(sum(lens), 128, generator=gen).bfloat16().to(DEV), icache, slots.to(DEV), "ue8m0")
    q8 = torch.randn(2, 1, 64, 128, generator=gen).to(iu.F8).to(DEV)
    w = (torch.randn(2, 64, generator=gen) / 8).to(DEV)
    lens_d = torch.tensor(lens, dtype=torch.int32, device=DEV)
    logits = xfa.mla_index_logits(q8, w, icache, table.to(DEV), lens_d, 2 * page)
    idx = xfa.mla_index_topk_slots(logits, table.to(DEV), lens_d, topk, page_block_size=page)
    assert idx.shape == (2, 1, topk) and idx.dtype == torch.int32
    for b, n in enumerate(lens):
        assert (idx[b, 0, n:] == -1).all()
        assert torch.equal(idx[b, 0, :n].cpu().long().sort().values, slots[sum(lens[:b]):][:n].sort().values)
    q = torch.randn(2, 1, heads, mu.D, generator=gen).bfloat16()
    sparse = xfa.flash_mla_with_kvcache(q.to(DEV), kv.to(DEV), None, None, indices=idx)
    dense = xfa.flash_mla_with_kvcache(q.to(DEV), kv.to(DEV), table.to(DEV), lens_d)
    rows = latent.float().split(lens)
    ora = mu.oracle(type("Rows", (), dict(kx=[r[:, None, :] for r in rows])), q)
    mu.assert_case("dense", dense[0].cpu(), dense[1].cpu(), ora)
    mu.assert_case("sparse", sparse[0].cpu(), sparse[1].cpu(), ora)
