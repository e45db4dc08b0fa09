"""CPU: the MLA indexer (ABI 2.14) - the restated quantiser and block layout, the
float64 reference of the logits, the 2.14 surface, and every refusal of the two C entries that
needs no device (fake aligned pointers: each case fails before a launch), reported through
fmha_last_error().
"""
import ctypes as C

import pytest
import torch

from tests import mla_index_util as iu
from xf_flash_attention_cutlass_amd import capi

SYMS = ("fmha_mla_index_cache_append_fp8", "fmha_mla_index_logits")
FAKE = 0x10000


@pytest.mark.parametrize("fmt", [None, "ue8m0"])
def test_quantiser_and_layout(fmt):
    g = torch.Generator().manual_seed(1)
    k = (torch.randn(40, 128, generator=g) * (8.0 ** (torch.arange(40) % 3))[:, None]).bfloat16()
    k[7] = 0
    b8, ds = iu.quantize_ref(k, fmt)
    amax = k.float().abs().amax(-1)
    assert ds[7] == 1.0 and (b8[7] == 0).all()
    live = amax > 0
    if fmt == "ue8m0":
        assert ((ds.view(torch.int32) & 0x7FFFFF) == 0).all()
        assert (ds[live] >= amax[live] / 448.0).all() and (ds[live] < 2 * amax[live] / 448.0).all()
    else:
        assert torch.equal(ds[live], amax[live] / 448.0)
    back = b8.view(iu.F8).float() * ds[:, None]
    assert ((back - k.float()).abs() <= amax[:, None] * 2.0 ** -3).all()         # e4m3: 3 mantissa bits
    cache = torch.full((3, 16 * 132), 0x7E, dtype=torch.uint8)
    slots = torch.randperm(48, generator=g)[:40]
    iu.write_slots(cache, 16, slots, b8, ds)
    raw = cache.view(3, 16 * 132)
    s = int(slots[5])
    assert torch.equal(raw[s // 16, (s % 16) * 128:(s % 16 + 1) * 128], b8[5])
    assert raw[s // 16, 16 * 128 + 4 * (s % 16):][:4].view(torch.float32)[0] == ds[5]


def test_reference_matches_the_definition():
    """logits_ref against the plain triple loop on a 2-sequence problem, causal rule included."""
    g = torch.Generator().manual_seed(2)
    page, lens, sq, heads = 16, [19, 1], 2, 32
    k = torch.randn(48, 128, generator=g).bfloat16()
    b8, ds = iu.quantize_ref(k)
    cache = torch.full((3, page * 132), 0xFF, dtype=torch.uint8)
    iu.write_slots(cache, page, torch.arange(48), b8, ds)
    table = torch.tensor([[2, 0], [1, 3]], dtype=torch.int32)
    q8 = torch.randn(2, sq, heads, 128, generator=g).to(iu.F8).view(torch.uint8)
    w = torch.randn(2 * sq, heads, generator=g)
    ref, mag = iu.logits_ref(q8, w, cache, page, table, lens, 24)
    for bi, n in enumerate(lens):
        for i in range(sq):
            vis = max(0, min(n - sq + i + 1, n))
            assert (ref[bi * sq + i, vis:] == iu.NEG_INF).all()
            for s in range(vis):
                slot = int(table[bi, s // page]) * page + s % page
                dot = q8[bi, i].view(iu.F8).double() @ b8[slot].view(iu.F8).double()
                want = float(ds[slot]) * float((w[bi * sq + i].double() * dot.clamp(min=0)).sum())
                assert abs(float(ref[bi * sq + i, s]) - want) <= 1e-12 * float(mag[bi * sq + i, s])


def test_surface_2_14():
    import xf_flash_attention_cutlass_amd as xfa
    from tests.test_abi import header_symbols
    for sym in SYMS:
        assert sym in header_symbols() and sym in capi.EXPORTED and hasattr(capi.lib(), sym)
    ver = capi.lib().fmha_version().decode().split()[1]
    assert tuple(int(x) for x in ver.split(".")) >= (2, 14)
    for op in ("mla_index_logits", "mla_index_cache_append_fp8"):
        assert getattr(xfa.paged_attn, op) is getattr(xfa.paged_attn, "_" + op)
        assert op not in dir(xfa.paged_attn)
    for name in ("mla_index_logits", "mla_index_cache_append_fp8", "mla_index_topk_slots", "mla_index_cache_block_bytes"):
        assert name in xfa.__all__ and callable(getattr(xfa, name))
    assert xfa.mla_index_cache_block_bytes(64) == 64 * 132
    assert xfa.paged_attn._mla_index_chunk % 128 == 0


def _append(k=FAKE, k_row=128, cache=FAKE + (1 << 30), slots=FAKE + (1 << 29), tokens=4, blocks=8, page=64, fmt=0):
    L = capi.lib()
    L.fmha_mla_index_cache_append_fp8(k, k_row, cache, slots, tokens, blocks, page, fmt, False, None)
    return L.fmha_last_status(), L.fmha_last_error().decode()


@pytest.mark.parametrize("over,needle", [
    (dict(k=None), "non-null"), (dict(cache=None), "non-null"), (dict(slots=None), "non-null"),
    (dict(tokens=-1), "non-negative"), (dict(blocks=-1), "non-negative"),
    (dict(page=24), "positive multiple of 16"), (dict(page=0), "positive multiple of 16"),
    (dict(fmt=2), "scale_fmt"), (dict(fmt=-1), "scale_fmt"),
    (dict(k_row=-128), "multiple of 8"), (dict(k_row=132), "multiple of 8"),
    (dict(k=FAKE + 8), "16-byte aligned"), (dict(cache=FAKE + (1 << 30) + 4), "16-byte aligned"),
    (dict(slots=FAKE + (1 << 29) + 4), "8-byte aligned"),
])
def test_append_refusals(over, needle):
    st, msg = _append(**over)
    assert st != 0 and needle in msg, msg
    assert _append(tokens=0) == (0, "")                       # an empty append succeeds, unlaunched


def _logits(q=FAKE, w=FAKE + (1 << 26), cache=FAKE + (1 << 30), out=FAKE + (1 << 29), table=FAKE + (1 << 27),
            bt=20, lens=FAKE + (1 << 25), sq=1, max_k=1061, batch=0, heads=64, d=128, blocks=64, page=64,
            strides=(64 * 128, 64 * 128, 128), row=1101):
    L = capi.lib()
    st = None if strides is None else (C.c_int64 * 3)(*strides)
    L.fmha_mla_index_logits(q, w, cache, out, table, bt, lens, sq, max_k, batch, heads, d, blocks, page, st, row, None)
    return L.fmha_last_status(), L.fmha_last_error().decode(), L.fmha_last_kernel().decode()


@pytest.mark.parametrize("over,needle", [
    (dict(q=None), "non-null"), (dict(w=None), "non-null"), (dict(cache=None), "non-null"),
    (dict(out=None), "non-null"), (dict(table=None), "non-null"), (dict(lens=None), "non-null"),
    (dict(strides=None), "q_strides must be a non-null"),
    (dict(heads=16), "32 or 64 heads"), (dict(heads=128), "32 or 64 heads"), (dict(d=64), "head_size 128"),
    (dict(sq=0), "seqlen_q must be at least 1"), (dict(batch=-1), "non-negative"),
    (dict(page=24), "positive multiple of 16"), (dict(page=0), "positive multiple of 16"),
    (dict(blocks=0), "num_blocks must be at least 1"),
    (dict(max_k=-1), "max_seqlen_k must lie in"), (dict(max_k=20 * 64 + 1, row=4096), "max_seqlen_k must lie in"),
    (dict(row=1060), "logits_row_stride"),
    (dict(batch=2, strides=(-8192, 8192, 128)), "multiples of 16"), (dict(strides=(8192, 8192, 72)), "multiples of 16"),
    (dict(q=FAKE + 8), "16-byte aligned"), (dict(cache=FAKE + (1 << 30) + 8), "16-byte aligned"),
    (dict(w=FAKE + (1 << 26) + 2), "4-byte aligned"), (dict(out=FAKE + (1 << 29) + 1), "4-byte aligned"),
    (dict(table=FAKE + (1 << 27) + 2), "4-byte aligned"), (dict(lens=FAKE + (1 << 25) + 2), "4-byte aligned"),
    (dict(batch=1 << 30, max_k=1 << 20, bt=1 << 14, row=1 << 20), "more than one launch covers"),
])
def test_logits_refusals(over, needle):
    st, msg, kern = _logits(**over)
    assert st != 0 and needle in msg and kern == "", (msg, kern)
    assert _logits() == (0, "", "")                           # batch 0: validated, unlaunched, fine
