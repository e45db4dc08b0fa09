"""GPU: fmha_mla_cache_append_fp8 (append to the fp8 paged latent cache) against
the torch restatement of its quantiser and row (tests/mla_fp8_util.py): the written bytes - e4m3
bytes, fp32 descales, rotary features - are held to it EXACTLY, as tests/test_fp8_quantize_gpu.py
holds fmha_quantize_fp8.  Rows go through a shuffled slot_mapping into a cache poisoned with 0x55,
so every byte outside the written rows is shown untouched.
"""
import ctypes as C

import pytest
import torch

from tests import mla_fp8_util as m8
from tests import mla_util as mu
from xf_flash_attention_cutlass_amd import capi

pytestmark = pytest.mark.gpu

DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
PAGE, BLOCKS = 16, 9
POISON = 0x55


def tokens_of(dt, n, seed):
    """[n, 576] in dt: groups that differ, an all-zero group, a row of zeros, one huge and one tiny
    group (descales far apart; fp16: inside its range)."""
    x = m8.make_rows(n, torch.Generator().manual_seed(seed))
    x[3, 128:256] = 0
    x[5] = 0
    x[7, 384:512] *= 1000.0
    x[9, :128] *= 2.0 ** -12
    return x.to(DTYPES[dt])


def shuffled_slots(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randperm(BLOCKS * PAGE, generator=g)[:n].contiguous()


def expected_cache(x, slots):
    """The poisoned cache with row slots[t] = the packed row of token t, for the valid slots."""
    want = torch.full((BLOCKS * PAGE, m8.ROW), POISON, dtype=torch.uint8)
    ok = (slots >= 0) & (slots < BLOCKS * PAGE)
    want[slots[ok]] = m8.rows_of(x.float(), x.dtype)[ok]
    return want.view(BLOCKS, PAGE, 1, m8.ROW)


def poisoned():
    return torch.full((BLOCKS, PAGE, 1, m8.ROW), POISON, dtype=torch.uint8, device=mu.DEV)


@pytest.mark.parametrize("dt", list(DTYPES))
def test_bytes_equal_the_restatement_views_of_one_tensor(dt):
    """latent and k_pe as the two views of one 576-wide tensor; 101 tokens (a partial last
    workgroup) through a shuffled slot_mapping."""
    import xf_flash_attention_cutlass_amd as xfa
    x = tokens_of(dt, 101, 3)
    slots = shuffled_slots(101, 4)
    kc = poisoned()
    xd = x.to(mu.DEV)
    assert not xd[:, :512].is_contiguous()
    xfa.mla_cache_append_fp8(xd[:, :512], xd[:, 512:], kc, slots.to(mu.DEV))
    got, want = kc.cpu(), expected_cache(x, slots)
    gb, gd, gr = m8.unpack_rows(got.view(-1, m8.ROW), DTYPES[dt])
    wb, wd, wr = m8.unpack_rows(want.view(-1, m8.ROW), DTYPES[dt])
    assert torch.equal(gd.view(torch.int32), wd.view(torch.int32)), "descales"
    assert torch.equal(gb, wb), "e4m3 bytes"
    assert torch.equal(gr.view(torch.int16), wr.view(torch.int16)), "rotary features"
    assert torch.equal(got, want)                         # and every other byte is still 0x55
    written = torch.zeros(BLOCKS * PAGE, dtype=torch.bool)
    written[slots] = True
    assert int((got.view(-1, m8.ROW)[~written] != POISON).sum()) == 0 and int((~written).sum()) == BLOCKS * PAGE - 101


@pytest.mark.parametrize("dt", list(DTYPES))
def test_separate_strided_tensors_and_float8_cache(dt):
    """latent and k_pe as separate tensors with row strides of their own (640 and 128 elements,
    a storage offset), the cache given as float8_e4m3fn; through the C ABI too, same bytes."""
    import xf_flash_attention_cutlass_amd as xfa
    x = tokens_of(dt, 40, 5)
    slots = shuffled_slots(40, 6)
    la = torch.full((41, 640), float("nan"), dtype=DTYPES[dt], device=mu.DEV)
    pa = torch.full((41, 128), float("nan"), dtype=DTYPES[dt], device=mu.DEV)
    lat, pe = la[1:, 64:576], pa[1:, 64:]
    lat.copy_(x[:, :512])
    pe.copy_(x[:, 512:])
    want = expected_cache(x, slots)
    kc = poisoned()
    xfa.mla_cache_append_fp8(lat, pe, kc.view(torch.float8_e4m3fn), slots.to(mu.DEV))
    assert torch.equal(kc.cpu(), want)
    kc2 = poisoned()
    sd = slots.to(mu.DEV)
    capi.lib().fmha_mla_cache_append_fp8(lat.data_ptr(), lat.stride(0), pe.data_ptr(), pe.stride(0), kc2.data_ptr(),
                                         sd.data_ptr(), 40, BLOCKS, PAGE, DTYPES[dt] == torch.float16,
                                         capi.stream_handle())
    capi.check()
    torch.cuda.synchronize()
    assert torch.equal(kc2.cpu(), want)


def test_invalid_slots_are_skipped():
    """Negative slots (vLLM's padding, -1) and slots at or past num_blocks * page write nothing; the
    rows around them are written whole."""
    import xf_flash_attention_cutlass_amd as xfa
    x = tokens_of("bf16", 24, 7)
    slots = shuffled_slots(24, 8)
    slots[2], slots[11], slots[17], slots[23] = -1, BLOCKS * PAGE, -(2 ** 40), 2 ** 40
    kc = poisoned()
    xfa.mla_cache_append_fp8(x.to(mu.DEV)[:, :512], x.to(mu.DEV)[:, 512:], kc, slots.to(mu.DEV))
    got = kc.cpu()
    assert torch.equal(got, expected_cache(x, slots))
    assert int((got.view(-1, m8.ROW) != POISON).any(1).sum()) == 20


def test_zero_tokens_and_refusals_leave_the_cache_untouched():
    import xf_flash_attention_cutlass_amd as xfa
    L = capi.lib()
    kc = poisoned()
    x = tokens_of("bf16", 16, 9).to(mu.DEV)
    slots = shuffled_slots(16, 10).to(mu.DEV)
    xfa.mla_cache_append_fp8(x[:0, :512], x[:0, 512:], kc, slots[:0])                      # 0 tokens: succeeds
    L.fmha_mla_cache_append_fp8(x.data_ptr(), 576, x.data_ptr() + 1024, 576, kc.data_ptr(), slots.data_ptr(), 0,
                                BLOCKS, PAGE, False, capi.stream_handle())
    assert L.fmha_last_status() == 0

    def call(lat=x.data_ptr(), ls=576, pe=x.data_ptr() + 1024, ps=576, cache=kc.data_ptr(), sl=slots.data_ptr(),
             n=16, blocks=BLOCKS, page=PAGE):
        L.fmha_mla_cache_append_fp8(lat, ls, pe, ps, cache, sl, n, blocks, page, False, capi.stream_handle())
        return L.fmha_last_status(), L.fmha_last_error().decode()

    for kw, needle in ((dict(lat=None), "non-null"), (dict(sl=None), "non-null"), (dict(ls=580), "multiples of 8"),
                       (dict(ps=572), "multiples of 8"), (dict(pe=x.data_ptr() + 1028), "16-byte aligned"),
                       (dict(cache=kc.data_ptr() + 8), "16-byte aligned"), (dict(sl=slots.data_ptr() + 4), "8-byte aligned"),
                       (dict(page=24), "multiple of 16"), (dict(n=-1), "non-negative"), (dict(blocks=-1), "non-negative")):
        st, msg = call(**kw)
        torch.cuda.synchronize()
        assert st != 0 and needle in msg, msg
        assert int((kc != POISON).sum()) == 0
    for bad, match in ((dict(slots=slots.int()), "int64"), (dict(kc=kc.view(-1, m8.ROW)), "656"),
                       (dict(pe=x[:8, 512:]), "k_pe must be")):
        with pytest.raises(RuntimeError, match=match):
            xfa.mla_cache_append_fp8(x[:, :512], bad.get("pe", x[:, 512:]), bad.get("kc", kc), bad.get("slots", slots))
        assert int((kc != POISON).sum()) == 0
    st, msg = call()
    torch.cuda.synchronize()
    assert st == 0 and int((kc != POISON).any(-1).sum()) == 16


@pytest.mark.parametrize("dt", list(DTYPES))
def test_append_then_decode_equals_decode_over_the_packed_cache(dt):
    """The sequences of a cache built on the CPU, appended on the GPU through the slots its block
    table gives them, decode to the same bits as the CPU-packed cache."""
    import xf_flash_attention_cutlass_amd as xfa
    lens = [117, 33, 16, 0]
    gen = torch.Generator().manual_seed(12)
    seqs = [m8.make_rows(n, gen).to(DTYPES[dt]) for n in lens]
    c = m8.build_cache8([s.float() for s in seqs], PAGE, 1024 // PAGE, DTYPES[dt], "nan", seed=13)
    slots = torch.cat([c.table[i, torch.arange(n) // PAGE].long() * PAGE + torch.arange(n) % PAGE
                       for i, n in enumerate(lens)])
    rows = torch.cat(seqs).to(mu.DEV)
    kc = torch.full(c.kc.shape, 0xFF, dtype=torch.uint8, device=mu.DEV)
    xfa.mla_cache_append_fp8(rows[:, :512], rows[:, 512:], kc, slots.to(mu.DEV))
    assert torch.equal(kc.cpu(), c.kc)
    q = mu.make_q(len(lens), 2, 16, mu.D, DTYPES[dt], 14)
    for ns in (1, 0):
        o0, l0, _, _ = m8.run8(c, q, True, ns)
        o1, l1, _, _ = m8.run8(c, q, True, ns, kc=kc)
        assert torch.equal(o0, o1) and torch.equal(l0, l1)
    ora = mu.oracle(c, q, True)
    mu.assert_case(f"mla8-append-decode-{dt}", o1.cpu(), l1.cpu(), ora)
