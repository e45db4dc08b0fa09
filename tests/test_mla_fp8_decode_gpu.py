"""GPU: fmha_mla_decode_fp8 (MLA decode over an fp8 paged latent cache) against
the CPU oracle over the operand - the dequantised rows rounded to q's dtype - per sequence
(tests/mla_util.py's rule, unchanged), on byte caches behind a permuted block table whose every
byte outside the sequences is 0xFF (NaN as e4m3fn, bf16, fp16 and fp32), into NaN-filled outputs,
with inputs whose 128-feature groups differ (tests/mla_fp8_util.py).  Every case asserts the
kernel, its mapping, its grid and the split count (mla_fp8_util.run8).

It mirrors tests/test_mla_decode_gpu.py: bf16 / fp16 x the four shapes x num_splits {1, 3, 0} over
517 ... 0 keys; large pages, a tile straddling pages, fill independence, a non-default scale,
strided views, the three surfaces, reproducibility, a NULL LSE, refusals, graph capture of append
followed by decode, and which kernel a 16-bit and an fp8 cache reach through the Python wrapper.
"""
import ctypes as C

import pytest
import torch

from tests import mla_fp8_util as m8
from tests import mla_util as mu
from xf_flash_attention_cutlass_amd import capi

pytestmark = pytest.mark.gpu

DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
_CACHE, _ORACLE = {}, {}


def cache_of(dt, fill="nan", page=mu.PAGE):
    key = (dt, fill, page)
    if key not in _CACHE:
        _CACHE[key] = m8.make_cache8(list(mu.LENS), DTYPES[dt], fill, seed=23, page=page)
    return _CACHE[key]


def problem(dt, shape, page=mu.PAGE):
    """(cache, q, causal, oracle), computed once and shared (the oracle depends on neither the fill
    nor the page size: the sequences' rows are the same)."""
    h, sq, causal = mu.SHAPES[shape]
    c = cache_of(dt, page=page)
    q = mu.make_q(len(mu.LENS), sq, h, mu.D, DTYPES[dt], 23)
    if (dt, shape) not in _ORACLE:
        _ORACLE[dt, shape] = mu.oracle(cache_of(dt), q, causal)
    return c, q, causal, _ORACLE[dt, shape]


@pytest.mark.parametrize("num_splits", [1, 3, 0])
@pytest.mark.parametrize("shape", list(mu.SHAPES))
@pytest.mark.parametrize("dt", list(DTYPES))
def test_instances(dt, shape, num_splits, parity_report):
    c, q, causal, ora = problem(dt, shape)
    o, lse, kern, splits = m8.run8(c, q, causal, num_splits)
    mu.assert_case(f"mla8-{dt}-{shape}-splits{num_splits}", o.cpu(), lse.cpu(), ora, parity_report)


@pytest.mark.parametrize("num_splits", [1, 0])
def test_page_64(num_splits, parity_report):
    """A 64-row page holds two tiles; its halves 16 rows on are rows of the same page."""
    c, q, causal, ora = problem("bf16", "h8_sq3_causal", page=64)
    assert torch.equal(c.kx[0], cache_of("bf16").kx[0])
    o, lse, _, _ = m8.run8(c, q, causal, num_splits)
    mu.assert_case(f"mla8-page64-splits{num_splits}", o.cpu(), lse.cpu(), ora, parity_report)


def test_page_16_tile_straddles_pages(parity_report):
    """Page 16: every 32-key tile is two pages, which the permuted table puts apart."""
    c, q, causal, ora = problem("fp16", "h16_sq1")
    tab = c.table[0, :(517 + 15) // 16].long()
    assert ((tab[1::2] - tab[0:-1:2]) != 1).any()
    o, lse, _, _ = m8.run8(c, q, causal, 3)
    mu.assert_case("mla8-page16-straddle", o.cpu(), lse.cpu(), ora, parity_report)


@pytest.mark.parametrize("shape,num_splits", [("h8_sq3_causal", 1), ("h16_sq1", 0)])
def test_fill_independence(shape, num_splits):
    """What lies outside the sequences (rows past their ends - e4m3 bytes, descales and rotary
    features alike -, the pages no entry names, the poison page the table's tail points at) does
    not reach the outputs: caches filled with 0x00, 0xFF and 0x7E give the same bits."""
    h, sq, causal = mu.SHAPES[shape]
    q = mu.make_q(len(mu.LENS), sq, h, mu.D, torch.bfloat16, 23)
    got = []
    for fill in ("zero", "nan", "big"):
        c = cache_of("bf16", fill)
        assert int(c.kc[c.poison].min()) == int(c.kc[c.poison].max()) == m8.FILL_BYTES[fill]
        o, lse, _, _ = m8.run8(c, q, causal, num_splits)
        got.append((o.cpu(), lse.cpu()))
        assert not torch.isnan(got[-1][0]).any() and not torch.isnan(got[-1][1]).any()
    for o, lse in got[1:]:
        assert torch.equal(o, got[0][0]) and torch.equal(lse, got[0][1])


def test_scale(parity_report):
    """softmax_scale = 2 x 576^-1/2 against the oracle over 2 q (exact in bf16)."""
    c, q, causal, _ = problem("bf16", "h16_sq1")
    ora = mu.oracle(c, q, causal, q_mul=2.0)
    o, lse, _, _ = m8.run8(c, q, causal, 3, scale=2.0 * mu.D ** -0.5)
    mu.assert_case("mla8-scale2", o.cpu(), lse.cpu(), ora, parity_report)


def test_strided_views(parity_report):
    """q and o as views inside NaN-poisoned arenas: the arena is untouched outside o."""
    c, q, causal, ora = problem("bf16", "h8_sq3_causal")
    b, sq, h, _ = q.shape
    qa = torch.full((b, sq + 1, h + 2, mu.D + 64), float("nan"), dtype=q.dtype, device=mu.DEV)
    qv = qa[:, 1:, 1:h + 1, 64:]
    qv.copy_(q)
    oa = torch.full((b, sq + 2, h + 1, mu.DV + 128), float("nan"), dtype=q.dtype, device=mu.DEV)
    ov = oa[:, 1:sq + 1, :h, 64:64 + mu.DV]
    assert not qv.is_contiguous() and not ov.is_contiguous()
    for ns in (1, 3):
        ov.fill_(float("nan"))
        o, lse, _, _ = m8.run8(c, q, causal, ns, o=ov, qd=qv)
        mu.assert_case(f"mla8-strided-splits{ns}", ov.cpu(), lse.cpu(), ora, parity_report)
        inside = torch.zeros_like(oa, dtype=torch.bool)
        inside[:, 1:sq + 1, :h, 64:64 + mu.DV] = True
        assert torch.isnan(oa[~inside]).all()
    assert torch.isnan(qa[:, 0]).all()


def test_surfaces_bitwise_equal_and_reproducible():
    """The C ABI, the pybind op and the Python wrapper (a uint8 and a float8_e4m3fn view of the
    cache) give the same bits, and so do two calls."""
    import xf_flash_attention_cutlass_amd as xfa
    c, q, causal, _ = problem("fp16", "h40_sq2_causal")
    kc, tab = c.kc.to(mu.DEV), c.table.to(mu.DEV)
    lens = torch.tensor(c.lens, dtype=torch.int32, device=mu.DEV)
    qd = q.to(mu.DEV)
    for ns in (1, 0):
        o0, l0, _, splits = m8.run8(c, q, causal, ns)
        o1, l1, _, _ = m8.run8(c, q, causal, ns)
        assert torch.equal(o0, o1) and torch.equal(l0, l1)
        o2, l2 = xfa.paged_attn.mla_decode_fp8(qd, kc, tab, lens, 512, mu.D ** -0.5, causal, ns, None)
        assert capi.lib().fmha_last_num_splits() == splits
        o3, l3 = xfa.flash_mla_with_kvcache(qd, kc, tab, lens, causal=causal, num_splits=ns)
        out = torch.full_like(o0, float("nan"))
        o4, l4 = xfa.flash_mla_with_kvcache(qd, kc.view(torch.float8_e4m3fn), tab, lens, causal=causal,
                                            num_splits=ns, out=out)
        assert o4 is out
        for o, l in ((o2, l2), (o3, l3), (o4, l4)):
            assert torch.equal(o, o0) and torch.equal(l, l0)


def test_no_lse_pointer():
    c, q, causal, _ = problem("bf16", "h16_sq1")
    for ns in (1, 3):
        o0, _, _, _ = m8.run8(c, q, causal, ns)
        o1, lse, _, _ = m8.run8(c, q, causal, ns, want_lse=False)
        assert lse is None and torch.equal(o0, o1)


def test_refused_calls_leave_outputs_untouched():
    L = capi.lib()
    c, q, causal, _ = problem("bf16", "h16_sq1")
    b, sq, h, _ = q.shape
    qd, kc, tab = q.to(mu.DEV), c.kc.to(mu.DEV), c.table.to(mu.DEV)
    lens = torch.tensor(c.lens, dtype=torch.int32, device=mu.DEV)
    o = torch.full((b, sq, h, mu.DV), float("nan"), dtype=q.dtype, device=mu.DEV)
    lse = torch.full((b, h, sq), float("nan"), dtype=torch.float32, device=mu.DEV)
    dense = [qd.stride(0), qd.stride(1), qd.stride(2), o.stride(0), o.stride(1), o.stride(2)]

    def call(d=mu.D, dv=mu.DV, page=c.page, window=(-1, -1), splits=0, table=tab.data_ptr(), strides=dense,
             max_sk=c.width * c.page):
        st = (C.c_int64 * 6)(*strides)
        L.fmha_mla_decode_fp8(qd.data_ptr(), kc.data_ptr(), o.data_ptr(), lse.data_ptr(), table, tab.stride(0),
                              lens.data_ptr(), sq, max_sk, b, h, d, dv, page, st, mu.D ** -0.5,
                              window[0], window[1], splits, False, capi.stream_handle())
        return L.fmha_last_status(), L.fmha_last_error().decode()

    for kw, needle in ((dict(d=512), "(576, 512) only"), (dict(d=656), "(576, 512) only"),
                       (dict(page=24), "multiple of 16"),
                       (dict(window=(64, 0)), "(-1, -1) and (-1, 0)"), (dict(splits=129), "at most 128"),
                       (dict(table=None), "block_table"), (dict(max_sk=c.width * c.page + 1), "max_seqlen_k"),
                       (dict(strides=dense[:5] + [516]), "multiples of 8")):
        st, msg = call(**kw)
        torch.cuda.synchronize()
        assert st != 0 and needle in msg, msg
        assert L.fmha_last_kernel() == b"" and L.fmha_last_num_splits() == 0
        assert torch.isnan(o).all() and torch.isnan(lse).all()
    st, msg = call()
    torch.cuda.synchronize()
    assert st == 0 and not torch.isnan(o).any()


def test_graph_capture_append_then_decode():
    """One capture of append followed by decode, replayed on an emptied cache and NaN outputs after
    a warm-up call (the scratch pool is warm: no allocation and no host sync inside the capture),
    equals the eager result."""
    import xf_flash_attention_cutlass_amd as xfa
    dt = torch.bfloat16
    lens_l, page, h = [200, 77, 33, 0], 16, 128
    gen = torch.Generator().manual_seed(77)
    seqs = [m8.make_rows(n, gen).to(dt) for n in lens_l]
    c = m8.build_cache8([s.float() for s in seqs], page, 1024 // page, dt, "nan", seed=5)
    tab = c.table.to(mu.DEV)
    lens = torch.tensor(lens_l, dtype=torch.int32, device=mu.DEV)
    rows = torch.cat(seqs).to(mu.DEV)                                   # [tokens, 576]
    slots = torch.cat([c.table[i, torch.arange(n) // page].long() * page + torch.arange(n) % page
                       for i, n in enumerate(lens_l)]).to(mu.DEV)
    q = mu.make_q(len(lens_l), 1, h, mu.D, dt, 77).to(mu.DEV)
    empty = torch.full(c.kc.shape, 0xFF, dtype=torch.uint8, device=mu.DEV)
    kc = empty.clone()
    out = torch.full((len(lens_l), 1, h, mu.DV), float("nan"), dtype=dt, device=mu.DEV)

    def step():
        xfa.mla_cache_append_fp8(rows[:, :512], rows[:, 512:], kc, slots)
        return xfa.flash_mla_with_kvcache(q, kc, tab, lens, out=out)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        o0, l0 = step()                                                 # warm-up on the capture stream
        want_o, want_l = o0.clone(), l0.clone()
        splits = capi.lib().fmha_last_num_splits()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert splits > 1 and torch.equal(kc.cpu(), c.kc)                   # the append wrote the packed rows
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        _, l1 = step()
    kc.copy_(empty)
    out.fill_(float("nan"))
    l1.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want_o) and torch.equal(l1, want_l) and torch.equal(kc.cpu(), c.kc)
    ora = mu.oracle(c, q.cpu(), False)
    mu.assert_case("mla8-graph-append-decode", out.cpu(), l1.cpu(), ora)


def test_wrapper_picks_the_kernel_by_the_cache():
    """A 16-bit cache through flash_mla_with_kvcache still runs fmha_mla_decode_kernel<...>; the fp8
    cache runs the new kernel with the expected grid and split count."""
    import xf_flash_attention_cutlass_amd as xfa
    L = capi.lib()
    c8, q, causal, _ = problem("bf16", "h128_sq1")
    c16 = mu.make_cache(list(mu.LENS), torch.bfloat16, seed=23)
    qd, lens = q.to(mu.DEV), torch.tensor(c8.lens, dtype=torch.int32, device=mu.DEV)
    b, sq, h, _ = q.shape
    tiles = (sq * h + 15) // 16
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    splits = mu.expected_splits(0, b, tiles, c8.width * c8.page, cus)
    grid = "grid=%dx1x1 block=256" % ((b * splits * tiles + 3) // 4)
    xfa.flash_mla_with_kvcache(qd, c16.kc.to(mu.DEV), c16.table.to(mu.DEV), lens, causal=causal)
    kern = L.fmha_last_kernel().decode()
    assert kern.startswith("fmha_mla_decode_kernel<tiles>") and grid in kern and L.fmha_last_num_splits() == splits
    xfa.flash_mla_with_kvcache(qd, c8.kc.to(mu.DEV), c8.table.to(mu.DEV), lens, causal=causal)
    kern = L.fmha_last_kernel().decode()
    assert kern.startswith("fmha_mla_decode_fp8_kernel<tiles>") and grid in kern and L.fmha_last_num_splits() == splits
    # a byte cache that is not 656 wide is no fp8 latent cache: the 16-bit path refuses its dtype
    with pytest.raises(RuntimeError, match="dtype of q"):
        xfa.flash_mla_with_kvcache(qd, torch.zeros(4, 16, 1, 576, dtype=torch.uint8, device=mu.DEV),
                                   c8.table.to(mu.DEV), lens)
