"""GPU: fmha_mla_decode (MLA decode over a paged latent cache) against the CPU
oracle, per sequence (tests/mla_util.py), on caches behind a permuted block table, poisoned with NaN
outside the sequences, into NaN-filled outputs.  Every case asserts the kernel, its mapping, its
grid and the split count (mla_util.run).

Instances: bf16 / fp16 x {16 heads (one row tile: the waves are key splits), 8 heads x 3 causal
positions (24 rows: a tile straddling positions and a partial tile), 128 heads (8 row tiles),
40 heads x 2 causal positions} x num_splits {1, 3, 0}, over 517, 300, 65, 33, 32, 31, 2, 1 and 0
keys.  Then: large pages, fill independence, a non-default scale, strided views, the three
surfaces, reproducibility, refusals, graph capture and the chunked merge of two partial calls.
"""
import ctypes as C

import pytest
import torch

from tests import mla_util as mu
from xf_flash_attention_cutlass_amd import capi

pytestmark = pytest.mark.gpu

DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
_CACHE, _ORACLE = {}, {}


def cache_of(dt, fill="nan", page=mu.PAGE, lens=None):
    key = (dt, fill, page, tuple(lens or mu.LENS))
    if key not in _CACHE:
        _CACHE[key] = mu.make_cache(list(lens or mu.LENS), DTYPES[dt], fill, seed=23, page=page,
                                    width=1024 // page)
    return _CACHE[key]


def problem(dt, shape, page=mu.PAGE):
    """(cache, q, causal, oracle), computed once and shared (the oracle does not depend on the fill
    or the page size: the sequences' values are the same)."""
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
    o, lse, kern, splits = mu.run(c, q, causal, num_splits)
    mu.assert_case(f"mla-{dt}-{shape}-splits{num_splits}", o.cpu(), lse.cpu(), ora, parity_report)


@pytest.mark.parametrize("num_splits", [1, 0])
def test_page_64(num_splits, parity_report):
    """A 64-row page holds two tiles; its halves 16 rows on are rows of the same page."""
    c, q, causal, ora = problem("bf16", "h8_sq3_causal", page=64)
    assert torch.equal(c.kx[0], cache_of("bf16").kx[0])
    o, lse, _, _ = mu.run(c, q, causal, num_splits)
    mu.assert_case(f"mla-page64-splits{num_splits}", o.cpu(), lse.cpu(), ora, parity_report)


def test_page_16_tile_straddles_pages(parity_report):
    """Page 16: every 32-key tile is two pages, which the permuted table puts apart."""
    c, q, causal, ora = problem("fp16", "h16_sq1")
    tab = c.table[0, :(517 + 15) // 16].long()
    assert ((tab[1::2] - tab[0:-1:2]) != 1).any()
    o, lse, _, _ = mu.run(c, q, causal, 3)
    mu.assert_case("mla-page16-straddle", o.cpu(), lse.cpu(), ora, parity_report)


@pytest.mark.parametrize("shape,num_splits", [("h8_sq3_causal", 1), ("h16_sq1", 0)])
def test_fill_independence(shape, num_splits):
    """What lies outside the sequences (rows past their ends, the pages no entry names, the poison
    page the table's tail points at) does not reach the outputs: zero-, NaN- and max-filled caches
    give the same bits."""
    h, sq, causal = mu.SHAPES[shape]
    q = mu.make_q(len(mu.LENS), sq, h, mu.D, torch.bfloat16, 23)
    got = []
    for fill in ("zero", "nan", "big"):
        o, lse, _, _ = mu.run(cache_of("bf16", fill), q, causal, num_splits)
        got.append((o.cpu(), lse.cpu()))
        assert not torch.isnan(got[-1][0]).any() and not torch.isnan(got[-1][1]).any()
    for o, lse in got[1:]:
        assert torch.equal(o, got[0][0]) and torch.equal(lse, got[0][1])


def test_scale(parity_report):
    """softmax_scale = 2 x 576^-1/2 against the oracle over 2 q (exact in bf16)."""
    c, q, causal, _ = problem("bf16", "h16_sq1")
    ora = mu.oracle(c, q, causal, q_mul=2.0)
    o, lse, _, _ = mu.run(c, q, causal, 3, scale=2.0 * mu.D ** -0.5)
    mu.assert_case("mla-scale2", o.cpu(), lse.cpu(), ora, parity_report)


def test_strided_views(parity_report):
    """q and o as views inside NaN-poisoned arenas (row and head strides larger than the dense
    ones, a storage offset): the arena is untouched outside o."""
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
        o, lse, _, _ = mu.run(c, q, causal, ns, o=ov, qd=qv)
        mu.assert_case(f"mla-strided-splits{ns}", ov.cpu(), lse.cpu(), ora, parity_report)
        inside = torch.zeros_like(oa, dtype=torch.bool)
        inside[:, 1:sq + 1, :h, 64:64 + mu.DV] = True
        assert torch.isnan(oa[~inside]).all()
    assert torch.isnan(qa[:, 0]).all()


def test_surfaces_bitwise_equal_and_reproducible():
    """The C ABI, the pybind op and the Python wrapper give the same bits, and so do two calls."""
    import xf_flash_attention_cutlass_amd as xfa
    c, q, causal, _ = problem("fp16", "h40_sq2_causal")
    kc, tab = c.kc.to(mu.DEV), c.table.to(mu.DEV)
    lens = torch.tensor(c.lens, dtype=torch.int32, device=mu.DEV)
    qd = q.to(mu.DEV)
    for ns in (1, 0):
        o0, l0, _, splits = mu.run(c, q, causal, ns)
        o1, l1, _, _ = mu.run(c, q, causal, ns)
        assert torch.equal(o0, o1) and torch.equal(l0, l1)
        o2, l2 = xfa.paged_attn.mla_decode(qd, kc, tab, lens, 512, mu.D ** -0.5, causal, ns, None)
        assert capi.lib().fmha_last_num_splits() == splits
        o3, l3 = xfa.flash_mla_with_kvcache(qd, kc, tab, lens, causal=causal, num_splits=ns)
        out = torch.full_like(o0, float("nan"))
        o4, l4 = xfa.flash_mla_with_kvcache(qd, kc, tab, lens, causal=causal, num_splits=ns, out=out)
        assert o4 is out
        for o, l in ((o2, l2), (o3, l3), (o4, l4)):
            assert torch.equal(o, o0) and torch.equal(l, l0)


def test_no_lse_pointer():
    c, q, causal, _ = problem("bf16", "h16_sq1")
    for ns in (1, 3):
        o0, _, _, _ = mu.run(c, q, causal, ns)
        o1, lse, _, _ = mu.run(c, q, causal, ns, want_lse=False)
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

    def call(d=mu.D, dv=mu.DV, page=c.page, window=(-1, -1), splits=0, table=tab.data_ptr(), strides=dense):
        st = (C.c_int64 * 6)(*strides)
        L.fmha_mla_decode(qd.data_ptr(), kc.data_ptr(), o.data_ptr(), lse.data_ptr(), table, tab.stride(0),
                          lens.data_ptr(), sq, c.width * c.page, b, h, d, dv, page, st, mu.D ** -0.5,
                          window[0], window[1], splits, False, capi.stream_handle())
        return L.fmha_last_status(), L.fmha_last_error().decode()

    for kw, needle in ((dict(d=512), "(576, 512) only"), (dict(page=24), "multiple of 16"),
                       (dict(window=(64, 0)), "(-1, -1) and (-1, 0)"), (dict(splits=129), "at most 128"),
                       (dict(table=None), "block_table"),
                       (dict(strides=dense[:5] + [516]), "multiples of 8")):
        st, msg = call(**kw)
        torch.cuda.synchronize()
        assert st != 0 and needle in msg, msg
        assert L.fmha_last_kernel() == b"" and L.fmha_last_num_splits() == 0
        assert torch.isnan(o).all() and torch.isnan(lse).all()
    st, msg = call()
    torch.cuda.synchronize()
    assert st == 0 and not torch.isnan(o).any()


def test_graph_capture():
    """One capture and replay after a warm-up call (the scratch pool is warm: no allocation and no
    host sync inside the capture)."""
    import xf_flash_attention_cutlass_amd as xfa
    c, q, causal, _ = problem("bf16", "h128_sq1")
    kc, tab = c.kc.to(mu.DEV), c.table.to(mu.DEV)
    lens = torch.tensor(c.lens, dtype=torch.int32, device=mu.DEV)
    qd = q.to(mu.DEV)
    out = torch.full((*q.shape[:3], mu.DV), float("nan"), dtype=q.dtype, device=mu.DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        o0, l0 = xfa.flash_mla_with_kvcache(qd, kc, tab, lens, out=out)     # warm-up on the capture stream
        want_o, want_l = o0.clone(), l0.clone()
        splits = capi.lib().fmha_last_num_splits()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert splits > 1
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        _, l1 = xfa.flash_mla_with_kvcache(qd, kc, tab, lens, out=out)
    out.fill_(float("nan"))
    l1.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want_o) and torch.equal(l1, want_l)


def test_chunked_merge(parity_report):
    """A prefix part and a suffix part over two block tables (both full attention), merged by
    merge_attn_states as two 256-column halves through the strides, equal the single call's
    oracle (fmha_merge_states stays limited to head size 256)."""
    import xf_flash_attention_cutlass_amd as xfa
    dt = torch.bfloat16
    lens = [517, 300, 65, 33]
    cut = [256, 299, 1, 33]                          # suffixes of 261, 1, 64 and 0 keys
    full = cache_of("bf16", lens=lens)
    h, sq = 16, 2
    q = mu.make_q(len(lens), sq, h, mu.D, dt, 29)
    ora = mu.oracle(full, q, False)
    gen = torch.Generator().manual_seed(0)
    parts = []
    for rng in ([(0, n) for n in cut], [(n, m) for n, m in zip(cut, lens)]):
        ks = [full.kx[i][a:b] for i, (a, b) in enumerate(rng)]
        pc = mu.build_cache(ks, ks, mu.PAGE, mu.WIDTH, False, dt, "nan", seed=int(torch.randint(99, (1,), generator=gen)))
        o, lse, _, _ = mu.run(pc, q, False, 3)
        parts.append((o, lse))
    out = torch.full_like(parts[0][0], float("nan"))
    lse_out = None
    for lo in (0, 256):
        _, lse_out = xfa.merge_attn_states([p[0][..., lo:lo + 256] for p in parts], [p[1] for p in parts],
                                           out=out[..., lo:lo + 256])
    mu.assert_case("mla-chunked-merge", out.cpu(), lse_out.cpu(), ora, parity_report)
