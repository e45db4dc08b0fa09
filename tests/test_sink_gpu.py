"""GPU: the attention-sink forward (fmha_fwd_sink, fmha_varlen_fwd_sink, fmha_page_kvcache_fwd_sink)
through the C ABI, one group of cases per mechanism: the epilogue of the
compiler-scheduled kernel, the post-pass behind the generated D = 128 bodies and the folded decode
merge, and the split combines (split-KV prefill, the decode kernel).  Every case asserts the
kernel that ran and the ` sink=` tag of fmha_last_kernel().

The reference is tests/sink_ref.py (float64 explicit form; the low-precision estimate in the
input dtype).  Rules: forward / varlen max|O - ref| <= 2 max|pt - ref|, kvcache 3 x + 1e-5, LSE
within 1e-3 of float64; `sink=pass` launches get + eps / 2 max|ref|, since O is rounded to the
dtype a second time there and that is the most a second rounding to nearest adds."""
import ctypes
import itertools

import pytest
import torch

from tests import decode_util as du
from tests import sink_ref as sr
from xf_flash_attention_cutlass_amd import capi

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, FP = torch.bfloat16, torch.float16
MASKS = {"noncausal": dict(), "causal": dict(causal=True), "window4_0": dict(window=(4, 0)),
         "causal_softcap30": dict(causal=True, softcap=30.0)}


def _windows(causal=False, window=(-1, -1), softcap=0.0):
    return (int(window[0]), 0) if causal else (int(window[0]), int(window[1]))


def _qkv(b, sq, sk, h, hk, d, dtype, seed, q_mul=1.0):
    g = torch.Generator().manual_seed(seed)
    q = (torch.randn(b, sq, h, d, generator=g) * q_mul).to(dtype)
    k = torch.randn(b, sk, hk, d, generator=g).to(dtype)
    v = torch.randn(b, sk, hk, d, generator=g).to(dtype)
    return q, k, v


class knobs:
    """fmha_set_option for the block, the old values restored afterwards."""

    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        L = capi.lib()
        self.old = {n: L.fmha_get_option(n.encode()) for n in self.kv}
        try:
            for n, v in self.kv.items():
                assert L.fmha_set_option(n.encode(), v) == 0, n
        except BaseException:
            self.__exit__()
            raise

    def __exit__(self, *exc):
        for n, v in self.old.items():
            capi.lib().fmha_set_option(n.encode(), v)


def _strides(*ts):
    return (ctypes.c_int64 * 12)(*[s for t in ts for s in t.stride()[:3]])


def run_dense(q, k, v, sink, num_splits=1, want_lse=True, o=None, mask=None):
    """fmha_fwd_sink (sink None: fmha_fwd_strided, the base entry) on device copies; `o`: a
    device view to write into.  Returns (o, lse, kernel, splits), o / lse still on the device."""
    L = capi.lib()
    mask = mask or {}
    b, sq, h, d = q.shape
    sk, hk = k.shape[1], k.shape[2]
    wl, wr = _windows(**mask)
    qd, kd, vd = (x.to(DEV) for x in (q, k, v))
    if o is None:
        o = torch.full_like(qd, float("nan"))
    lse = torch.full((b, h, sq), float("nan"), dtype=torch.float32, device=DEV) if want_lse else None
    args = [qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), o.data_ptr(), None, capi.ptr(lse), sq, sk, b,
            h, hk, d, _strides(qd, kd, vd, o), d ** -0.5, wl, wr, mask.get("softcap", 0.0),
            q.dtype == FP, num_splits, capi.stream_handle(), 0.0, None]
    if sink is None:
        L.fmha_fwd_strided(*args)
    else:
        sd = sink.to(DEV)
        L.fmha_fwd_sink(*args, sd.data_ptr())
    capi.check()
    torch.cuda.synchronize()
    return o, lse, L.fmha_last_kernel().decode(), L.fmha_last_num_splits()


def run_varlen(q, k, v, sink, lens_q, lens_k, used_k=None, mask=None):
    """fmha_varlen_fwd_sink (sink None: fmha_varlen_fwd_ex) over packed q [total_q, h, d]."""
    L = capi.lib()
    mask = mask or {}
    tq, h, d = q.shape
    hk = k.shape[1]
    wl, wr = _windows(**mask)
    cu = lambda lens: torch.tensor([0] + list(itertools.accumulate(lens)), dtype=torch.int32).to(DEV)
    cu_q, cu_k = cu(lens_q), cu(lens_k)
    used = torch.tensor(used_k, dtype=torch.int32).to(DEV) if used_k is not None else None
    qd, kd, vd = (x.to(DEV) for x in (q, k, v))
    o = torch.full_like(qd, float("nan"))
    lse = torch.full((h, tq), float("nan"), dtype=torch.float32, device=DEV)
    args = [qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), o.data_ptr(), lse.data_ptr(), cu_q.data_ptr(),
            cu_k.data_ptr(), capi.ptr(used), None, 0, 0, None, 0, max(lens_q), max(lens_k), tq,
            len(lens_q), h, hk, d, d ** -0.5, wl, wr, mask.get("softcap", 0.0), q.dtype == FP,
            capi.stream_handle(), 0.0, None]
    if sink is None:
        L.fmha_varlen_fwd_ex(*args)
    else:
        sd = sink.to(DEV)
        L.fmha_varlen_fwd_sink(*args, sd.data_ptr())
    capi.check()
    torch.cuda.synchronize()
    return o, lse, L.fmha_last_kernel().decode()


def run_paged(c: du.Cache, q, sink, num_splits, mask=None):
    """fmha_page_kvcache_fwd_sink (sink None: fmha_page_kvcache_fwd_ex) on a device copy of the
    cache, into NaN-filled outputs."""
    L = capi.lib()
    mask = mask or {}
    b, sq, h, d = q.shape
    hk = c.kc.shape[2]
    wl, wr = _windows(**mask)
    qd, kc, vc, tab = q.to(DEV), c.kc.to(DEV), c.vc.to(DEV), c.table.to(DEV)
    lens = torch.tensor(c.lens, dtype=torch.int32).to(DEV)
    o = torch.full_like(qd, float("nan"))
    lse = torch.full((b, h, sq), float("nan"), dtype=torch.float32, device=DEV)
    args = [qd.data_ptr(), kc.data_ptr(), vc.data_ptr(), o.data_ptr(), lse.data_ptr(), tab.data_ptr(),
            tab.stride(0), lens.data_ptr(), sq, c.width * c.page, b, h, hk, d, c.page, d ** -0.5, wl,
            wr, 0.0, None, 0, num_splits, 1 if c.fp8 else 0, c.k_scale, c.v_scale, None,
            q.dtype == FP, capi.stream_handle()]
    if sink is None:
        L.fmha_page_kvcache_fwd_ex(*args)
    else:
        sd = sink.to(DEV)
        L.fmha_page_kvcache_fwd_sink(*args, sd.data_ptr())
    capi.check()
    torch.cuda.synchronize()
    return o, lse, L.fmha_last_kernel().decode(), L.fmha_last_num_splits()


def paged_refs(c: du.Cache, q, sink, mask=None) -> sr.FwdRefs:
    """Per sequence over the exact cache values (float32(stored) x scale); pt over the cache
    rounded to q's dtype.  A sequence without keys: O = 0, LSE = +inf."""
    mask = mask or {}
    outs, lses, pts = [], [], []
    for i in range(q.shape[0]):
        qi, kx, vx = q[i:i + 1], c.kx[i][None], c.vx[i][None]
        o64, l64 = sr.sink_attention(qi.double(), kx.double(), vx.double(), sink.double(), **mask)
        pt, _ = sr.sink_attention(qi, kx.to(q.dtype), vx.to(q.dtype), sink.to(q.dtype),
                                  reorder_ops=True, **mask)
        outs.append(o64)
        lses.append(l64)
        pts.append(pt)
    return sr.FwdRefs(torch.cat(outs), torch.cat(lses), torch.cat(pts))


def _tagged(kern, name, tag):
    assert kern.startswith(name + " ") and kern.endswith(" sink=" + tag), f"ran {kern!r}, wanted {name} .. sink={tag}"


# ---------------------------------------------------------------- epilogue ----------------
@pytest.mark.parametrize("dtype", [BF, FP], ids=["bf16", "fp16"])
@pytest.mark.parametrize("mask", list(MASKS))
@pytest.mark.parametrize("d", [64, 40])
def test_epilogue(parity_report, d, mask, dtype):
    q, k, v = _qkv(2, 130, 130, 8, 2, d, dtype, 11 + d)
    sink = sr.sink_values(8)
    o, lse, kern, _ = run_dense(q, k, v, sink, mask=MASKS[mask])
    _tagged(kern, "fmha_fwd_kernel<8 waves>", "epilogue")
    sr.check_fwd(f"sink epilogue d{d} {mask} {dtype}", o, lse, sr.fwd_refs(q, k, v, sink, **MASKS[mask]),
                 dtype, parity_report)


def test_epilogue_causal_fewer_queries_than_keys(parity_report):
    q, k, v = _qkv(2, 70, 130, 8, 2, 64, BF, 21)
    sink = sr.sink_values(8)
    o, lse, kern, _ = run_dense(q, k, v, sink, mask=dict(causal=True))
    _tagged(kern, "fmha_fwd_kernel<8 waves>", "epilogue")
    sr.check_fwd("sink epilogue causal sq70 sk130", o, lse, sr.fwd_refs(q, k, v, sink, causal=True), BF,
                 parity_report)


def test_epilogue_varlen_with_an_empty_sequence(parity_report):
    lens_q, lens_k, used = (1, 33, 130, 5), (1, 33, 130, 7), (1, 33, 130, 0)
    q, k, v = _qkv(1, sum(lens_q), sum(lens_k), 8, 2, 64, BF, 22)
    q, k, v = q[0], k[0], v[0]
    sink = sr.sink_values(8)
    o, lse, kern = run_varlen(q, k, v, sink, lens_q, lens_k, used, mask=dict(causal=True))
    _tagged(kern, "fmha_fwd_kernel<8 waves>", "epilogue")
    refs = sr.fwd_refs_varlen(q, k, v, sink, lens_q, lens_k, used, causal=True)
    sr.check_fwd("sink epilogue varlen seqused_k", o, lse, refs, BF, parity_report)
    last = slice(sum(lens_q) - 5, None)                      # the sequence without keys
    assert not o[last].float().abs().sum().item() > 0 and bool((lse[:, last] == float("inf")).all())


# ---------------------------------------------------------------- post-pass ---------------
@pytest.mark.parametrize("dtype", [BF, FP], ids=["bf16", "fp16"])
@pytest.mark.parametrize("causal,kernel", [(True, "fmha_fwdpp_kernel"), (False, "fmha_fwdpp16_kernel")])
def test_pass_generated_bodies(parity_report, causal, kernel, dtype):
    q, k, v = _qkv(2, 300, 300, 4, 2, 128, dtype, 31)
    sink = sr.sink_values(4)
    mask = dict(causal=True) if causal else {}
    o, lse, kern, _ = run_dense(q, k, v, sink, mask=mask)
    _tagged(kern, kernel, "pass")
    sr.check_fwd(f"sink pass {kernel} {dtype}", o, lse, sr.fwd_refs(q, k, v, sink, **mask), dtype,
                 parity_report, second_rounding=True)


def test_pass_varlen(parity_report):
    lens = (1, 70, 257)
    q, k, v = _qkv(1, sum(lens), sum(lens), 4, 2, 128, BF, 32)
    q, k, v = q[0], k[0], v[0]
    sink = sr.sink_values(4)
    o, lse, kern = run_varlen(q, k, v, sink, lens, lens, mask=dict(causal=True))
    _tagged(kern, "fmha_fwdpp_kernel", "pass")
    assert lse.shape == (4, sum(lens))
    sr.check_fwd("sink pass varlen", o, lse, sr.fwd_refs_varlen(q, k, v, sink, lens, lens, causal=True),
                 BF, parity_report, second_rounding=True)


def test_pass_paged_prefill(parity_report):
    lens = [300, 131, 70]
    ks, vs = du.make_kv(lens, 2, 128, 33)
    c = du.build_cache(ks, vs, 16, 320 // 16, False, BF, "nan", seed=33)
    q = du.make_q(3, 70, 4, 128, BF, 33)
    sink = sr.sink_values(4)
    o, lse, kern, _ = run_paged(c, q, sink, 1, mask=dict(causal=True))
    _tagged(kern, "fmha_fwdpp_paged_kernel", "pass")
    sr.check_fwd("sink pass paged prefill", o, lse, paged_refs(c, q, sink, dict(causal=True)), BF,
                 parity_report, mult=3.0, atol=1e-5, second_rounding=True)


def test_pass_strided_view_and_null_lse():
    """O as a head-sliced view inside an arena of 0x55 bytes: the pass walks the call's own O
    strides, so every byte outside the view is unchanged and the view equals the contiguous
    run's O; with softmax_lse = NULL the pass reads the LSE from pool scratch: the same O."""
    q, k, v = _qkv(2, 300, 300, 4, 2, 128, BF, 34)
    sink = sr.sink_values(4)
    o_ref, _, kern, _ = run_dense(q, k, v, sink, mask=dict(causal=True))
    _tagged(kern, "fmha_fwdpp_kernel", "pass")
    arena = torch.full((2, 300, 8, 128), 0, dtype=BF, device=DEV)
    arena.view(torch.uint8).fill_(0x55)
    view = arena[:, :, 2:6]
    o, _, kern, _ = run_dense(q, k, v, sink, mask=dict(causal=True), o=view)
    _tagged(kern, "fmha_fwdpp_kernel", "pass")
    assert torch.equal(view.view(torch.int16), o_ref.view(torch.int16))
    outside = torch.ones(2, 300, 8, 128, dtype=torch.bool, device=DEV)
    outside[:, :, 2:6] = False
    assert bool((arena.view(torch.int16)[outside] == 0x5555).all())
    o_nolse, lse_none, kern, _ = run_dense(q, k, v, sink, mask=dict(causal=True), want_lse=False)
    _tagged(kern, "fmha_fwdpp_kernel", "pass")
    assert lse_none is None and torch.equal(o_nolse.view(torch.int16), o_ref.view(torch.int16))


# ---------------------------------------------------------------- combine -----------------
@pytest.mark.parametrize("comb_row", [0, 1])
@pytest.mark.parametrize("d", [64, 128])
def test_combine_split_prefill(parity_report, d, comb_row):
    q, k, v = _qkv(1, 64, 2048, 4, 2, d, BF, 41 + d)
    sink = sr.sink_values(4)
    with knobs(comb_row=comb_row):
        o, lse, kern, splits = run_dense(q, k, v, sink, num_splits=4)
    _tagged(kern, "fmha_fwd_kernel<8 waves>", "combine")
    assert splits == 4
    sr.check_fwd(f"sink combine split prefill d{d} comb_row{comb_row}", o, lse, sr.fwd_refs(q, k, v, sink),
                 BF, parity_report)


DECODE_LENS = [0, 100, 777]


def _decode_problem(hk, sq, d, fp8, seed=51):
    ks, vs = du.make_kv(DECODE_LENS, hk, d, seed)
    c = du.build_cache(ks, vs, 16, 1024 // 16, fp8, BF, "nan", seed=seed)
    return c, du.make_q(3, sq, 8, d, BF, seed)


@pytest.mark.parametrize("num_splits", [0, 8])
@pytest.mark.parametrize("fp8", [False, True], ids=["kv16", "fp8"])
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("sq", [1, 2])
@pytest.mark.parametrize("hk", [2, 1])
def test_combine_decode(parity_report, hk, sq, d, fp8, num_splits):
    c, q = _decode_problem(hk, sq, d, fp8)
    sink = sr.sink_values(8)
    mask = dict(causal=True) if sq > 1 else {}
    with knobs(dec_fold=0):
        o, lse, kern, splits = run_paged(c, q, sink, num_splits, mask=mask)
    _tagged(kern, "fmha_decode_kernel<16 rows>", "combine")
    assert splits >= 4
    sr.check_fwd(f"sink combine decode hk{hk} sq{sq} d{d} fp8={fp8} splits{num_splits}", o, lse,
                 paged_refs(c, q, sink, mask), BF, parity_report, mult=3.0, atol=1e-5)


def test_decode_folded_merge_takes_the_pass(parity_report):
    c, q = _decode_problem(2, 1, 128, False)
    sink = sr.sink_values(8)
    with knobs(dec_fold=1):
        o, lse, kern, _ = run_paged(c, q, sink, 8)
    _tagged(kern, "fmha_decode_kernel<16 rows>", "pass")
    sr.check_fwd("sink pass decode dec_fold", o, lse, paged_refs(c, q, sink), BF, parity_report,
                 mult=3.0, atol=1e-5, second_rounding=True)


# ---------------------------------------------------------------- exactness ---------------
def _mechanism_case(mech, q_mul=1.0, seed=61):
    """(runner(sink) -> (o, lse, kernel), heads) of one case per mechanism; q_mul scales q."""
    if mech == "epilogue":
        q, k, v = _qkv(2, 130, 130, 8, 2, 64, BF, seed, q_mul)
        return (lambda s: run_dense(q, k, v, s, mask=dict(causal=True))[:3]), 8, (q, k, v)
    if mech == "pass":
        q, k, v = _qkv(2, 300, 300, 4, 2, 128, BF, seed, q_mul)
        return (lambda s: run_dense(q, k, v, s, mask=dict(causal=True))[:3]), 4, (q, k, v)
    q, k, v = _qkv(1, 64, 2048, 4, 2, 64, BF, seed, q_mul)
    return (lambda s: run_dense(q, k, v, s, num_splits=4)[:3]), 4, (q, k, v)


@pytest.mark.parametrize("mech", ["epilogue", "pass", "combine"])
def test_minus_inf_sink_is_the_base_entry_bit_for_bit(mech):
    run, h, _ = _mechanism_case(mech)
    o0, l0, kern0 = run(None)
    o, lse, kern = run(torch.full((h,), float("-inf")))
    assert kern == kern0 + " sink=" + mech
    assert torch.equal(o.view(torch.int16), o0.view(torch.int16))
    assert torch.equal(lse.view(torch.int32), l0.view(torch.int32))


@pytest.mark.parametrize("mech", ["epilogue", "pass", "combine"])
def test_large_sink_against_very_negative_scores(mech):
    """Scores near -50 (k near a fixed vector w, q = -50 w / (|w|^2 scale)) and sink = +40: the
    sink takes all the mass.  exp2(s log2e - m) against the running max would overflow fp32 here
    (e^90); the stable merge gives |O| <= 1e-6 max|O0|, |LSE - 40| <= 1e-3, nothing inf or NaN."""
    run, h, (q, k, v) = _mechanism_case(mech)
    d = q.shape[-1]
    g = torch.Generator().manual_seed(62)
    k.copy_((1.0 + 0.05 * torch.randn(k.shape, generator=g)).to(k.dtype))
    q.copy_((-50.0 / d ** 0.5 + 0.05 * torch.randn(q.shape, generator=g)).to(q.dtype))
    o0, l0, _ = run(None)
    assert bool(torch.isfinite(l0).all()) and -60.0 < l0.mean().item() < -35.0     # the setup itself
    o, lse, kern = run(torch.full((h,), 40.0))
    assert kern.endswith(" sink=" + mech)
    assert bool(torch.isfinite(o.float()).all()) and bool(torch.isfinite(lse).all())
    assert o.float().abs().max().item() <= 1e-6 * o0.float().abs().max().item()
    assert (lse - 40.0).abs().max().item() <= 1e-3


# ---------------------------------------------------------------- the Python interface ----
@pytest.mark.parametrize("fp8", [False, True], ids=["kv16", "fp8"])
def test_python_kvcache_sink_equals_the_c_entry(fp8):
    """flash_attn_with_kvcache(sink=) (a bf16 sink: cast to fp32 for the call) gives the bits of
    fmha_page_kvcache_fwd_sink, over a bf16 and an fp8 paged cache."""
    import xf_flash_attention_cutlass_amd as xfa
    c, q = _decode_problem(2, 1, 128, fp8)
    sink = sr.sink_values(8).to(BF)
    o_c, lse_c, kern, _ = run_paged(c, q, sink.float(), 0)
    _tagged(kern, "fmha_decode_kernel<16 rows>", "combine")
    lens = torch.tensor(c.lens, dtype=torch.int32, device=DEV)
    o, lse = xfa.flash_attn_with_kvcache(q.to(DEV), c.kc.to(DEV), c.vc.to(DEV), cache_seqlens=lens,
                                         block_table=c.table.to(DEV), k_scale=c.k_scale,
                                         v_scale=c.v_scale, return_softmax_lse=True, sink=sink.to(DEV))
    assert capi.lib().fmha_last_kernel().decode().endswith(" sink=combine")
    assert torch.equal(o.view(torch.int16), o_c.view(torch.int16))
    assert torch.equal(lse.view(torch.int32), lse_c.view(torch.int32))
