"""GPU: every forward body on buffers where everything the call does not own holds poison.

Each problem lives inside larger allocations (tests/fwd_own_util.py): rows behind and in front of
every batch, a spare head, a row pitch wider than head_size, rows past seqused_k / cache_seqlens,
rows in front of cache_leftpad, pages and cache batches no sequence owns - all of them zero, NaN or
the dtype's largest value in turn.  Indices, table entries and lengths are always valid: a wrong
read shows as NaN, Inf or a changed bit, never as a fault.  One test runs the three fills of one
problem and requires (fwd_own_util.judge_case): no NaN / Inf in the owned O and LSE (LSE = +inf and
O = 0 exactly on the rows without a key); bits under `nan` and `big` equal to those under `zero`;
every element of the o arena outside the view and of the LSE guards, and the q / k / v arenas,
unchanged; the entry's own parity rule against the oracle over the owned data; the kernel name,
body= field and split count the case names.  tests/test_fwd_own_util.py shows on the CPU that these
conditions reject six planted defects and counts the bodies the table names.

  A  fmha_fwd_kernel through fmha_fwd_strided / fmha_fwd_sink: every (NW, MASK, FEAT, sink)
     instantiation of every bucket, both dtypes, bucket-wide and narrower head sizes, fwd_pipe x masks
  B  the generated D = 128 bodies (plain, full, 16x16, paged; the 4-wave one of the variants build),
     dense and packed
  C  packed sequences with seqused_k on fmha_fwd_kernel; each sequence alone gives the same bits
  D  prefill over a cache: one page per sequence with and without cache_leftpad, paged, fp8; the
     Python wrapper with cache_batch_idx
  E  fmha_varlen_fwd_fp8 with seqused_k on the 4-wave and the 8-wave kernel
  F  split-KV: the stream's scratch primed by a launch of the same geometry with NaN values and a
     far larger LSE, against the same call primed by an all-zero launch
"""
import os

import pytest
import torch

from tests import fwd_own_util as fu
from tests import sink_ref as sr

pytestmark = pytest.mark.gpu
DEV = "cuda"
_VAR = {}


def _ids(cases):
    return [fu.case_id(c) for c in cases]


def _lib_for(c):
    """None (the product library), or the variants build for the cases that name one of its kernels
    (loaded as tests/test_kernel_variants_gpu.py loads it; skipped where it is not built)"""
    if "variants" not in c.extra:
        return None
    from xf_flash_attention_cutlass_amd import capi
    if not os.path.exists(capi.VARIANTS_PATH):
        pytest.skip("the variants library is not built")
    if "lib" not in _VAR:
        _VAR["lib"] = capi.load(capi.VARIANTS_PATH)
    return _VAR["lib"]


def _ready(c):
    L = _lib_for(c)
    reason = fu.session_skip(c, L)
    if reason:
        pytest.skip(reason)
    return L


@pytest.mark.parametrize("c", fu.CASES, ids=_ids(fu.CASES))
def test_case(c, parity_report):
    L = _ready(c)
    fu.check_case(c, lambda p: fu.launch(p, L), parity_report)


@pytest.mark.parametrize("c", fu.ISOLATION, ids=_ids(fu.ISOLATION))
def test_isolation(c):
    """each packed sequence run alone, with the same max_seqlen arguments, gives the bits it has
    inside the batch"""
    L = _ready(c)
    p = fu.build(c, "nan")
    out = fu.launch(p, L)
    assert fu.name_ok(c, out.kern, out.splits), out.kern
    o, lse = fu.view(p.o, out.o)[0], fu.view(p.lse, out.lse)[0]
    for i, sl in enumerate(sr.seq_slices(fu.LQ)):
        if fu.LQ[i] == 0:
            continue
        pi = fu.build(c, "nan", only=i)
        oi = fu.launch(pi, L)
        assert fu.name_ok(c, oi.kern, oi.splits), oi.kern
        assert torch.equal(fu._bits(fu.view(pi.o, oi.o)[0]), fu._bits(o[sl])), f"O of sequence {i}"
        assert torch.equal(fu._bits(fu.view(pi.lse, oi.lse)[0]), fu._bits(lse[:, sl])), f"LSE of sequence {i}"


def _primer(c, kind):
    """a launch of the case's geometry that leaves the split scratch all zero, or full of NaN
    partials under an LSE far above the real one (q x 8, V = NaN)"""
    p = fu.build(c, "zero")
    if kind == "zero":
        for a in (p.q, p.k, p.v):
            fu.view(a).zero_()
    else:
        fu.view(p.q).mul_(8.0)
        fu.view(p.v).fill_(float("nan"))
    return p


@pytest.mark.parametrize("c", fu.SPLIT_CASES, ids=_ids(fu.SPLIT_CASES))
def test_split_scratch(c, parity_report):
    """every partial the combine reads was written by this launch: the pool is one block per
    stream, reused by every call"""
    _ready(c)

    def primed(kind):
        def run(p):
            if p.fill == "nan":                        # (the other two fills: the scratch as it lies)
                fu.launch(_primer(c, kind))
            return fu.launch(p)
        return run

    outs = fu.check_case(c, primed("nan"), parity_report)
    ref = primed("zero")(fu.build(c, "nan"))
    assert fu.name_ok(c, ref.kern, ref.splits), ref.kern
    assert torch.equal(fu._bits(ref.o), fu._bits(outs["nan"].o))
    assert torch.equal(fu._bits(ref.lse), fu._bits(outs["nan"].lse))


def test_wrapper_cache_batch_idx(parity_report):
    """flash_attn_with_kvcache over a dense cache of five batches of which cache_batch_idx names two:
    the other three, and the rows past cache_seqlens, hold the fill"""
    import xf_flash_attention_cutlass_amd as xfa
    from tests import decode_util as du
    from xf_flash_attention_cutlass_amd import capi
    d, hk, sq, cap, dtype = 64, 2, 33, 272, torch.bfloat16
    lens, idx = [200, 77], [3, 1]
    ks, vs = du.make_kv(lens, hk, d, 400)
    q = du.make_q(2, sq, fu.H, d, dtype, 401)
    res = {}
    for fill in fu.FILLS:
        kc = du._fill_pool((5, cap, hk, d), False, dtype, fill)
        vc = du._fill_pool((5, cap, hk, d), False, dtype, fill)
        for i, (n, j) in enumerate(zip(lens, idx)):
            kc[j, :n], vc[j, :n] = ks[i].to(dtype), vs[i].to(dtype)
        kd, vd = kc.to(DEV), vc.to(DEV)
        out, lse = xfa.flash_attn_with_kvcache(
            q.to(DEV), kd, vd, cache_seqlens=torch.tensor(lens, dtype=torch.int32, device=DEV),
            cache_batch_idx=torch.tensor(idx, dtype=torch.int32, device=DEV), causal=True,
            return_softmax_lse=True)
        torch.cuda.synchronize()
        kern = capi.lib().fmha_last_kernel().decode()
        assert kern.startswith("fmha_fwd_kernel<"), kern            # prefill, not the decode kernel
        assert torch.equal(fu._bits(kd.cpu()), fu._bits(kc)) and torch.equal(fu._bits(vd.cpu()), fu._bits(vc))
        res[fill] = (out.cpu(), lse.cpu())
        assert torch.isfinite(res[fill][0].float()).all() and torch.isfinite(res[fill][1]).all(), fill
    for fill in ("nan", "big"):
        assert torch.equal(fu._bits(res[fill][0]), fu._bits(res["zero"][0])), fill
        assert torch.equal(fu._bits(res[fill][1]), fu._bits(res["zero"][1])), fill
    o, lse = res["nan"]
    for i, n in enumerate(lens):
        ref, pt, lref = fu._dense_refs(q[i:i + 1], ks[i].to(dtype)[None], vs[i].to(dtype)[None], (-1, 0), 0.0,
                                       None, None)
        ok, err, bound = fu.orc.parity_ok(o[i:i + 1], ref, pt, 3.0, 1e-5)
        lerr = ((lse[i:i + 1] - lref).abs() - fu.LSE_RTOL * lref.abs()).max().item()
        print(f"D-wrapper-cache_batch_idx seq{i}: err {err:.3e} bound {bound:.3e}; lse err {lerr:.3e}")
        parity_report(dict(case=f"D-wrapper-cache_batch_idx-seq{i}", group="D", metric="o", err=err,
                           bound=bound, kernel=kern.split(" persistent=")[0], ok=bool(ok)))
        assert ok and lerr <= fu.LSE_ATOL, (err, bound, lerr)
