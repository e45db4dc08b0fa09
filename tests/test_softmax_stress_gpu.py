"""GPU: every rescale path of the forward softmax, off the unit-randn regime.

The forward kernels exponentiate against a reference max that may lag the true max by `fwd_slack`
log2 units and catch up in a rare branch.  Unit randn never enters it at the default
slack, so these cases scale the keys (tests/softmax_stress_util.py: growing, late_step, descending,
mixed_rows) and run at fwd_slack 0, 8 and 16.  tests/test_softmax_stress_util.py shows on the CPU
that each case's inputs force the branch and that the rules below reject a kernel that gets it
wrong.

  A  fmha_fwd_kernel, every head-size bucket but the D = 128 ping-pong one, masks x patterns x slack,
     fwd_pipe 0 / 1 / 2
  B  the same kernel with ALiBi, softcap, both; packed sequences; dropout; a leftpad cache
  C  split-KV and both combines, with and without a sink
  D  the D = 128 ping-pong kernels: left windows, ALiBi, softcap, no right window, paged K/V
  E  sinks, one case per mechanism
  F  fp8 forward: the 4-wave kernel and the 8-wave one, dense and packed
  G  decode, bf16 and fp8 caches, with and without the folded combine

Every case makes its inputs on the CPU, writes into NaN-filled buffers, asserts the kernel that ran
(and the split count where it forces one) and feeds `parity_report`.  Knobs are set through
`_option` only and restored.  Rules (the project's): O finite and within 2 x the low-precision
estimate's error (fp8: 3 x + 1e-3; decode: decode_util.judge); without softcap, dropout and fp8
also within the a priori bound u (max|v| + max|ref|) 1.05; LSE within 1e-3 + 1e-5 |ref| with the
same +inf rows.
"""
import ctypes
import itertools
from contextlib import ExitStack

import pytest
import torch

from oracle import attention_ref as orc
from tests import decode_util as du
from tests import sink_ref as sr
from tests import softmax_stress_util as su
from tests.fp8_model import attention_fp8_kernel_model
from tests.softmax_stress_util import BF, FP, _option

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")


def _capi():
    from xf_flash_attention_cutlass_amd import capi
    return capi


def _knobs(stack, slack, knobs=()):
    stack.enter_context(_option("fwd_slack", slack))
    for n, v in knobs:
        stack.enter_context(_option(n, v))


def _session(name):
    return _capi().lib().fmha_get_option(name.encode())


def _need(name, value, knobs=()):
    """skip when the session's knob (XFA_TEST_OPTIONS) sends the launch to another kernel"""
    if name not in dict(knobs) and _session(name) != value:
        pytest.skip(f"the kernel this case asserts needs {name} = {value}; the session runs "
                    f"{name} = {_session(name)}")


def _strides(*ts):
    return (ctypes.c_int64 * 12)(*[s for t in ts for s in t.stride()[:3]])


def run_dense(q, k, v, window, num_splits=1, slopes=None, softcap=0.0, sink=None):
    """fmha_fwd_sink (sink None: fmha_fwd_strided): (o, lse) on the CPU, the kernel, the splits"""
    capi = _capi()
    L = capi.lib()
    b, sq, h, d = q.shape
    sk, hk = k.shape[1], k.shape[2]
    qd, kd, vd = (x.to(DEV) for x in (q, k, v))
    o = torch.full_like(qd, NAN)
    lse = torch.full((b, h, sq), NAN, dtype=torch.float32, device=DEV)
    sl = slopes.to(DEV).contiguous() if slopes is not None else None
    args = [qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), o.data_ptr(), capi.ptr(sl), lse.data_ptr(),
            sq, sk, b, h, hk, d, _strides(qd, kd, vd, o), d ** -0.5, window[0], window[1], softcap,
            q.dtype == FP, num_splits, capi.stream_handle(), 0.0, None]
    if sink is None:
        L.fmha_fwd_strided(*args)
    else:
        sd = sink.to(DEV)
        L.fmha_fwd_sink(*args, sd.data_ptr())
    capi.check()
    torch.cuda.synchronize()
    return o.cpu(), lse.cpu(), L.fmha_last_kernel().decode(), L.fmha_last_num_splits()


def run_paged(c: du.Cache, q, window, num_splits=1):
    """fmha_page_kvcache_fwd_ex on a device copy of the cache"""
    capi = _capi()
    L = capi.lib()
    b, sq, h, d = q.shape
    hk = c.kc.shape[2]
    qd, kc, vc, tab = q.to(DEV), c.kc.to(DEV), c.vc.to(DEV), c.table.to(DEV)
    lens = torch.tensor(c.lens, dtype=torch.int32).to(DEV)
    lp = torch.tensor(c.leftpad, dtype=torch.int32).to(DEV) if c.leftpad is not None else None
    o = torch.full_like(qd, NAN)
    lse = torch.full((b, h, sq), NAN, dtype=torch.float32, device=DEV)
    L.fmha_page_kvcache_fwd_ex(
        qd.data_ptr(), kc.data_ptr(), vc.data_ptr(), o.data_ptr(), lse.data_ptr(), tab.data_ptr(),
        tab.stride(0), lens.data_ptr(), sq, c.width * c.page, b, h, hk, d, c.page, d ** -0.5,
        window[0], window[1], 0.0, None, 0, num_splits, 1 if c.fp8 else 0, c.k_scale, c.v_scale,
        capi.ptr(lp), q.dtype == FP, capi.stream_handle())
    capi.check()
    torch.cuda.synchronize()
    return o.cpu(), lse.cpu(), L.fmha_last_kernel().decode(), L.fmha_last_num_splits()


def _kname(kern):
    """the kernel's name without its schedule: the parity rows are counted by it"""
    return kern.split(" persistent=")[0]


def _ran(kern, want):
    assert kern.startswith(want), f"ran {kern!r}, wanted {want}"


def _sink_at_median(lse_ref):
    """per head, the median finite reference LSE: the sink then carries real weight"""
    h = lse_ref.shape[1]
    per = lse_ref.permute(1, 0, 2).reshape(h, -1)
    return torch.stack([x[torch.isfinite(x)].median() for x in per]).float()


def _sink_refs(q, k, v, sink, window, second_rounding):
    causal = window == (-1, 0)
    r = sr.fwd_refs(q, k, v, sink, causal=causal, window=window)
    ap = None if second_rounding else su._rounding_bound(q, k, v, False, ref=r.ref64)
    return su.Refs(r.ref64.float(), r.pt, r.lse64.float(), ap)


# --------------------------------------------------------------- A - E: the dense table --------
def _expect(c: su.Case):
    """(kernel prefix, sink tag or None) a case must run"""
    if c.group == "D" or (c.group == "E" and c.d == 128):
        _need("fwd_w4", 4)
        m16 = c.mask == "full" and not c.feat
        return ("fmha_fwdpp16_kernel " if m16 else "fmha_fwdpp_kernel "), ("pass" if c.feat == "sink" else None)
    if c.d == 128 and c.splits == 1:
        assert ("fwd_w4", 0) in c.knobs
    tag = None
    if "sink" in c.feat:
        tag = "combine" if c.splits > 1 else "epilogue"
    return "fmha_fwd_kernel<", tag


@pytest.mark.parametrize("c", su.CASES, ids=[su.case_id(c) for c in su.CASES])
def test_dense(c, parity_report):
    want, tag = _expect(c)
    q, k, v = su.inputs(c)
    window = su.MASKS[c.mask]
    base = su.case_refs(su.input_key(c))
    sink = _sink_at_median(base.lse) if "sink" in c.feat else None
    with ExitStack() as st:
        _knobs(st, c.slack, c.knobs)
        o, lse, kern, splits = run_dense(q, k, v, window, c.splits, su.slopes_of(c), su.softcap_of(c), sink)
    _ran(kern, want)
    assert splits == c.splits, (splits, kern)
    r, atol = base, 0.0
    if sink is not None:
        assert kern.endswith(" sink=" + tag), kern
        r = _sink_refs(q, k, v, sink, window, tag == "pass")
        if tag == "pass":                      # O rounded a second time (tests/test_sink_gpu.py)
            atol = 0.5 * sr.EPS[c.dtype] * r.ref.abs().max().item()
    su.assert_case(su.case_id(c), o, lse, r, parity_report, atol=atol, extra=dict(kernel=_kname(kern)))


def test_fp16_edge_of_slack(parity_report):
    """fp16 at fwd_slack = 16: one row's P at one key is 2^15.9998 >= 65520 unless the launch keeps
    the effective slack of an fp16 launch at 15 or below (su.fp16_edge_inputs; the CPU twin shows
    that the unclamped arithmetic gives inf there).  d 64: fmha_fwd_kernel's pipeline; d 128 under
    fwd_w4 = 0: the same kernel's other bucket."""
    for d, knobs in ((64, ()), (128, (("fwd_w4", 0),))):
        q, k, v = su.fp16_edge_inputs(d)
        r = su.refs(q, k, v)
        for slack in (16, 15):
            with ExitStack() as st:
                _knobs(st, slack, knobs)
                o, lse, kern, _ = run_dense(q, k, v, (-1, -1))
            _ran(kern, "fmha_fwd_kernel<")
            su.assert_case(f"fp16 edge d{d} s{slack}", o, lse, r, parity_report,
                           extra=dict(kernel=_kname(kern)))


# --------------------------------------------------------------- B: packed, dropout, leftpad ---
@pytest.fixture(scope="module")
def xfa():
    import xf_flash_attention_cutlass_amd as m
    return m


def _cu(lens):
    return torch.tensor([0] + list(itertools.accumulate(lens)), dtype=torch.int32)


VARLEN = [1, 63, 65, 200, 417]


@pytest.mark.parametrize("slack", su.SLACKS)
def test_varlen(xfa, slack, parity_report):
    """flash_attn_varlen_func, d 64, causal, each sequence's keys grown separately"""
    tot = sum(VARLEN)
    q, k, v = (su._randn((tot, hh, 64), 70 + i, BF) for i, hh in enumerate((su.H, su.HK, su.HK)))
    sl = sr.seq_slices(VARLEN)
    k = torch.cat([su._growing(k[s][None], 40.0)[0] for s in sl])
    cu = _cu(VARLEN).to(DEV)
    with _option("fwd_slack", slack):
        out, lse, _ = xfa.flash_attn_varlen_func(q.to(DEV), k.to(DEV), v.to(DEV), cu, cu, max(VARLEN),
                                                 max(VARLEN), causal=True, return_attn_probs=True)
        kern = _capi().lib().fmha_last_kernel().decode()
    torch.cuda.synchronize()
    _ran(kern, "fmha_fwd_kernel<")
    out, lse = out.cpu(), lse.cpu()
    for i, s in enumerate(sl):
        qs, ks, vs = q[s][None], k[s][None], v[s][None]
        su.assert_case(f"B-varlen-d64-growing40-s{slack}-seq{i}", out[s][None], lse[:, s][None],
                       su.refs(qs, ks, vs, (-1, 0)), parity_report, extra=dict(kernel=_kname(kern)))


@pytest.mark.parametrize("d,knobs", [(64, ()), (128, (("fwd_w4", 0),))])
def test_dropout(xfa, d, knobs, parity_report):
    """p = 0.17: dropout turns the pipeline off, so raise_max runs beside drop_tile.  The mask is
    the one the launch returns (tests/test_dropout_gpu.py checks it against the CPU Philox)."""
    c = su._case("B", d, BF, "causal", "growing40", 8, knobs)
    q, k, v = su.inputs(c)
    p = 0.17
    with ExitStack() as st:
        _knobs(st, 8, knobs)
        r = xfa.paged_attn.fwd(q.to(DEV), k.to(DEV), v.to(DEV), None, None, p, d ** -0.5, True, -1, 0,
                               0.0, True, None)
        kern = _capi().lib().fmha_last_kernel().decode()
        assert _capi().lib().fmha_last_num_splits() == 1
    torch.cuda.synchronize()
    _ran(kern, "fmha_fwd_kernel<")
    out, lse, s = r[0].cpu(), r[5].cpu(), r[6]
    mask = ~torch.signbit(s[:, :, :su.SQ, :su.SK].float()).cpu()
    ref, _ = orc.attention_ref(q, k, v, None, None, None, p, mask, causal=True)
    pt, _ = orc.attention_ref(q, k, v, None, None, None, p, mask, causal=True, upcast=False,
                              reorder_ops=True)
    lref = orc.attention_lse_ref(q, k, causal=True)
    su.assert_case(f"B-dropout-d{d}-growing40", out, lse, su.Refs(ref, pt, lref, None), parity_report,
                   extra=dict(kernel=_kname(kern)))


def _paged_case(name, c, q, window, want, report, num_splits=1):
    o, lse, kern, splits = run_paged(c, q, window, num_splits)
    _ran(kern, want)
    assert splits == num_splits
    ora = du.oracle(c, q, window)
    r = su.Refs(ora.ref, ora.pt, ora.lse, su._rounding_bound(q, None, torch.cat(c.vx), False, ref=ora.ref))
    # the project's kvcache rule: 3 x + 1e-5
    su.assert_case(name, o, lse, r, report, mult=3.0, atol=1e-5, extra=dict(kernel=_kname(kern)))


@pytest.mark.parametrize("d", [64, 128])
def test_leftpad_cache(d, parity_report):
    """cache_leftpad on a one-page cache (the masked loops of fmha_fwd_kernel; D = 128 too: a
    leftpad launch is not eligible for the ping-pong kernels)"""
    lens, lp = [417, 300], [5, 23]
    c = su.grown_cache(lens, d, BF, False, "growing40", 432, 1, leftpad=lp)
    q = du.make_q(2, su.SQ, su.H, d, BF, 81)
    with _option("fwd_slack", 8):
        _paged_case(f"B-leftpad-d{d}-growing40", c, q, (-1, 0), "fmha_fwd_kernel<", parity_report)


@pytest.mark.parametrize("slack", [8, 0])
@pytest.mark.parametrize("pattern", ["growing4", "growing40"])
@pytest.mark.parametrize("page,want", [(16, "fmha_fwdpp_paged_kernel "), (48, "fmha_fwd_kernel<")])
def test_paged_prefill(page, want, pattern, slack, parity_report):
    """D = 128 prefill over a paged cache: page 16 runs the paged ping-pong kernel, page 48 (no
    power of two) is refused by it and runs fmha_fwd_kernel's paged staging"""
    _need("fwd_w4", 4)
    lens = [417, 333]
    c = su.grown_cache(lens, 128, BF, False, pattern, page, (417 + page - 1) // page + 1)
    q = du.make_q(2, su.SQ, su.H, 128, BF, 82)
    with _option("fwd_slack", slack):
        _paged_case(f"D-paged{page}-d128-{pattern}-s{slack}", c, q, (-1, 0), want, parity_report)


# --------------------------------------------------------------- F: fp8 forward ----------------
def _fp8_want(c: su.Fp8Case):
    if su.MASKS[c.mask][0] >= 0 or ("fp8_w4", 0) in c.knobs:
        return "fmha_fwd_fp8_kernel<8 waves>"
    _need("fp8_w4", 1, c.knobs)
    return "fmha_fwd8w_kernel "


@pytest.mark.parametrize("c", su.FP8_CASES, ids=[su.fp8_case_id(c) for c in su.FP8_CASES])
def test_fp8(c, xfa, parity_report):
    want = _fp8_want(c)
    capi = _capi()
    L = capi.lib()
    (q8, qs), (k8, ks), (v8, vs) = su.fp8_inputs(c.kind, c.pattern)
    window = su.MASKS[c.mask]
    qd, kd, vd = q8.to(DEV), k8.to(DEV), v8.to(DEV)
    out = torch.full(q8.shape, NAN, device=DEV, dtype=c.out)
    with ExitStack() as st:
        _knobs(st, c.slack, c.knobs)
        if c.kind == "dense":
            lse = torch.full((1, su.H, su.SQ), NAN, device=DEV, dtype=torch.float32)
            L.fmha_fwd_fp8(qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), out.data_ptr(), lse.data_ptr(),
                           qs, ks, vs, su.SQ, su.SK, 1, su.H, su.HK, 128, 128 ** -0.5, window[0],
                           window[1], c.out == FP, capi.stream_handle())
            capi.check()
        else:
            cu = _cu(su.FP8_LENS).to(DEV)
            out, lse = xfa.paged_attn.varlen_fwd_fp8(qd, kd, vd, out, cu, cu, None, max(su.FP8_LENS),
                                                     max(su.FP8_LENS), qs, ks, vs, 128 ** -0.5, False,
                                                     window[0], window[1], c.out == FP)
        kern = L.fmha_last_kernel().decode()
    torch.cuda.synchronize()
    _ran(kern, want)
    out, lse = out.cpu(), lse.cpu()
    probs, _ = su.fp8_problems(c)
    a = 0
    for i, (p8, pk8, pv8) in enumerate(probs):
        n = p8.shape[1]
        o_i = out if c.kind == "dense" else out[a:a + n][None]
        l_i = lse if c.kind == "dense" else lse[:, a:a + n][None]
        a += n
        r = su.fp8_refs(p8, pk8, pv8, qs, ks, vs, window, c.out)
        sk = pk8.shape[1]
        w = (window[0], sk) if window[0] >= 0 and window[1] < 0 else window
        mdl = attention_fp8_kernel_model(p8, pk8, pv8, qs, ks, vs, window_size=w, slack=c.slack).to(c.out)
        extra = dict(kernel=_kname(kern), model_err=(mdl.float() - r.ref.float()).abs().max().item())
        su.assert_case(f"{su.fp8_case_id(c)}-seq{i}", o_i, l_i, r, parity_report, mult=3.0, atol=1e-3,
                       extra=extra)


# --------------------------------------------------------------- G: decode ---------------------
@pytest.mark.parametrize("fold", [0, 1])
@pytest.mark.parametrize("num_splits", [4, 8])
@pytest.mark.parametrize("pattern", ["growing40", "late40"])
@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("d", [128, 64])
def test_decode(d, fp8, pattern, num_splits, fold, parity_report):
    """sq = 1 over caches of 600 and 417 keys (640 a row: 20 tiles of 32, up to 8 splits).  Every
    split ends with its own max, far apart under these keys, and the step of late_step lies in the
    last split; the combine (or the folded merge) has to bring them together."""
    c, q = su.decode_problem(d, fp8, pattern)
    with ExitStack() as st:
        _knobs(st, 8, (("dec_fold", fold), ("dec_mr", 16), ("dec_hmaj", 0), ("fwd_decode", 1)))
        o, lse, kern, splits = du.run_decode(c, q, num_splits, {}, 16)
    assert splits == num_splits, (splits, kern)
    name = f"G-decode-d{d}-{'fp8' if fp8 else 'bf16'}-{pattern}-x{num_splits}-fold{fold}"
    ok, f = du.judge(o, lse, du.oracle(c, q))
    print(f"{name}: {f}")
    kn = _kname(kern)
    parity_report(dict(case=name, metric="o", err=f["err"], bound=f["bound"], kernel=kn,
                       ok=f["err"] <= f["bound"] and f["nan_o"] == 0))
    parity_report(dict(case=name, metric="lse", err=f["lse_err"], bound=du.LSE_ATOL, kernel=kn,
                       ok=f["lse_err"] <= du.LSE_ATOL and f["inf_ok"] and f["nan_lse"] == 0))
    assert ok, f"{name}: {f}"
