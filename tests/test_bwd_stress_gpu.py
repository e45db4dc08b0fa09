"""GPU: every backward instance off the unit-randn regime.

Every other backward test draws q, k, v and dO as unit randn, where D = rowsum(dO * O) is small
beside dP, a wrongly unmasked score costs P = 1 / sk and the LSE comes from a forward that never
rescaled.  These cases put the key-scale patterns of tests/softmax_stress_util.py on q and k
(tests/bwd_stress_util.py): peaked rows (|D| = |dP|), masked scores far above the row's LSE, |S c|
in the hundreds, forwards at fwd_slack 0 and 16, dO scaled by 256 (fp16) and 2^20 (bf16), packed
sequences and sinks at the median LSE.  tests/test_bwd_stress_util.py shows on the CPU that the
rule below rejects a kernel with a wrong D or a wrongly unmasked block on these inputs.

Every case makes its inputs on the CPU, runs `flash_attn_func` (`flash_attn_varlen_func`) with
autograd, keeps the forward's O and LSE, and judges dq / dk / dv by the stress rule
(`bwd_stress_util.check_stress`: `check_grads`' two rules with the error of the low-precision
estimate taken as the larger of |pt - ref| and |emu - ref|, emu = `emulate_bwd` fed that O and
LSE).  Since the second estimate stands on the forward's LSE, the LSE is first held to the
forward's own rule (1e-3 + 1e-5 |ref|, the same +inf rows).  Gradients must be finite; non-FEAT
cases also pass `assert_exact_zeros`; deterministic cases are bitwise equal across two runs and
in dk / dv to the atomic run.  Knobs are set through `_option` only and restored.  Each row of
`parity_report` carries `widen`, `emu_plain` and the forward kernel's name, and `emu_plain` is
held under the cap of tests/bwd_stress_util.py (3) on every case, dense and packed.
"""
from contextlib import ExitStack

import pytest
import torch

from tests import bwd_stress_util as su
from tests import bwd_util as bu
from tests import sink_ref as sr
from tests.softmax_stress_util import LSE_ATOL, LSE_RTOL, _option

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def xfa():
    import xf_flash_attention_cutlass_amd as m
    return m


def _lib():
    from xf_flash_attention_cutlass_amd import capi
    return capi.lib()


def _need(name, value):
    """skip when the session's knob (XFA_TEST_OPTIONS) sends the forward to another kernel"""
    have = _lib().fmha_get_option(name.encode())
    if have != value:
        pytest.skip(f"the forward this case asserts needs {name} = {value}; the session runs "
                    f"{name} = {have}")


def _kname(kern):
    return kern.split(" persistent=")[0]


def _knobs(stack, c: su.Case):
    if c.slack is not None:
        stack.enter_context(_option("fwd_slack", c.slack))
    if c.w4 == 0:
        stack.enter_context(_option("fwd_w4", 0))


def _run(xfa, c: su.Case, qkvg, det, sink=None):
    """(grads on the CPU (dq, dk, dv[, dsink]), O, LSE, the forward kernel's name)"""
    q, k, v, g = qkvg
    qd, kd, vd = (x.to(DEV).requires_grad_(True) for x in (q, k, v))
    causal, window = su.MASKS[c.mask]
    kw = dict(causal=causal, window_size=window, deterministic=det, return_attn_probs=True)
    if c.feat:
        kw.update(softcap=su.SOFTCAP, alibi_slopes=su.slopes_of(c).to(DEV))
    leaves = (qd, kd, vd)
    if sink is not None:
        sd = sink.to(DEV).requires_grad_(True)
        kw.update(sink=sd)
        leaves += (sd,)
    with ExitStack() as st:
        _knobs(st, c)
        if c.w4 is None:
            out, lse, _ = xfa.flash_attn_func(qd, kd, vd, **kw)
        else:
            # The D = 128 ping-pong forward takes single-pass launches only, and a dense launch of
            # these shapes splits its keys; a packed launch never does.  So the batch goes as b
            # sequences of equal length, under fwd_w4 = 0 too: the pair differs in the kernel only.
            b, sq, sk = q.shape[0], q.shape[1], k.shape[1]
            cu_q, cu_k = (su.cu([n] * b).to(DEV) for n in (sq, sk))
            out, lse, _ = xfa.flash_attn_varlen_func(qd.flatten(0, 1), kd.flatten(0, 1), vd.flatten(0, 1),
                                                     cu_q, cu_k, sq, sk, **kw)
            out = out.view(q.shape)
            lse = lse.view(lse.shape[0], b, sq).permute(1, 0, 2)        # [h, b * sq] -> [b, h, sq]
        kern = _lib().fmha_last_kernel().decode()
    grads = torch.autograd.grad(out, leaves, g.to(DEV))
    return [x.cpu() for x in grads], out.detach().cpu(), lse.cpu(), kern


def _check_lse(name, lse, own):
    """the forward's LSE by the forward's own rule against the emulation's fp32 LSE"""
    fin = torch.isfinite(own)
    assert torch.equal(torch.isinf(lse) & (lse > 0), ~fin), f"{name}: the LSE's +inf rows differ"
    err = ((lse[fin] - own[fin]).abs() - LSE_RTOL * own[fin].abs()).max().item() if fin.any() else 0.0
    assert err <= LSE_ATOL, f"{name}: forward LSE off by {err:.3g} beyond 1e-5 |ref|"


def _deterministic(name, got, again, atomic):
    for nm, x, y in zip(bu.NAMES, got, again):
        assert torch.equal(x, y), f"{name} {nm}: two deterministic runs differ"
    assert torch.equal(got[1], atomic[1]), f"{name}: dk differs from the atomic run"
    assert torch.equal(got[2], atomic[2]), f"{name}: dv differs from the atomic run"


def _check_need(name, rows):
    """The second estimate stands on the O and LSE the forward stored, so a forward that stored
    them wrong would raise |emu - ref| and the bound with it: its error over the plain bound is
    held under the cap the CPU twin holds the emulation's own O and LSE to."""
    need = su.widen_needed(rows)
    print(f"{name}: widen_needed " + " ".join(f"{g} {x:.2f}" for g, x in need.items()))
    assert max(need.values()) <= su.NEED_CAP, f"{name}: widen_needed {need} > {su.NEED_CAP}"


def _show(rows):
    print("; ".join(f"{r['metric']} {r['err']:.3g}/{r['bound']:.3g} w{r['widen']:.2f}" for r in rows))


@pytest.mark.parametrize("c", su.CASES, ids=su.case_id)
def test_dense(xfa, parity_report, c):
    if c.w4 == 4:
        _need("fwd_w4", 4)
    name = "bwd stress " + su.case_id(c)
    qkvg = su.inputs(c)
    refs, sref = su.case_refs(su.input_key(c))
    sink = sref.sink if sref else None
    got, o, lse, kern = _run(xfa, c, qkvg, c.det, sink)
    if c.w4 is not None:
        want = "fmha_fwdpp" if c.w4 == 4 else "fmha_fwd_kernel<"
        assert kern.startswith(want), f"ran {kern!r}, wanted {want}"
    if c.det:
        again = _run(xfa, c, qkvg, True, sink)[0]
        atomic = _run(xfa, c, qkvg, False, sink)[0]
        _deterministic(name, got, again, atomic)
        if sink is not None:
            assert torch.equal(got[3], again[3]), f"{name}: dsink differs between two runs"
    ekw = su.emu_kw(c)
    _check_lse(name, lse, bu.emulate_fwd(*qkvg[:3], sink=sink, **ekw)[1])
    emu = bu.emulate_bwd(*qkvg, o=o, lse=lse, sink=sink, **ekw)
    rows = su.check_stress(name, got[:3], refs, emu, c.dtype, parity_report, su.mult_of(c),
                           extra=dict(kernel=_kname(kern)))
    _show(rows)
    _check_need(name, rows)
    if not c.feat:
        causal, window = su.MASKS[c.mask]
        bu.assert_exact_zeros(name, got[:3], causal, window)
    if sink is not None:
        sr.check_dsink(name, got[3], sref.ds64, sref.dspt, sref.term, parity_report)


@pytest.mark.parametrize("p", su.PACKED, ids=su.case_id)
def test_packed(xfa, parity_report, p):
    """`flash_attn_varlen_func` over sequences of 1 .. 300 queries and 20 .. 600 keys (queries
    beyond the keys and keys beyond the queries), each sequence's keys grown separately; every
    sequence is judged on its own, the report keeps the worst row per metric, with the largest
    `emu_plain` over the sequences beside it (`emu_plain_case`)."""
    name = "bwd stress " + su.case_id(p)
    causal, window = su.MASKS[p.mask]
    q, k, v, g = su.packed_inputs(p.d, p.dtype, p.pattern)
    cu_q, cu_k = su.cu(su.PACKED_LQ), su.cu(su.PACKED_LK)

    def run(det):
        qd, kd, vd = (x.to(DEV).requires_grad_(True) for x in (q, k, v))
        out, lse, _ = xfa.flash_attn_varlen_func(
            qd, kd, vd, cu_q.to(DEV), cu_k.to(DEV), max(su.PACKED_LQ), max(su.PACKED_LK),
            causal=causal, window_size=window, deterministic=det, return_attn_probs=True)
        kern = _lib().fmha_last_kernel().decode()
        grads = torch.autograd.grad(out, (qd, kd, vd), g.to(DEV))
        return [x.cpu() for x in grads], out.detach().cpu(), lse.cpu(), kern

    got, o, lse, kern = run(p.det)
    if p.det:
        _deterministic(name, got, run(True)[0], run(False)[0])
    refs = su.packed_refs(p.d, p.dtype, p.mask, p.pattern)
    emus = su.packed_emulate(p, o, lse)
    worst, failures, rows = bu.WorstRows(), [], []
    for i, (sq_, sk_) in enumerate(zip(bu.seq_slices(cu_q), bu.seq_slices(cu_k))):
        seq = (got[0][sq_][None], got[1][sk_][None], got[2][sk_][None])
        own = bu.emulate_fwd(q[sq_][None], k[sk_][None], v[sk_][None], causal, window)[1]
        _check_lse(f"{name} seq{i}", lse[:, sq_][None], own)
        try:
            rows += su.check_stress(f"{name} seq{i}", seq, refs[i], emus[i], p.dtype, worst,
                                    extra=dict(kernel=_kname(kern)))
        except AssertionError as e:
            failures.append(str(e))
        bu.assert_exact_zeros(f"{name} seq{i}", seq, causal, window)
    _show(worst.rows.values())
    need = su.widen_needed(rows)
    for r in worst.rows.values():        # a kept row's emu_plain is its own sequence's
        r["emu_plain_case"] = need.get(r["metric"].split()[0])
    worst.flush(parity_report)
    assert not failures, "; ".join(failures)
    _check_need(name, rows)


@pytest.mark.parametrize("pattern", ["unit", "growing4"])
@pytest.mark.parametrize("mask", ["full", "causal"])
@pytest.mark.parametrize("d", [64, 128])
def test_gradients_are_linear_in_dout(xfa, d, mask, pattern):
    """No tolerance: deterministic bf16 gradients of dO * 2^6 are 2^6 x the gradients of dO, bit
    for bit.  D, dP and dS scale exactly, P does not depend on dO and the slice order is fixed, so
    anything added into dQ / dK / dV that is not linear in dO breaks it: stale workspace, an LSE
    read in D's place.  Compared on every element of magnitude >= 2^-60 in both results; the
    others must be below 2^-59 in both (fp32 flush-to-zero may differ there)."""
    c = su.Case("", d, su.BF, mask, False, True, pattern, None, 1.0, None, False)
    q, k, v, g = su.inputs(c)
    one = _run(xfa, c, (q, k, v, g), True)[0]
    big = _run(xfa, c, (q, k, v, (g.float() * 64).to(su.BF)), True)[0]
    for nm, a, b_ in zip(bu.NAMES, one, big):
        a, b_ = a.float() * 64, b_.float()
        assert torch.isfinite(a).all() and torch.isfinite(b_).all(), nm
        both = (a.abs() >= 2.0 ** -60) & (b_.abs() >= 2.0 ** -60)
        assert both.any(), nm
        assert torch.equal(a[both], b_[both]), \
            f"{nm}: {(a[both] != b_[both]).sum().item()} of {int(both.sum())} elements differ"
        assert (a[~both].abs() < 2.0 ** -59).all() and (b_[~both].abs() < 2.0 ** -59).all(), nm
