"""GPU: the MLA prefill backward (fmha_bwd_mla_pre / dkdv / dq kernels: head size 192 for Q K^T,
128 for V) against the float64 oracle, per sequence, under the backward's rules
(`bwd_util.check_grads`: global rule mult 3 and the block rule; `assert_exact_zeros`).

The forward's O and LSE come from `paged_attn.fwd_mla` / `varlen_fwd_mla`.  The cases are
tests/bwd_mla_util.py CASES, the ones tests/test_bwd_mla_ref.py proves satisfiable on the CPU.
Every case runs through the C ABI on poisoned `bwd_util.Arena` operands (4 KiB guards; v and dv
strided views of [tokens, hk, 256] buffers, the kv-projection layout): every dq / dk / dv element is
written, no guard byte and none of the columns beside v and dv changes.
"""
import pytest
import torch

import xf_flash_attention_cutlass_amd as xfa
from tests import bwd_mla_util as mu
from tests import bwd_util as bu

pytestmark = pytest.mark.gpu
DEV = mu.DEV
DTS = list(mu.DTYPES)


def _bits(x):
    return x.contiguous().view(torch.int16 if x.element_size() == 2 else torch.int32)


def _same(a, b):
    return all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("case", mu.CASES, ids=[c.name for c in mu.CASES])
def test_case_through_the_c_abi_on_poisoned_arenas(case, dt, parity_report):
    dtype = mu.DTYPES[dt]
    got = mu.run_capi_arena(xfa, case, dtype, fill=0xFF)
    mu.check_case(f"bwd_mla {case.name} {dt}", got, case, dtype, parity_report)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("name", ["p_causal", "p_rev_full", "d64x400_w20_0", "d300x113_causal"])
def test_results_do_not_depend_on_the_poison(name, dt):
    """Fills 0xFF (NaNs: an unwritten or leaked element shows) and 0x00: identical bits."""
    case, dtype = mu.CASE[name], mu.DTYPES[dt]
    a = mu.run_capi_arena(xfa, case, dtype, fill=0xFF)
    b = mu.run_capi_arena(xfa, case, dtype, fill=0x00)
    assert _same(a, b), f"{name} {dt}: results differ between fills 0xFF and 0x00"


def _device_operands(case, dtype, scale=None, q=None):
    """NaN-filled dq / dk / dv beside the case's inputs (q: another q in their place) and its forward"""
    q, k, v, g = (x.to(DEV) for x in (q, *mu.make(case, dtype)[1:])) if q is not None else (
        x.to(DEV) for x in mu.make(case, dtype))
    out, lse = mu.forward(xfa, case, q, k, v, scale)
    t = dict(q=q, k=k, v=v, dout=g, out=out, lse=lse)
    for n, like in (("dq", q), ("dk", k), ("dv", v)):
        t[n] = torch.full_like(like, float("nan"))
    return t


def _grads(t):
    return tuple(t[n].cpu() for n in bu.NAMES)


# ------------------------------------------------------------------ reproducibility, graph -----
@pytest.mark.parametrize("dt", DTS)
def test_two_calls_and_a_graph_replay_are_bit_equal(dt):
    case, dtype = mu.CASE["p_causal"], mu.DTYPES[dt]
    t = _device_operands(case, dtype)
    cus = (mu.cu(case.lens_q).to(DEV), mu.cu(case.lens_k).to(DEV))
    assert mu.capi_call(case, t, cus=cus)[0] == 0
    torch.cuda.synchronize()
    first = _grads(t)
    assert mu.capi_call(case, t, cus=cus)[0] == 0
    torch.cuda.synchronize()
    assert _same(first, _grads(t))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):              # warm-up on the capture stream: its scratch pool exists
        assert mu.capi_call(case, t, cus=cus)[0] == 0
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for n in bu.NAMES:
        t[n].fill_(float("nan"))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        status, msg, _ = mu.capi_call(case, t, cus=cus)
    assert status == 0, msg
    torch.cuda.synchronize()
    assert all(torch.isnan(t[n]).all() for n in bu.NAMES), "the capture itself must not run the kernels"
    g.replay()
    torch.cuda.synchronize()
    assert _same(first, _grads(t))


# ------------------------------------------------------------------ surface --------------------
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("name", ["d113x300_causal", "p_causal"])
def test_c_abi_pybind_and_wrappers_agree_bit_for_bit(name, dt):
    """The test that fails without the feature: before it none of these entries exists."""
    case, dtype = mu.CASE[name], mu.DTYPES[dt]
    t = _device_operands(case, dtype)
    status, msg, kern = mu.capi_call(case, t)
    torch.cuda.synchronize()
    assert status == 0, msg
    assert kern.startswith(mu.KERNELS + " persistent=0 xcdq=0 grid="), kern
    assert "block=256" in kern
    c = _grads(t)
    p = mu.run_pybind(xfa, case, dtype)
    out_w, *w = mu.run_wrapper(xfa, case, dtype)
    assert _same(c, p), "C ABI != pybind"
    assert _same(c, w), "C ABI != autograd through the wrapper"
    # the wrapper's forward is flash_attn_func's at this shape, bit for bit
    q, k, v, _ = (x.to(DEV) for x in mu.make(case, dtype))
    with torch.no_grad():
        if case.packed:
            cq, ck = mu.cu(case.lens_q).to(DEV), mu.cu(case.lens_k).to(DEV)
            ref = xfa.flash_attn_varlen_func(q, k, v, cq, ck, max(case.lens_q), max(case.lens_k), causal=case.causal)
            own, lse, _ = xfa.flash_attn_mla_varlen_func(q, k, v, cq, ck, max(case.lens_q), max(case.lens_k),
                                                         causal=case.causal, return_attn_probs=True)
        else:
            qd, kd, vd = (mu.as_dense(case, x) for x in (q, k, v))
            ref = xfa.flash_attn_func(qd, kd, vd, causal=case.causal)
            own, lse, _ = xfa.flash_attn_mla_func(qd, kd, vd, causal=case.causal, return_attn_probs=True)
    assert not own.requires_grad and not lse.requires_grad
    assert _same((ref.reshape(-1, case.h, mu.DV).cpu(),), (own.reshape(-1, case.h, mu.DV).cpu(),))
    assert _same((out_w,), (own.reshape(-1, case.h, mu.DV).cpu(),))


def test_wrapper_lse_carries_no_gradient_and_deterministic_changes_nothing():
    case, dtype = mu.CASE["d113x300_causal"], torch.bfloat16
    q, k, v, g = (mu.as_dense(case, x.to(DEV)) for x in mu.make(case, dtype))
    res = []
    for det in (False, True):
        qq, kk, vv = (x.clone().requires_grad_(True) for x in (q, k, v))
        out, lse, _ = xfa.flash_attn_mla_func(qq, kk, vv, causal=True, deterministic=det, return_attn_probs=True)
        assert out.requires_grad and not lse.requires_grad
        res.append(tuple(x.cpu() for x in torch.autograd.grad(out, (qq, kk, vv), g)))
    assert _same(*res)


def test_a_strided_and_a_transposed_dout_give_the_same_bits():
    case, dtype = mu.CASE["d113x300_causal"], torch.bfloat16
    q, k, v, g = (mu.as_dense(case, x.to(DEV)) for x in mu.make(case, dtype))
    qq, kk, vv = (x.clone().requires_grad_(True) for x in (q, k, v))
    out = xfa.flash_attn_mla_func(qq, kk, vv, causal=True)
    want = tuple(x.cpu() for x in torch.autograd.grad(out, (qq, kk, vv), g, retain_graph=True))
    wide = torch.zeros(*g.shape[:-1], 2 * mu.DV, dtype=dtype, device=DEV)
    wide[..., :mu.DV] = g                                        # rows 256 apart: read in place
    got = tuple(x.cpu() for x in torch.autograd.grad(out, (qq, kk, vv), wide[..., :mu.DV], retain_graph=True))
    assert _same(want, got)
    tr = g.transpose(-1, -2).contiguous().transpose(-1, -2)      # last dimension not unit-stride
    got = tuple(x.cpu() for x in torch.autograd.grad(out, (qq, kk, vv), tr))
    assert _same(want, got)


@pytest.mark.parametrize("dt", DTS)
def test_non_default_scale(dt, parity_report):
    """softmax_scale = 192^-1/2 / 2 on 2 q (exact in either dtype) is the default scale on q: dk and
    dv are the case's own, and dq is half its dq."""
    case, dtype = mu.CASE["d113x300_causal"], mu.DTYPES[dt]
    q = mu.make(case, dtype)[0]
    twice = (q.float() * 2).to(dtype)
    assert torch.equal(twice.float() / 2, q.float())
    scale = mu.DQK ** -0.5 / 2
    t = _device_operands(case, dtype, scale, q=twice.to(DEV))
    status, msg, _ = mu.capi_call(case, t, scale)
    torch.cuda.synchronize()
    assert status == 0, msg
    dq, dk, dv = _grads(t)
    mu.check_case(f"bwd_mla scale / 2 {dt}", ((dq.float() * 2).to(dtype), dk, dv), case, dtype, parity_report)


# ------------------------------------------------------------------ refusals -------------------
def test_refusals_leave_nan_filled_outputs_nan():
    case, dtype = mu.CASE["p_causal"], torch.bfloat16
    t = _device_operands(case, dtype)
    bad = [
        (dict(pair=(128, 128)), "(192, 128) only"),
        (dict(t=dict(t, dout=None)), "dout must be a non-null"),
        (dict(t=dict(t, lse=None)), "softmax_lse must be a non-null"),
        (dict(t=dict(t, q=t["q"][:, :, 4:])), "16-byte aligned"),
        (dict(t=dict(t, dout=t["dout"][:, :, 4:])), "dout must be a 16-byte aligned"),
    ]
    for over, needle in bad:
        kw = dict(t=t)
        kw.update(over)
        status, msg, kern = mu.capi_call(case, kw.pop("t"), **kw)
        assert status == 1 and needle in msg and kern == "", (over.keys(), status, msg, kern)
    dense = mu.CASE["d113x300_full"]
    td = _device_operands(dense, dtype)
    status, msg, kern = mu.capi_call(dense, dict(td, dk=None))
    assert status == 1 and "dk must be a non-null" in msg and kern == ""
    with pytest.raises(RuntimeError, match="dq must have shape"):
        xfa.paged_attn.bwd_mla(*(mu.as_dense(dense, td[n]) for n in ("dout", "q", "k", "v", "out")), td["lse"],
                               mu.as_dense(dense, td["dq"])[:, :50], None, None)
    with pytest.raises(RuntimeError, match="softmax_lse must be fp32"):
        xfa.paged_attn.varlen_bwd_mla(t["dout"], t["q"], t["k"], t["v"], t["out"], t["lse"].half(), t["dq"], t["dk"],
                                      t["dv"], mu.cu(case.lens_q).to(DEV), mu.cu(case.lens_k).to(DEV), 300, 333)
    torch.cuda.synchronize()
    for x in (t, td):
        assert all(torch.isnan(x[n]).all() for n in bu.NAMES)
