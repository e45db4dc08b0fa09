"""Every backward instance csrc/fmha_bwd.hip dispatches — head-dim bucket {64, 128, 256} x dtype x
MASK x FEAT x deterministic = 48 — against the float64 oracle, through flash_attn_func autograd,
with the global gradient rule and the per-block rule of tests/bwd_util.py.

Shape: b2 h4/hk2, sq 113 (77 in the 256 bucket), sk spanning three key blocks with a ragged tail
(600; 300 in the 256 bucket).  MASK = on is causal or the window (100, 30); FEAT = on is ALiBi with
per-batch slopes plus softcap 20 on q scaled x4 (as test_bwd_softcap_alibi, whose x5 global
multiplier it also takes).  tests/test_bwd_util.py asserts the table is complete."""
import pytest
import torch

from oracle import attention_ref as orc
from tests import bwd_util as bu

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def xfa():
    import xf_flash_attention_cutlass_amd as m
    return m


def _name(t):
    kind = "causal" if t.causal else ("w%d_%d" % t.window if t.mask else "full")
    return "d%d-%s-%s-%s-%s" % (t.d, str(t.dtype).split(".")[-1], kind,
                                "alibi_softcap" if t.feat else "plain", "det" if t.det else "atomic")


def _problem(t, seed):
    b, h, hk = 2, 4, 2
    sq, sk = (77, 300) if bu.bucket(t.d) == 256 else (113, 600)
    gen = torch.Generator().manual_seed(seed)
    q = torch.randn(b, sq, h, t.d, generator=gen)
    if t.feat:
        q = q * 4
    q = q.to(t.dtype)
    k, v = (torch.randn(b, sk, hk, t.d, generator=gen).to(t.dtype) for _ in range(2))
    g = torch.randn(b, sq, h, t.d, generator=gen).to(t.dtype)
    kw, okw = dict(causal=t.causal, window_size=t.window), dict(causal=t.causal, window_size=t.window)
    if t.feat:
        slopes = torch.rand(b, h, generator=gen) * 0.3
        kw.update(softcap=20.0, alibi_slopes=slopes.to(DEV))
        okw.update(softcap=20.0, attn_bias=orc.alibi_bias(slopes, sq, sk, causal=False))
    return (q, k, v, g), kw, okw


def _run(xfa, qkvg, **kw):
    q, k, v, g = qkvg
    qd, kd, vd = (x.to(DEV).requires_grad_(True) for x in (q, k, v))
    out = xfa.flash_attn_func(qd, kd, vd, **kw)
    return [x.cpu() for x in torch.autograd.grad(out, (qd, kd, vd), g.to(DEV))]


def _check_instance(xfa, t, parity_report, seed):
    qkvg, kw, okw = _problem(t, seed)
    got = _run(xfa, qkvg, deterministic=t.det, **kw)
    if t.det:
        again = _run(xfa, qkvg, deterministic=True, **kw)
        for nm, x, y in zip(bu.NAMES, got, again):
            assert torch.equal(x, y), f"{nm}: two deterministic runs differ"
        atomic = _run(xfa, qkvg, deterministic=False, **kw)
        assert torch.equal(got[1], atomic[1]), "dk differs from the atomic run"
        assert torch.equal(got[2], atomic[2]), "dv differs from the atomic run"
    refs = bu.ref_grads(*qkvg, **okw)
    bu.check_grads("instances " + _name(t), got, refs, t.dtype, parity_report,
                   mult=5.0 if t.feat else 3.0)
    if not t.feat:
        bu.assert_exact_zeros(_name(t), got, t.causal, t.window)


@pytest.mark.parametrize("t", bu.instance_table(), ids=_name)
def test_bwd_instance(xfa, parity_report, t):
    _check_instance(xfa, t, parity_report, seed=21)


@pytest.mark.parametrize("mask", ["full", "causal", "window"])
@pytest.mark.parametrize("d", [40, 104, 160])
def test_bwd_instance_padded_dim_deterministic(xfa, parity_report, d, mask):
    """Head dims below their bucket's width, deterministic, with ALiBi + softcap: the slice
    columns >= d are never written and must never be read."""
    causal = mask == "causal"
    t = bu.Instance(d, torch.bfloat16, mask != "full", True, True, causal,
                    (100, 30) if mask == "window" else (-1, -1))
    _check_instance(xfa, t, parity_report, seed=22)
