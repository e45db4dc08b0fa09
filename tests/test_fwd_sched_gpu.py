"""GPU: every forward kernel walks every item schedule to the same result (fwd_walk,
csrc/fmha_fwd_sched.h), at a shape the other tests' even shapes miss: 19 heads, 1100 rows = 5 row
blocks of 256 with the last one partial (the odd count takes the pair schedule's skip), and the
smallest batch with more items than CUs and a unit count that is no multiple of 8 (the per-XCD
queues then differ in length).  Each kernel runs once with one workgroup per item
(fwd_persistent = 0, the baseline, held to the oracle on two sampled (batch, head) pairs) and then
under the boustrophedon, the XCD-grouped pairs, the per-XCD dynamic queues and the global dynamic
queue (the dynamic ones twice: the counters reset themselves): the schedule fmha_last_kernel
reports is the one plan_fwd should choose, and O and LSE equal the baseline's bit for bit.
"""
import functools

import pytest
import torch

from oracle import attention_ref as orc
from tests import test_fp8_gpu as f8
from tests.test_kernel_variants_gpu import _run, _variants

pytestmark = pytest.mark.gpu
DEV = "cuda"
H, S, D, ROWS = 19, 1100, 128, 256
KNOBS = (b"fwd_persistent", b"fwd_order", b"fwd_dyn", b"fwd_xcdq", b"fwd_waves", b"fwd_w4", b"fp8_w4")

# kernel name, variants build, kernel-choice knob, causal, has dynamic queues on dense input
KERNELS = [
    ("fmha_fwd_kernel<8 waves>", False, (b"fwd_w4", 0), True, True),
    ("fmha_fwdpp_kernel", False, (b"fwd_w4", 2), True, True),
    ("fmha_fwdpp16_kernel", False, (b"fwd_w4", 3), False, True),
    ("fmha_fwd8w_kernel", False, (b"fp8_w4", 1), True, True),
    ("fmha_fwd_fp8_kernel<8 waves>", False, (b"fp8_w4", 0), True, False),
    ("fmha_fwd4_kernel", True, (b"fwd_w4", 1), True, True),
    ("fmha_fwd8pp_kernel", True, (b"fp8_w4", 2), True, True),
]


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _batch():
    b = 1
    while not (b * H * ((S + ROWS - 1) // ROWS) > _cus() and (b * H) % 8):
        b += 1
    return b


@functools.lru_cache(maxsize=None)
def _inputs(fp8):
    b = _batch()
    if fp8:
        return f8._case(b, H, H, S, S, 19)
    g = torch.Generator().manual_seed(19)
    return tuple(torch.randn(b, S, H, D, generator=g).bfloat16() for _ in range(3))


def _expected(setting, dyn_ok):
    """(persistent, xcdq) plan_fwd chooses: slots = CUs, 5 * b * 19 items > slots by _batch()"""
    pairs = 2 if _cus() % 8 == 0 else 1
    order, dyn, xcdq = setting
    if dyn == 2 and dyn_ok:
        return 3, int(xcdq and _cus() % 8 == 0 and _batch() * H >= 8)
    return (pairs if order == 1 else 1), 0


@pytest.mark.parametrize("name,variants,choice,causal,dyn_ok", KERNELS, ids=[k[0] for k in KERNELS])
def test_every_schedule_gives_the_baseline(name, variants, choice, causal, dyn_ok):
    from xf_flash_attention_cutlass_amd import capi
    lib = _variants() if variants else capi.lib()
    fp8 = choice[0] == b"fp8_w4"
    b = _batch()
    o = torch.empty(b, S, H, D, device=DEV, dtype=torch.bfloat16)
    lse = torch.empty(b, H, S, device=DEV, dtype=torch.float32)
    wr = 0 if causal else -1
    if fp8:
        (q8, qs), (k8, ks), (v8, vs) = _inputs(True)
        qd, kd, vd = (x.to(DEV) for x in (q8, k8, v8))
        call = lambda: lib.fmha_fwd_fp8(qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), o.data_ptr(),  # noqa: E731
                                        lse.data_ptr(), qs, ks, vs, S, S, b, H, H, D, D ** -0.5, -1, wr,
                                        False, capi.stream_handle())
    else:
        q, k, v = _inputs(False)
        qd, kd, vd = (x.to(DEV) for x in (q, k, v))
        call = lambda: lib.fmha_fwd(qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), o.data_ptr(), None, S, S,  # noqa: E731
                                    b, H, H, D, 0.0, capi.stream_handle(), None, D ** -0.5, None,
                                    lse.data_ptr(), -1, wr, 0.0, False, False, 1)

    def run(options, persistent, xcdq):
        for knob, val in options.items():
            assert lib.fmha_set_option(knob, val) == 0, lib.fmha_last_error()
        o.fill_(float("nan"))
        lse.fill_(float("nan"))
        kern = _run(lib, call)
        assert kern.startswith(f"{name} persistent={persistent} xcdq={xcdq} "), kern
        return o.cpu(), lse.cpu()

    old = {knob: lib.fmha_get_option(knob) for knob in KNOBS}
    try:
        base = run({b"fwd_waves": 8, choice[0]: choice[1], b"fwd_persistent": 0}, 0, 0)
        # order, dyn, xcdq; the dynamic queues twice (their counters reset themselves)
        for setting in [(0, 0, 1), (1, 0, 1), (1, 2, 1), (1, 2, 1), (1, 2, 0), (1, 2, 0)]:
            persistent, xq = _expected(setting, dyn_ok)
            got = run({b"fwd_persistent": 1, b"fwd_order": setting[0], b"fwd_dyn": setting[1],
                       b"fwd_xcdq": setting[2]}, persistent, xq)
            assert torch.equal(got[0], base[0]) and torch.equal(got[1], base[1]), (name, setting)
    finally:
        for knob, val in old.items():
            lib.fmha_set_option(knob, val)

    # the baseline against the oracle, two sampled (batch, head) pairs
    for bi, hi in ((0, 0), (b - 1, H - 1)):
        out = base[0][bi:bi + 1, :, hi:hi + 1].float()
        if fp8:
            q1, k1, v1 = (x[bi:bi + 1, :, hi:hi + 1] for x in (q8, k8, v8))
            ref, _ = orc.attention_ref(q1.float() * qs, k1.float() * ks, v1.float() * vs, causal=causal)
            pt = orc.attention_fp8_pt(q1, k1, v1, qs, ks, vs, causal=causal).to(torch.bfloat16)
            ok, err, bound = orc.parity_ok(out, ref, pt, 3.0, 1e-3)     # the fp8 tests' model
        else:
            q1, k1, v1 = (x[bi:bi + 1, :, hi:hi + 1] for x in (q, k, v))
            ref, _ = orc.attention_ref(q1, k1, v1, causal=causal)
            pt, _ = orc.attention_ref(q1, k1, v1, causal=causal, upcast=False, reorder_ops=True)
            ok, err, bound = orc.parity_ok(out, ref, pt, 2.0, 1e-5)
        assert ok, f"{name} ({bi}, {hi}): max|out-ref| = {err:.3g} > {bound:.3g}"
