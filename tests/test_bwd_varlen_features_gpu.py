"""Varlen backward crossed with windows, ALiBi, softcap and deterministic mode (the diagonal
sk_i - sq_i differs per sequence there), against the per-sequence float64 oracle; and a dense
sweep across the kernel's own tile edges (32-row query tiles, 32 / 64 keys per wave, 256-key
blocks, 128 in the 256 bucket), including sq = 1 and sk < 32."""
import itertools

import pytest
import torch

from tests import bwd_util as bu

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, FP = torch.bfloat16, torch.float16

# sq_i > sk_i (33 > 20, 130 > 64), sk_i < 32, sq_i = 1
LQ, LK = [1, 33, 300, 77, 130], [147, 20, 300, 600, 64]
WINDOWS = [(32, 8), (0, 0), (100, 0), "causal"]

# dQ of the softcap cases (q scaled x4: peaked rows) takes the block bound x 14.8 =
# 1.5 x 9.85, the largest ratio measured on the kernels as they were before these tests
# (w100_0-alibi-softcap-det-float16-d64-h8_1, seq 0, the single row of a 1 x 147 sequence).
# Reason: a flash-attention backward takes D = rowsum(dO * O) from the forward's stored O, i.e.
# rounded to the dtype.  On a row whose softmax has one key at P ~ 1 (0.9907 there) the exact dQ
# is close to 0, dS_j = P_j (dP_j - D) is the difference of two O(sqrt(d)) numbers, and the
# rounding of O leaves dQ_row ~ dD * K_j * scale with dD ~ eps/2 * |dO . O|: one scalar error
# per row.  The low-precision oracle forms dP_j - sum(P dP) from the same rounded dP and does not
# see it, so its error there is 30x smaller and the bound with it.  Blocks of one row (sq_i = 1,
# row 32 of sq_i = 33) expose it; in a 32-row block the other rows' error hides it.  The CPU model
# of a correct kernel shows the same (tests/test_bwd_util.py::test_stored_o_rounding_on_peaked_rows:
# 11.0 on that block, 0.58 with D from the unrounded O), so it is the algorithm, not a defect of
# these kernels.  Only the sequences that end in a one-row block take the factor; their dK / dV,
# the other sequences and every case without softcap keep the plain bound.
DQ_PEAKED_BLOCK_FACTOR = 14.8


def _varlen_cases():
    """windows x (ALiBi, softcap) x deterministic in full; dtype, head dim and the head counts
    are paired onto them (each of the 8 combinations appears 4 times)."""
    cases = []
    for wi, (fi, (alibi, softcap)), det in itertools.product(
            range(4), enumerate(itertools.product((False, True), (0.0, 20.0))), (False, True)):
        c = (2 * fi + det + 3 * wi) % 8
        cases.append((WINDOWS[wi], alibi, softcap, det, (BF, FP)[c % 2], (64, 128)[c // 2 % 2],
                      ((4, 2), (8, 1))[c // 4]))
    return cases


def _vname(c):
    win, alibi, softcap, det, dtype, d, (h, hk) = c
    w = win if win == "causal" else "w%d_%d" % win
    return "%s-%s%s%s-%s-d%d-h%d_%d" % (w, "alibi" if alibi else "noalibi",
                                        "-softcap" if softcap else "", "-det" if det else "",
                                        str(dtype).split(".")[-1], d, h, hk)


@pytest.fixture(scope="module")
def xfa():
    import xf_flash_attention_cutlass_amd as m
    return m


def _varlen_run(xfa, q, k, v, g, lq, lk, max_q, max_k, **kw):
    cu_q = torch.tensor([0] + list(itertools.accumulate(lq)), dtype=torch.int32, device=DEV)
    cu_k = torch.tensor([0] + list(itertools.accumulate(lk)), dtype=torch.int32, device=DEV)
    qd, kd, vd = (x.to(DEV).requires_grad_(True) for x in (q, k, v))
    out = xfa.flash_attn_varlen_func(qd, kd, vd, cu_q, cu_k, max_q, max_k, **kw)
    return [x.cpu() for x in torch.autograd.grad(out, (qd, kd, vd), g.to(DEV))]


@pytest.mark.parametrize("case", _varlen_cases(), ids=_vname)
def test_bwd_varlen_features(xfa, parity_report, case):
    win, alibi, softcap, det, dtype, d, (h, hk) = case
    causal = win == "causal"
    window = (-1, -1) if causal else win
    gen = torch.Generator().manual_seed(41)
    q = torch.randn(sum(LQ), h, d, generator=gen) * (4 if softcap else 1)
    q = q.to(dtype)
    k, v = (torch.randn(sum(LK), hk, d, generator=gen).to(dtype) for _ in range(2))
    g = torch.randn(sum(LQ), h, d, generator=gen).to(dtype)
    slopes = torch.rand(len(LQ), h, generator=gen) * 0.3 if alibi else None
    kw = dict(causal=causal, window_size=window, softcap=softcap, deterministic=det)
    got = _varlen_run(xfa, q, k, v, g, LQ, LK, max(LQ), max(LK),
                      alibi_slopes=slopes.to(DEV) if alibi else None, **kw)
    cu_q = [0] + list(itertools.accumulate(LQ))
    cu_k = [0] + list(itertools.accumulate(LK))
    refs = bu.ref_grads_varlen(q, k, v, g, cu_q, cu_k, slopes, causal=causal, window_size=window,
                               softcap=softcap)
    # x5 on the global rule where softcap meets ALiBi, as tests/test_bwd_gpu.py
    mult = 5.0 if alibi and softcap else 3.0
    worst = bu.WorstRows()
    try:
        for i, (sq_, sk_) in enumerate(zip(bu.seq_slices(cu_q), bu.seq_slices(cu_k))):
            seq = (got[0][sq_][None], got[1][sk_][None], got[2][sk_][None])
            what = f"varlen {_vname(case)} seq{i}"
            bu.check_grads(what, seq, refs[i], dtype, worst, mult=mult,
                           block_factor={"dq": DQ_PEAKED_BLOCK_FACTOR}
                           if softcap and LQ[i] % bu.BLOCK == 1 else None)
            bu.assert_exact_zeros(what, seq, causal, window)
    finally:
        worst.flush(parity_report)
    for i, (sq_, sk_) in enumerate(zip(bu.seq_slices(cu_q), bu.seq_slices(cu_k))):
        what = f"varlen {_vname(case)} seq{i}"
        # isolation, no tolerance: dK / dV of a key block accumulate over its query tiles in a
        # fixed order that does not depend on the other sequences of the batch (the same
        # max_seqlen bounds are passed, so the window arguments are normalised alike)
        alone = _varlen_run(xfa, q[sq_], k[sk_], v[sk_], g[sq_], [LQ[i]], [LK[i]], max(LQ), max(LK),
                            alibi_slopes=slopes[i:i + 1].to(DEV) if alibi else None, **kw)
        assert torch.equal(alone[1], got[1][sk_]), f"{what}: dk differs when the sequence runs alone"
        assert torch.equal(alone[2], got[2][sk_]), f"{what}: dv differs when the sequence runs alone"


# ---------------------------------------------------------------- dense tile edges -------
def _sk_edges(d):
    bn = 128 if d > 128 else 256
    return [1, 31, 33, bn - 1, bn, bn + 1, 2 * bn + 1]


@pytest.mark.parametrize("sq,dtype", [(1, BF), (31, BF), (32, BF), (33, BF), (1, FP)],
                         ids=["sq1", "sq31", "sq32", "sq33", "sq1-fp16"])
@pytest.mark.parametrize("d", [64, 128, 256])
def test_bwd_tile_edges(xfa, parity_report, d, sq, dtype):
    """b1 h2/hk1, every sk edge x causal x {atomic, deterministic}.  sq = 1 is the backward
    coverage the q1k147 golden fixture (excluded from test_bwd_golden) never gave."""
    h, hk = 2, 1
    worst = bu.WorstRows()
    try:
        _tile_edges(xfa, worst, d, sq, dtype, h, hk)
    finally:
        worst.flush(parity_report)


def _tile_edges(xfa, report, d, sq, dtype, h, hk):
    for sk, causal in itertools.product(_sk_edges(d), (False, True)):
        gen = torch.Generator().manual_seed(1000 * sq + sk)
        q = torch.randn(1, sq, h, d, generator=gen).to(dtype)
        k, v = (torch.randn(1, sk, hk, d, generator=gen).to(dtype) for _ in range(2))
        g = torch.randn(1, sq, h, d, generator=gen).to(dtype)
        refs = bu.ref_grads(q, k, v, g, causal=causal)
        for det in (False, True):
            qd, kd, vd = (x.to(DEV).requires_grad_(True) for x in (q, k, v))
            out = xfa.flash_attn_func(qd, kd, vd, causal=causal, deterministic=det)
            got = [x.cpu() for x in torch.autograd.grad(out, (qd, kd, vd), g.to(DEV))]
            what = "edges d%d %s %dx%d c%d det%d" % (d, str(dtype).split(".")[-1], sq, sk, causal, det)
            bu.check_grads(what, got, refs, dtype, report)
            bu.assert_exact_zeros(what, got, causal)
