"""The backward through the C ABI on poisoned memory: every operand (workspace and cu_seqlens
included) is an interior slice of a byte arena filled with 0xFF (NaN in every fp32 / 16-bit lane)
with 4 KiB guards around it (tests/bwd_util.py Arena).  Each case runs with the workspace filled
with 0xFF and with 0x00:

* deterministic: dq / dk / dv bit-identical under both fills (the slices are initialised by their
  own walk, never read before written), guards intact, every output element written, oracle rules;
* atomic: dk / dv bit-identical, dq finite and within the oracle rules, guards intact.

Deterministic runs use workspaces of 1, 2 and the device's own number of dQ slices: 1 and 2 make
one workgroup walk several key blocks at tiny b * hk (the read-modify-write path and the snake
order of fmha_bwd_kernel)."""
import functools
import itertools

import pytest
import torch

from tests import bwd_util as bu

pytestmark = pytest.mark.gpu

BF, FP = torch.bfloat16, torch.float16
# name: (b, sq, sk, h, hk, d, dtype, causal, window)
DENSE = {
    "300x1100-d64-bf16": (2, 300, 1100, 2, 1, 64, BF, False, (-1, -1)),
    "300x1100-d64-fp16": (2, 300, 1100, 2, 1, 64, FP, False, (-1, -1)),
    "300x1100-d128-bf16": (2, 300, 1100, 2, 1, 128, BF, False, (-1, -1)),
    "300x1100-d128-fp16": (2, 300, 1100, 2, 1, 128, FP, False, (-1, -1)),
    # late key blocks start at a query tile t_lo > 0
    "77x600-w100_30-d128": (1, 77, 600, 4, 1, 128, BF, False, (100, 30)),
    # sq > sk: the first 213 rows see no key
    "513x300-causal-d64": (2, 513, 300, 2, 2, 64, BF, True, (-1, -1)),
    # the first key block is seen by no row: its dk / dv are written as zeros
    "40x300-w16_8-d128": (1, 40, 300, 2, 1, 128, FP, False, (16, 8)),
    # padded head dims: slice columns >= d are never written
    "113x600-causal-d40": (1, 113, 600, 4, 2, 40, BF, True, (-1, -1)),
    "113x600-causal-d104": (1, 113, 600, 4, 2, 104, FP, True, (-1, -1)),
    # the 256 bucket: float atomics into the slices
    "77x300-d256": (1, 77, 300, 2, 1, 256, BF, False, (-1, -1)),
}
MODES = {"atomic": (False, None), "det1": (True, 1), "det2": (True, 2), "det_dev": (True, None)}

# varlen: a sequence shorter than one key block while max_seqlen_k gives several slices (a slice's
# first block lies past its end), an empty-query and an empty-key sequence
VL_Q, VL_K = [1, 300, 0, 77, 200], [147, 20, 64, 600, 0]


@functools.lru_cache(maxsize=None)
def _dense(name):
    b, sq, sk, h, hk, d, dtype, causal, window = DENSE[name]
    gen = torch.Generator().manual_seed(31)
    q = torch.randn(b, sq, h, d, generator=gen).to(dtype)
    k = torch.randn(b, sk, hk, d, generator=gen).to(dtype)
    v = torch.randn(b, sk, hk, d, generator=gen).to(dtype)
    g = torch.randn(b, sq, h, d, generator=gen).to(dtype)
    return (q, k, v, g), bu.ref_grads(q, k, v, g, causal=causal, window_size=window)


@functools.lru_cache(maxsize=None)
def _varlen(causal):
    h, hk, d = 4, 2, 128
    gen = torch.Generator().manual_seed(32)
    q, g = (torch.randn(sum(VL_Q), h, d, generator=gen).bfloat16() for _ in range(2))
    k, v = (torch.randn(sum(VL_K), hk, d, generator=gen).bfloat16() for _ in range(2))
    cu_q = [0] + list(itertools.accumulate(VL_Q))
    cu_k = [0] + list(itertools.accumulate(VL_K))
    return (q, k, v, g), (cu_q, cu_k), bu.ref_grads_varlen(q, k, v, g, cu_q, cu_k, causal=causal)


@pytest.fixture(scope="module")
def xfa():
    import xf_flash_attention_cutlass_amd as m
    return m


def _compare_fills(mode, poisoned, zeroed):
    for nm, x, y in zip(bu.NAMES, poisoned, zeroed):
        if nm == "dq" and mode == "atomic":
            continue                    # float atomics: the summation order is not fixed
        assert torch.equal(x, y), f"{nm} depends on what the workspace held before the call"


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", list(DENSE))
def test_bwd_dirty_workspace(xfa, parity_report, name, mode):
    *_, dtype, causal, window = DENSE[name]
    det, n = MODES[mode]
    (q, k, v, g), refs = _dense(name)
    runs = [bu.capi_bwd(xfa, q, k, v, g, causal=causal, window=window, deterministic=det,
                        n_slices=n, ws_fill=fill) for fill in (0xFF, 0x00)]
    _compare_fills(mode, *runs)
    for fill, got in zip(("ff", "00"), runs):
        bu.check_grads(f"workspace {name} {mode} fill{fill}", got, refs, dtype, parity_report)
        bu.assert_exact_zeros(f"{name} {mode}", got, causal, window)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("causal", [False, True])
def test_bwd_dirty_workspace_varlen(xfa, parity_report, causal, mode):
    det, n = MODES[mode]
    (q, k, v, g), (cu_q, cu_k), refs = _varlen(causal)
    runs = [bu.capi_varlen_bwd(xfa, q, k, v, g, VL_Q, VL_K, causal=causal, deterministic=det,
                               n_slices=n, ws_fill=fill) for fill in (0xFF, 0x00)]
    _compare_fills(mode, *runs)
    worst = bu.WorstRows()
    try:
        for fill, got in zip(("ff", "00"), runs):
            for i, (sq_, sk_) in enumerate(zip(bu.seq_slices(cu_q), bu.seq_slices(cu_k))):
                seq = (got[0][sq_][None], got[1][sk_][None], got[2][sk_][None])
                what = f"workspace varlen c{int(causal)} {mode} fill{fill} seq{i}"
                bu.check_grads(what, seq, refs[i], torch.bfloat16, worst)
                bu.assert_exact_zeros(what, seq, causal)
    finally:
        worst.flush(parity_report)
