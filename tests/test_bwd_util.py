"""CPU checks of the backward tests' own rule (tests/bwd_util.py): an emulated correct kernel
(fp32 accumulation, P / dS rounded to the dtype) passes `check_grads`, every planted tiling defect
fails it, and the instance table covers every instance csrc/fmha_bwd.hip dispatches."""
import itertools

import pytest
import torch

from oracle import attention_ref as orc
from tests import bwd_util as bu


def _inputs(dtype, sq, sk, h, hk, d, seed=0, b=1):
    gen = torch.Generator().manual_seed(seed)
    q = torch.randn(b, sq, h, d, generator=gen).to(dtype)
    k = torch.randn(b, sk, hk, d, generator=gen).to(dtype)
    v = torch.randn(b, sk, hk, d, generator=gen).to(dtype)
    g = torch.randn(b, sq, h, d, generator=gen).to(dtype)
    return q, k, v, g


CASES = {
    # name: (dtype, sq, sk, h, hk, d, causal, window, defect)
    "dk_block": (torch.float16, 113, 600, 4, 2, 64, False, (-1, -1)),
    "dq_tail": (torch.bfloat16, 113, 600, 4, 2, 128, False, (-1, -1)),
    "dq_twice": (torch.bfloat16, 113, 600, 4, 2, 64, False, (100, 30)),
    "dv_lastkey": (torch.bfloat16, 300, 300, 4, 1, 128, True, (-1, -1)),
}


@pytest.fixture(scope="module")
def problems():
    res = {}
    for name, (dtype, sq, sk, h, hk, d, causal, window) in CASES.items():
        q, k, v, g = _inputs(dtype, sq, sk, h, hk, d)
        refs = bu.ref_grads(q, k, v, g, causal=causal, window_size=window)
        res[name] = (q, k, v, g, refs)
    return res


@pytest.mark.parametrize("name", list(CASES))
def test_clean_emulation_passes(problems, name):
    dtype, *_, causal, window = CASES[name]
    q, k, v, g, refs = problems[name]
    rows = []
    bu.check_grads(name, bu.emulate_bwd(q, k, v, g, causal, window), refs, dtype, rows.append)
    assert len(rows) == 6 and all(r["err"] <= r["bound"] for r in rows)
    bu.assert_exact_zeros(name, bu.emulate_bwd(q, k, v, g, causal, window), causal, window)


@pytest.mark.parametrize("name", list(CASES))
def test_planted_defect_fails(problems, name):
    dtype, *_, causal, window = CASES[name]
    q, k, v, g, refs = problems[name]
    got = bu.emulate_bwd(q, k, v, g, causal, window, defect=name)
    with pytest.raises(AssertionError, match="block"):
        bu.check_grads(name, got, refs, dtype)


def test_lost_last_key_passes_the_global_rule_alone(problems):
    """The defect that motivates the block rule: dV without the last key's P column (causal
    300 x 300, h4/hk1, d128, bf16) sits where gradients are small and meets the global rule."""
    q, k, v, g, refs = problems["dv_lastkey"]
    got = bu.emulate_bwd(q, k, v, g, True, (-1, -1), defect="dv_lastkey")
    ok, err, bound = orc.parity_ok(got[2], refs.ref[2], refs.pt[2], 3.0, 1e-5)
    assert ok, (err, bound)
    ratio, _, _, where = bu.block_rule(got[2], refs.ref64[2], refs.pt[2], torch.bfloat16)
    assert ratio > 1.0 and where[1] == 299 // bu.BLOCK


def test_stored_o_rounding_on_peaked_rows():
    """Why tests/test_bwd_varlen_features_gpu.py widens the dQ block bound of its softcap cases:
    on a one-row block whose softmax is peaked (P_max = 0.99) a correct kernel, which takes
    D = rowsum(dO * O) from the stored (rounded) O, exceeds the block rule many times; with D
    from the unrounded O it passes.  Sequence 0 (1 x 147) of that test's
    w100_0-alibi-softcap-float16-d64-h8_1 case."""
    lq, lk, h, d, dtype = [1, 33, 300, 77, 130], [147, 20, 300, 600, 64], 8, 64, torch.float16
    gen = torch.Generator().manual_seed(41)
    q = (torch.randn(sum(lq), h, d, generator=gen) * 4).to(dtype)[:1][None]
    k, v = (torch.randn(sum(lk), 1, d, generator=gen).to(dtype)[:147][None] for _ in range(2))
    g = torch.randn(sum(lq), h, d, generator=gen).to(dtype)[:1][None]
    slopes = (torch.rand(len(lq), h, generator=gen) * 0.3)[:1]
    bias = orc.alibi_bias(slopes, 1, 147, causal=False)
    refs = bu.ref_grads(q, k, v, g, window_size=(100, 0), softcap=20.0, attn_bias=bias)
    ratios = []
    for exact in (False, True):
        got = bu.emulate_bwd(q, k, v, g, False, (100, 0), softcap=20.0, attn_bias=bias, exact_d=exact)
        ratios.append(bu.block_rule(got[0], refs.ref64[0], refs.pt[0], dtype)[0])
    assert ratios[0] > 5.0 and ratios[1] < 1.0, ratios


def test_exact_zeros_helper():
    # causal sq > sk: the first sq - sk rows see no key; window (16, 8) at 40 x 300: keys before
    # 300 - 40 - 16 are seen by no row
    rows, keys = bu.visibility(513, 300, causal=True)
    assert rows.sum().item() == 300 and not rows[:213].any() and keys.all()
    rows, keys = bu.visibility(40, 300, window=(16, 8))
    assert rows.all() and not keys[:244].any() and keys[244:].all()
    rows, keys = bu.visibility(5, 0)
    assert not rows.any() and keys.numel() == 0
    q, k, v, g = _inputs(torch.bfloat16, 40, 300, 2, 1, 64)
    got = list(bu.emulate_bwd(q, k, v, g, False, (16, 8)))
    bu.assert_exact_zeros("clean", got, window=(16, 8))
    got[1] = got[1].clone()
    got[1][0, 3, 0, 5] = 1e-3
    with pytest.raises(AssertionError, match="dk"):
        bu.assert_exact_zeros("dirty", got, window=(16, 8))
    got[1][0, 3, 0, 5] = float("nan")
    with pytest.raises(AssertionError):
        bu.assert_exact_zeros("nan", got, window=(16, 8))


def test_varlen_refs_handle_empty_sequences():
    lq, lk = [3, 0, 5], [4, 7, 0]
    gen = torch.Generator().manual_seed(1)
    q, g = (torch.randn(sum(lq), 2, 64, generator=gen).bfloat16() for _ in range(2))
    k, v = (torch.randn(sum(lk), 1, 64, generator=gen).bfloat16() for _ in range(2))
    cu_q = [0] + list(itertools.accumulate(lq))
    cu_k = [0] + list(itertools.accumulate(lk))
    refs = bu.ref_grads_varlen(q, k, v, g, cu_q, cu_k, causal=True)
    assert [r.ref64[0].shape[1] for r in refs] == lq and [r.ref64[1].shape[1] for r in refs] == lk
    assert refs[0].ref64[0].dtype == torch.float64 and refs[0].ref64[0].abs().sum() > 0
    assert refs[1].ref64[1].abs().sum() == 0 and refs[2].ref64[0].abs().sum() == 0
    for r in refs:
        assert all(torch.isfinite(x).all() for x in r.ref64)


def test_instance_table_is_complete():
    table = bu.instance_table()
    keys = {(bu.bucket(t.d), t.dtype, t.mask, t.feat, t.det) for t in table}
    want = set(itertools.product((64, 128, 256), (torch.bfloat16, torch.float16), (False, True),
                                 (False, True), (False, True)))
    assert keys == want and len(table) == 48
    for t in table:
        assert t.mask == (t.causal or t.window != (-1, -1)) and not (t.causal and t.window != (-1, -1))
    # both mask kinds reach every (feat, det) pair
    for feat, det in itertools.product((False, True), repeat=2):
        kinds = {t.causal for t in table if t.mask and t.feat == feat and t.det == det}
        assert kinds == {False, True}
