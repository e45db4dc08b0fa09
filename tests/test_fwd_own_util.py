"""CPU: the builders, the case table and the conditions of the forward ownership tests
(tests/fwd_own_util.py, tests/test_fwd_own_gpu.py).

The planted defects.  `model_launch` is a tiled forward that reads whole 64-key tiles and whole
32-row tiles from the arenas; each defect is run under the three fills and conditions 1 - 3 of
`judge_case` must reject it.  Which (fill, condition) pairs do (asserted below, `CATCHES`):

  defect         problem                       zero    nan       big
  v_tail         dense d40 (33, 65) causal     -       1, 2      -
  v_tail         packed d64, seqused_k         -       1, 2      -
  slot_limit     packed d64, seqused_k         1       1, 2      1, 2
  slot_limit     one-page cache with leftpad   1       1, 2      1, 2
  k_bucket       dense d40 (33, 65) causal     -       1, 2      -
  leftpad_rows   one-page cache with leftpad   1       1, 2      1, 2
  o_tile         dense d40 (33, 65) causal     -       3         3
  stale_partial  dense d64 (70, 200) causal,   -       1, 2      1, 2
                 5 -> 4 splits

`zero` is the run the other two are compared with and the one in which a stray read changes least:
alone it rejects only a wrong key limit, and only because these problems hold rows that must see
no key (condition 1: their LSE is +inf and their O is 0; extra keys, even zero ones, make the LSE
finite).  `nan` shows a poison element that meets a zero weight
(0 x NaN: v_tail, k_bucket), which `big` cannot (0 x max = 0).  `big` and `nan` both show a stray
store of zeros (o_tile), which `zero` cannot, and rows past the limit taken for keys (slot_limit,
leftpad_rows).  No defect of this model is caught by `big` alone: it is kept for what the model
does not have and the kernels do - operations that drop a NaN and keep a finite value (the
hardware max of the row-max chain, the clamp and conversion of an fp8 operand).
"""
import itertools
from collections import Counter

import pytest
import torch

from tests import fwd_own_util as fu
from tests.softmax_stress_util import BF, FP

ALL = fu.CASES + fu.SPLIT_CASES


def _ids(cases):
    return [fu.case_id(c) for c in cases]


# ---------------------------------------------------------------- the table -------------------
def test_table_size_and_ids():
    assert len(fu.CASES) == 153 and len(fu.SPLIT_CASES) == 9 and len(fu.ISOLATION) == 6
    assert Counter(c.group for c in fu.CASES) == dict(A=99, B=22, C=11, D=14, E=7)
    assert len(set(_ids(ALL))) == len(ALL)
    assert 100 <= len(ALL) < 300                       # "the low hundreds"


def test_every_listed_instantiation_is_asserted():
    """A: the 16 (NW, MASK, FEAT, sink) instantiations of the 64 and 128 buckets and the 8 of the
    256 bucket, in both dtypes, each named by a case (the GPU test asserts the name, the wave
    count, the sink mechanism; MASK and FEAT follow from the launch, fmha_fwd.hip launch_fwd_nw)"""
    have = Counter((c.inst, c.dtype) for c in fu.CASES if c.group == "A")
    for hd in (64, 128, 256):
        for nw in ((4, 8) if hd < 256 else (4,)):
            for m, f, s in itertools.product((False, True), repeat=3):
                for dt in (BF, FP):
                    assert have[((hd, nw, m, f, s), dt)] >= 1, (hd, nw, m, f, s, dt)
    for c in fu.CASES:
        if c.group != "A":
            continue
        hd, nw, m, f, s = c.inst
        assert fu.bucket(c.d) == hd and c.kernel == f"fmha_fwd_kernel<{nw} waves>"
        assert dict(c.knobs).get("fwd_waves", 4) == nw or hd == 256
        assert m == (c.mask != "full") and f == bool(c.feat) and s == c.sink
        assert hd != 128 or dict(c.knobs)["fwd_w4"] == 0
        assert not (c.sink and "alibi" in c.feat)      # the entry refuses the pair
    # narrower head sizes of every bucket, 160 once, fwd_pipe x masks
    ds = Counter(c.d for c in fu.CASES if c.group == "A")
    assert all(ds[d] >= 1 for d in (40, 64, 96, 128, 192, 256)) and ds[160] == 1
    pipes = {(fu.bucket(c.d), dict(c.knobs)["fwd_pipe"], c.mask) for c in fu.CASES if "pipe" in c.extra}
    assert pipes == set(itertools.product((64, 128), (0, 1, 2), fu.MASKS3))
    shapes = {c.shape for c in fu.CASES if c.group == "A"}
    assert shapes == set(fu.SHAPES)
    assert {c.hk for c in fu.CASES if c.group == "A"} == {1, 2}


def test_every_listed_body_is_asserted():
    have = Counter((c.kernel, c.body, c.entry, c.dtype) for c in fu.CASES if c.group == "B")
    for dt in (BF, FP):
        for entry in ("strided", "varlen"):
            for kern, body in (("fmha_fwdpp_kernel", "plain"), ("fmha_fwdpp_kernel", "full"),
                               ("fmha_fwdpp16_kernel", None), ("fmha_fwd4_kernel", None)):
                assert have[(kern, body, entry, dt)] >= 1, (kern, body, entry, dt)
        for entry in ("varlen_paged", "cache_paged"):
            assert have[("fmha_fwdpp_paged_kernel", "paged", entry, dt)] >= 1
    b = [c for c in fu.CASES if c.group == "B"]
    assert {(c.mask, c.feat) for c in b if c.body == "plain"} == {("causal", ""), ("w-1_17", "")}
    assert {(c.mask, c.feat) for c in b if c.body == "full"} == {("w64_0", ""), ("causal", "alibi"),
                                                                 ("causal", "softcap")}
    # a left window is in effect only where it is shorter than the keys
    assert all(c.shape[1] > 64 for c in b if c.mask == "w64_0" and c.entry == "strided")
    e = Counter(c.kernel for c in fu.CASES if c.group == "E")
    assert e["fmha_fwd8w_kernel"] >= 2 and e["fmha_fwd_fp8_kernel<8 waves>"] >= 2
    d = [c for c in fu.CASES if c.group == "D"]
    assert {c.d for c in d if c.entry == "cache_paged" and "fp8" not in c.extra} == {64, 256}
    assert {c.d for c in d if "fp8" in c.extra} == {64, 128}
    assert {("leftpad" in c.extra) for c in d if c.entry == "cache"} == {True, False}
    f = fu.SPLIT_CASES
    plain = [c for c in f if not c.sink]
    assert {(c.d, c.splits, c.mask) for c in plain} == set(itertools.product((64, 128), (2, 5), ("full", "causal")))
    for axis in ("d", "splits", "mask"):               # comb_row 0 and 1 with every value of each
        assert {(getattr(c, axis), dict(c.knobs)["comb_row"]) for c in plain} == set(
            itertools.product({getattr(c, axis) for c in plain}, (0, 1)))
    assert sum(c.sink for c in f) == 1
    assert {fu.expected_splits(c) for c in f} == {2, 4, 5}
    # prefill, not decode: more than one 32-row tile of GQA-packed rows
    assert all(c.shape[0] * (fu.H // c.hk) > 32 for c in d + f)
    assert {c.d for c in fu.CASES if c.group == "C" and c.entry == "varlen"} == {64, 128, 256}
    assert len({c.kernel + str(c.body) for c in fu.ISOLATION}) == 4


# ---------------------------------------------------------------- the builders ----------------
def _check_arena(a: fu.Arena, want, fill, dtype, rows_owned=None):
    """the view round-trips, the owned mask is exactly the view (or its owned rows), everything
    else holds the fill"""
    v = fu.view(a)
    if rows_owned is None:
        assert torch.equal(fu._bits(v), fu._bits(want))
        assert int(a.owned.sum()) == v.numel()
    else:
        assert torch.equal(fu._bits(v[:, rows_owned]), fu._bits(want[None][:, rows_owned]))
        assert int(a.owned.sum()) == v[:, rows_owned].numel()
    assert fu.view(a, a.owned).sum() == a.owned.sum()
    pool = fu._fill(1, dtype, fill)
    assert bool((fu._bits(a.buf)[~a.owned] == fu._bits(pool)[0]).all())


def _check_margins(a: fu.Arena, strided, d):
    n = a.buf.numel()
    b, rows, heads, _ = a.shape
    row = a.strides[1]
    first = a.base
    last = a.base + (b - 1) * a.strides[0] + (rows - 1) * row
    assert first >= fu.FRONT * row and last + fu.BACK * row + row <= n
    if strided:
        assert a.strides[2] >= fu.bucket(d) and a.strides[2] > d           # pitch
        assert row >= (heads + 1) * a.strides[2]                           # one spare head
        # every batch has its own margins
        assert a.strides[0] >= (fu.FRONT + rows + fu.BACK) * row
    assert all(s % 8 == 0 for s in a.strides[:3])
    assert a.base % 8 == 0


@pytest.mark.parametrize("c", ALL, ids=_ids(ALL))
def test_builder(c):
    fill = fu.FILLS[len(fu.case_id(c)) % 3]
    p = fu.build(c, fill)
    q = p.data[0]
    strided = c.entry == "strided"
    kv_dtype = fu.F8 if p.fp8 else c.dtype
    _check_arena(p.q, q if q.dim() == 4 else q[None], fill, kv_dtype)
    _check_margins(p.q, strided, c.d)
    _check_margins(p.o, strided, c.d)
    assert torch.isnan(fu.view(p.o).float()).all() and torch.isnan(fu.view(p.lse)).all()
    assert int(p.o.owned.sum()) == fu.view(p.o).numel()
    assert p.o.shape == p.q.shape and p.o.strides == p.q.strides
    assert p.lse.base == fu.LSE_GUARD and p.lse.buf.numel() == fu.view(p.lse).numel() + 2 * fu.LSE_GUARD
    if p.cache is None:
        own = None if strided else fu._own_k_rows(p.lq, p.lk, p.used)
        for a, x in ((p.k, p.data[1]), (p.v, p.data[2])):
            _check_arena(a, x, fill, kv_dtype, own)
            _check_margins(a, strided, c.d)
        assert p.k.strides == p.v.strides              # the generated D = 128 bodies need it
    else:
        t = p.cache
        assert int(t.table.min()) >= 0 and int(t.table.max()) < t.kc.shape[0]
        assert all(0 <= n <= t.width * t.page for n in t.lens)
        if t.leftpad is not None:
            assert all(0 <= l <= n for l, n in zip(t.leftpad, t.lens))
    if not strided and p.cache is None or c.entry == "varlen_paged":
        assert len(p.lq) == len(p.lk) == len(p.used) == p.b
        assert all(0 <= u <= n for u, n in zip(p.used, p.lk))
        assert max(p.lq) <= p.max_sq and max(p.used) <= p.max_sk
        assert 0 in p.lq and 0 in p.used               # a sequence without queries, one without keys


def test_packed_isolation_problem():
    c = fu.ISOLATION[0]
    full, one = fu.build(c, "nan"), fu.build(c, "nan", only=2)
    sl = slice(sum(fu.LQ[:2]), sum(fu.LQ[:3]))
    assert torch.equal(fu.view(one.q)[0], fu.view(full.q)[0, sl])
    assert (one.lq, one.lk, one.used) == ([300], [300], [257])
    assert (one.max_sq, one.max_sk) == (full.max_sq, full.max_sk)


# ---------------------------------------------------------------- the planted defects ---------
M_DENSE = fu._case("M", "strided", 40, BF, 2, (33, 65), "causal")
M_PACKED = fu._case("M", "varlen", 64, FP, 2, (), "w100_17")
M_CACHE = fu._case("M", "cache", 64, BF, 2, (33,), "causal", extra=("leftpad",))
M_SPLIT = fu._case("M", "strided", 64, BF, 2, (70, 200), "causal", splits=5)
MODEL_CASES = (M_DENSE, M_PACKED, M_CACHE, M_SPLIT)

N12 = {("nan", 1), ("nan", 2)}
NB12 = N12 | {("big", 1), ("big", 2)}
ZNB = NB12 | {("zero", 1)}
CATCHES = [
    ("v_tail", M_DENSE, N12),
    ("v_tail", M_PACKED, N12),
    ("slot_limit", M_PACKED, ZNB),
    ("slot_limit", M_CACHE, ZNB),
    ("k_bucket", M_DENSE, N12),
    ("leftpad_rows", M_CACHE, ZNB),
    ("o_tile", M_DENSE, {("nan", 3), ("big", 3)}),
    ("stale_partial", M_SPLIT, NB12),
]


def _judge(c, defect):
    probs = {f: fu.build(c, f) for f in fu.FILLS}
    outs = {f: fu.model_launch(probs[f], defect) for f in fu.FILLS}
    return fu.judge_case(c, probs, outs, fu.oracle(c))


@pytest.mark.parametrize("c", MODEL_CASES, ids=_ids(MODEL_CASES))
def test_correct_model_passes(c):
    assert _judge(c, None) == []


@pytest.mark.parametrize("defect,c,want", CATCHES, ids=[f"{d}-{fu.case_id(c)}" for d, c, _ in CATCHES])
def test_planted_defect_is_rejected(defect, c, want):
    fails = _judge(c, defect)
    got = {(fill, cond) for fill, cond, _ in fails if cond <= 3}
    print(defect, fu.case_id(c), sorted(got), [f for f in fails if f[1] > 3])
    assert got, f"{defect} passes conditions 1 - 3 under every fill"
    assert got == want


def test_every_defect_is_planted():
    assert {d for d, _, _ in CATCHES} == set(fu.DEFECTS)


def test_wrong_kernel_is_rejected():
    """condition 5: a launch that ran another body fails whatever it computed"""
    c = M_DENSE
    probs = {f: fu.build(c, f) for f in fu.FILLS}
    outs = {f: fu.model_launch(probs[f])._replace(kern="fmha_fwdpp_kernel persistent=0 body=plain")
            for f in fu.FILLS}
    assert {cond for _, cond, _ in fu.judge_case(c, probs, outs, fu.oracle(c))} == {5}
    outs = {f: fu.model_launch(probs[f])._replace(splits=2) for f in fu.FILLS}
    assert {cond for _, cond, _ in fu.judge_case(c, probs, outs, fu.oracle(c))} == {5}
