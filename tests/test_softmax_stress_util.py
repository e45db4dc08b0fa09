"""CPU: the inputs and pass rules of tests/test_softmax_stress_gpu.py do what they claim.

For every case that file parametrises (the same tables, tests/softmax_stress_util.py):

  * the reference and the low-precision estimate are finite;
  * the precondition of the case's regime holds, so that a pass on the GPU proves the rescale
    branch ran (amp = 40: overflow margin > 128; amp = 4: at least 30 (row, tile) jumps above 8
    and one in (8, 16]; `mixed`: a 32-row group in which some rows jump and some do not);
  * the fault-free tiled-softmax model passes the rules, and each of its deliberate faults is
    rejected by the very rule the GPU case applies.

`desc40` (growing(40) reversed) was meant to give no jump at all.  It does not: the key factor
falls by 15 % from one tile to the next while the max of 64 unit-normal scores varies by about as
much, so some rows still find their max late (sq 150, sk 417, d 64: 224 of 4200 (row, tile) pairs
jump by more than 8).  What holds, and what is asserted here: it jumps far less often than
growing(40) does (under a tenth as often, causal and full), at least half of its rows have
their max in their first visible tile (the no-rescale arm), and some rows' last tile lies more
than 24 log2 units under their max (P underflows even fp16's 2^-24).
"""
import pytest
import torch

from tests import softmax_stress_util as su
from tests.fp8_model import attention_fp8_kernel_model

INPUTS = sorted({su.input_key(c) for c in su.CASES}, key=su.case_id)


def _ids(cs):
    return [su.case_id(c) for c in cs]


def _slacks(c):
    """the fwd_slack values the GPU file runs these inputs at"""
    return sorted({x.slack for x in su.CASES if su.input_key(x) == c})


def _model(c, slack, **kw):
    q, k, v = su.inputs(c)
    sl = su.slopes_of(c)
    bias = None
    if sl is not None:
        # the kernel's causal frame (a per-row constant from the oracle's: the same O)
        bias = su.orc.alibi_bias_kernel(sl, q.shape[1], k.shape[1], causal=c.mask == "causal")
    return su.tiled_softmax_model(q, k, v, su.MASKS[c.mask], slack, softcap=su.softcap_of(c),
                                  bias=bias, **kw)


def test_table_covers_the_cross():
    ids = _ids(su.CASES)
    assert len(set(ids)) == len(ids)
    a = [c for c in su.CASES if c.group == "A"]
    assert len(a) <= 200
    assert {c.d for c in a} == {40, 64, 96, 128, 192, 256}
    for d in (64, 256):                                     # the full cross
        got = {(c.mask, c.pattern, c.slack) for c in a if c.d == d and c.dtype == su.BF and not c.knobs}
        assert len(got) == len(su.MASKS) * len(su.PATTERNS) * len(su.SLACKS)
    assert {dict(c.knobs).get("fwd_pipe", 1) for c in a if c.d == 64} == {0, 1, 2}
    assert {c.slack for c in su.CASES} == {0, 8, 16}


@pytest.mark.parametrize("c", INPUTS, ids=_ids(INPUTS))
def test_references_are_finite(c):
    r = su.case_refs(c)
    assert torch.isfinite(r.ref.float()).all() and torch.isfinite(r.pt.float()).all()
    assert not torch.isnan(r.lse).any()
    assert r.apriori is None or 0 < r.apriori < float("inf")


@pytest.mark.parametrize("c", [c for c in INPUTS if not c.feat], ids=_ids([c for c in INPUTS if not c.feat]))
def test_precondition(c):
    q, k, v = su.inputs(c)
    w = su.MASKS[c.mask]
    m = su.mask_of(w, q.shape[1], k.shape[1])
    top, n8 = su.tile_jumps(q, k, m, 8.0)
    if c.pattern in ("growing40", "late40", "mixed"):
        margin = su._overflow_margin(q, k, False, w)
        assert margin > 128, f"margin {margin:.1f}"
    if c.pattern == "growing4":
        assert n8 >= 30 and su.jumps_between(q, k, m, 8.0, 16.0) >= 1, (n8, top)
    if c.pattern == "mixed":
        assert su.mixed_groups(q, k, m) >= 1
    if c.pattern == "desc40":
        j = su._jumps(q, k, m)                                # NaN: not (yet) visible
        seen = ~torch.isnan(j)
        quiet = ((j > 0) & seen).sum(-1) == 0                 # rows whose first visible tile holds the max
        assert quiet.float().mean().item() >= 0.5
        if c.mask in ("causal", "full"):
            up = su.tile_jumps(*su.apply_pattern("growing40", *su._base(c.b, su.SQ, c.sk, su.H, su.HK, c.d, c.dtype)[:2]), m, 8.0)[1]
            assert n8 * 10 <= up, (n8, up)
        tm = su._tile_max(su._packed_scores(q, k, m))
        run = torch.cummax(tm, -1).values
        deficit = torch.where(torch.isfinite(tm), run - tm, torch.zeros_like(tm))
        assert deficit.max().item() > 24


FEAT = [c for c in INPUTS if c.feat]


@pytest.mark.parametrize("c", FEAT, ids=_ids(FEAT))
def test_precondition_with_score_features(c):
    """after softcap (q x 4) and ALiBi (in the kernels' own form, -slope |row + sk - sq - col|)
    the running max still jumps by more than 8 at 30 (row, tile) pairs or more"""
    q, k, v = su.inputs(c)
    sl = su.slopes_of(c)
    bias = su.orc.alibi_bias(sl, q.shape[1], k.shape[1], causal=False) if sl is not None else None
    m = su.mask_of(su.MASKS[c.mask], q.shape[1], k.shape[1])
    top, n8 = su.tile_jumps(q, k, m, 8.0, su.softcap_of(c), bias)
    assert n8 >= 30, (top, n8)


@pytest.mark.parametrize("c", INPUTS, ids=_ids(INPUTS))
def test_fault_free_model_passes(c):
    r = su.case_refs(c)
    for slack in _slacks(c):
        o, lse = _model(c, slack)
        ok, f = su.judge(o, lse, r)
        assert ok, (slack, f)


AMP40 = [c for c in INPUTS if c.pattern in ("growing40", "late40", "mixed") and "softcap" not in c.feat]


@pytest.mark.parametrize("c", AMP40, ids=_ids(AMP40))
def test_no_rescale_is_rejected(c):
    o, lse = _model(c, 8, fault="no_rescale")
    ok, f = su.judge(o, lse, su.case_refs(c))
    assert not f["finite"] and not ok


AMP4 = [c for c in INPUTS if c.pattern == "growing4" and not c.feat]


@pytest.mark.parametrize("c", AMP4, ids=_ids(AMP4))
def test_alpha_skips_l_is_rejected(c):
    """by the O bound and by the LSE tolerance, each on its own"""
    o, lse = _model(c, 8, fault="alpha_skips_l")
    ok, f = su.judge(o, lse, su.case_refs(c))
    assert not f["o_ok"] and not f["lse_ok"], f


LEFT = [c for c in INPUTS if c.mask in ("w100_17", "w64_0") and not c.feat]


@pytest.mark.parametrize("c", LEFT, ids=_ids(LEFT))
def test_fresh_as_zero_is_rejected(c):
    o, lse = _model(c, 8, fault="fresh_as_zero")
    ok, f = su.judge(o, lse, su.case_refs(c))
    assert not ok, f


@pytest.mark.parametrize("d", [64, 128])
def test_fp16_edge_of_slack(d):
    """fp16 and fwd_slack = 16.  The rescale keeps P within 2^slack, and 2^16 does not fit fp16:
    P >= 65520 rounds to inf.  That needs a lag inside (15.9996, 16], which random inputs do not
    hold (so the random slack-16 cases cannot tell), hence one built input (su.fp16_edge_inputs).
    On it the model is non-finite at slack 16 and passes at 15, the limit the launch applies.
    `p_saturates` at the fp16 maximum passes as well: clamping 65528 to 65504 is under half an
    fp16 ulp, so saturation would be harmless - the overflow to inf is the defect."""
    q, k, v = su.fp16_edge_inputs(d)
    r = su.refs(q, k, v)
    assert su.tile_jumps(q, k, None, 8.0)[1] == 1             # the built jump and no other
    o, lse = su.tiled_softmax_model(q, k, v, slack=16)
    ok, f = su.judge(o, lse, r)
    assert not f["finite"] and not ok
    for kw in (dict(slack=15), dict(slack=8), dict(slack=16, fault="p_saturates", p_limit=65504.0)):
        ok, f = su.judge(*su.tiled_softmax_model(q, k, v, **kw), r)
        assert ok, (kw, f)


# ------------------------------------------------------------------------------- fp8 ---------
FP8_INPUTS = sorted({(c.kind, c.pattern, c.mask, c.out) for c in su.FP8_CASES}, key=str)


def _fp8_figures(kind, pattern, mask, out, slack, clamp=True):
    """per problem of the case: (model_err, pt_err, bound) of the 4-wave kernel's model"""
    probs, (qs, ks, vs) = su.fp8_problems(su.Fp8Case(kind, pattern, mask, out, slack, ()))
    rows = []
    for q8, k8, v8 in probs:
        w = su.MASKS[mask]
        r = su.fp8_refs(q8, k8, v8, qs, ks, vs, w, out)
        sk = k8.shape[1]
        ww = (w[0], sk) if w[0] >= 0 and w[1] < 0 else w
        mdl = attention_fp8_kernel_model(q8, k8, v8, qs, ks, vs, window_size=ww, slack=slack,
                                         clamp_slack=clamp).to(out)
        err = (mdl.float() - r.ref.float()).abs().max().item()
        pt_err = (r.pt.float() - r.ref.float()).abs().max().item()
        rows.append((err, pt_err, 3 * pt_err + 1e-3, bool(torch.isfinite(mdl.float()).all())))
    return rows


@pytest.mark.parametrize("kind,pattern,mask,out", FP8_INPUTS, ids=[f"{a}-{b}-{c}-{str(d)[6:]}" for a, b, c, d in FP8_INPUTS])
def test_fp8_inputs_leave_room(kind, pattern, mask, out):
    """a condition on the inputs, not a tolerance: the kernel's own arithmetic (the model at
    slack 0 and 8) stays within 0.8 of the project's fp8 bound, which is tight on peaked rows"""
    for slack in (0, 8):
        for err, pt_err, bound, fin in _fp8_figures(kind, pattern, mask, out, slack):
            print(f"slack {slack}: model err {err:.4f} pt err {pt_err:.4f} bound {bound:.4f}")
            assert fin and err <= 0.8 * bound, (slack, err, bound)


@pytest.mark.parametrize("kind,pattern,mask,out", FP8_INPUTS, ids=[f"{a}-{b}-{c}-{str(d)[6:]}" for a, b, c, d in FP8_INPUTS])
def test_fp8_unclamped_slack16_is_rejected(kind, pattern, mask, out):
    """slack 16 without the limit of 8: P passes 448 and the e4m3 conversion has nothing finite
    to give; the fp8 rule rejects it in at least one problem of the case"""
    rows = _fp8_figures(kind, pattern, mask, out, 16, clamp=False)
    assert any(not fin or err > bound for err, _, bound, fin in rows), rows


@pytest.mark.parametrize("kind,pattern,mask,out", FP8_INPUTS, ids=[f"{a}-{b}-{c}-{str(d)[6:]}" for a, b, c, d in FP8_INPUTS])
def test_p_saturates_is_rejected_fp8(kind, pattern, mask, out):
    """the tiled model over the dequantised inputs with P in e4m3: clean at slack 8 it passes the
    fp8 rule; at slack 16 with P clamped at 448 (a saturating conversion) it does not"""
    probs, (qs, ks, vs) = su.fp8_problems(su.Fp8Case(kind, pattern, mask, out, 16, ()))
    bad = 0
    for q8, k8, v8 in probs:
        w = su.MASKS[mask]
        r = su.fp8_refs(q8, k8, v8, qs, ks, vs, w, out)
        x = [q8.float() * qs, k8.float() * ks, v8.float() * vs]
        ww = (w[0], k8.shape[1]) if w[0] >= 0 and w[1] < 0 else w
        o, lse = su.tiled_softmax_model(*x, ww, 8, p_dtype=su.F8)
        assert su.judge(o.to(out), lse, r, 3.0, 1e-3)[0]
        o, lse = su.tiled_softmax_model(*x, ww, 16, fault="p_saturates", p_limit=448.0, p_dtype=su.F8)
        bad += not su.judge(o.to(out), lse, r, 3.0, 1e-3)[0]
    assert bad >= 1


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("pattern", ["growing40", "late40"])
@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_decode_caches(fp8, pattern, d):
    """the decode caches: the exact cache values (what the kernel is defined over) keep the
    overflow margin of their pattern, and the oracle over them is finite"""
    from tests import decode_util as du
    c, q = su.decode_problem(d, fp8, pattern)
    for i, kx in enumerate(c.kx):
        margin = su._overflow_margin(q[i:i + 1], kx[None], False)
        # late_step: one query row and 9 stepped keys; the step must pass the default slack
        assert margin > (128 if pattern == "growing40" else 8), f"seq {i}: margin {margin:.1f}"
    ora = du.oracle(c, q)
    assert torch.isfinite(ora.ref.float()).all() and torch.isfinite(ora.pt.float()).all()


def test_packed_and_cache_inputs_of_group_b():
    """the packed sequences with 2 tiles or more, and the leftpad / paged caches, keep the margin"""
    from tests import decode_util as du
    for n in (200, 417):
        q, k = su._randn((1, n, su.H, 64), 1, su.BF), su._growing(su._randn((1, n, su.HK, 64), 2, su.BF), 40.0)
        assert su._overflow_margin(q, k, True) > 128, n
    c = su.grown_cache([417, 300], 64, su.BF, False, "growing40", 432, 1, leftpad=[5, 23])
    q = du.make_q(2, su.SQ, su.H, 64, su.BF, 81)
    for i, kx in enumerate(c.kx):
        assert su._overflow_margin(q[i:i + 1], kx[None], True) > 128


@pytest.mark.parametrize("d", [64, 128])
def test_unit_randn_never_leaves_the_no_rescale_regime(d):
    """why these tests exist: under unit randn q and k no (row, tile) pair jumps by more than the
    default slack of 8 log2 units (measured 3.9), so the rest of the suite never rescales"""
    q, k = su._randn((2, 512, 4, d), 1, su.BF), su._randn((2, 2048, 4, d), 2, su.BF)
    top, n8 = su.tile_jumps(q, k, None, 8.0)
    print(f"d {d}: largest jump {top:.2f}")
    assert 2.0 < top < 6.0 and n8 == 0
