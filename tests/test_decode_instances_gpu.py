"""Every instance of csrc/fmha_decode_kernel.h — head size {64, 128} x dtype x {16-bit, fp8 cache} x
{16, 32} rows x {4, 8} waves — under each of its five wave-to-work mappings (dec_hmaj 0 / 1 / 2,
dec_bal over dec_hmaj 1 / 2), through fmha_page_kvcache_fwd_ex on ragged paged caches (page 16,
permuted table) whose every byte the kernel must not depend on is poisoned: rows past a sequence's
end, rows in front of its leftpad, unnamed pages (tests/decode_util.py build_cache).

Pass rule (decode_util.judge): no NaN left in O or LSE; max|o - ref| <= 3 max|pt - ref| + 1e-5 (the
project's kvcache rule; 5x with softcap as tests/test_fwd_gpu.py's decode feature test); LSE within
1e-3 of the oracle with the same +inf pattern.  The oracle runs over the exact cache values
float32(stored) * scale.  run_decode asserts the kernel name (rows, 8 heads) and the launch grid,
so no case can silently run another kernel.  tests/test_decode_util.py shows on the CPU that these
shapes catch a V tail, a K tail, a lost tile, a page mix-up, a lost scale and a wrong combine
count.
"""
import pytest
import torch

from oracle import attention_ref as orc
from tests import decode_util as du

pytestmark = pytest.mark.gpu
DEV = "cuda"
BASE = du.BASE_KNOBS


def _run(c, q, plan, knobs=None, **kw):
    return du.run_decode(c, q, plan["num_splits"], knobs or plan["knobs"],
                         kw.pop("mr", 16 if plan["sq"] * plan["group"] <= 16 else 32),
                         heads8=plan["heads8"], want_grid=plan["grid"], **kw)


def _same(a, b):
    """Bit-identical (NaN payloads included)."""
    return a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8).flatten(),
                                              b.contiguous().view(torch.uint8).flatten())


# ---------------------------------------------------------------- (a) every instance -----
@pytest.mark.parametrize("t", du.instance_table(), ids=du.instance_name)
def test_decode_instance(parity_report, t):
    c, q, plan = du.instance_problem(t, "nan")
    o, lse, kern, splits = _run(c, q, plan, mr=t.mr)
    assert splits == plan["splits"]
    du.assert_case("decode instance " + du.instance_name(t), o, lse, du.oracle(c, q), parity_report)


def test_decode_instance_32_rows_forced(parity_report):
    """dec_mr = 32 with 15 query rows: the 32-row instance on a group the 16-row one would take."""
    t = du.Instance(128, torch.bfloat16, True, 16, "bal1")
    c, q, plan = du.instance_problem(t, "nan")
    o, lse, _, _ = _run(c, q, plan, dict(plan["knobs"], dec_mr=32), mr=32)
    du.assert_case("decode 15 rows on the 32-row tile", o, lse, du.oracle(c, q), parity_report)


def test_decode_bal_share_capped(parity_report):
    """The one shape past 1024 keys: 5 sequences x 32 splits = 160 slots, of which the long
    sequence's proportional share (142) is cut to dec_cap = 128, the scratch's split extent."""
    hk, group, sq, d = 4, 4, 1, 128
    ks, vs = du.make_kv(du.LENS_CAP, hk, d, 53)
    c = du.build_cache(ks, vs, du.PAGE, du.CAP_WIDTH, True, torch.bfloat16, "nan", seed=53)
    q = du.make_q(len(du.LENS_CAP), sq, hk * group, d, torch.bfloat16, 53)
    plan = du.plan_for(len(du.LENS_CAP), hk, du.CAP_WIDTH * du.PAGE, 32, BASE, sq, group)
    assert (plan["splits"], plan["slots"], plan["cap"]) == (32, 160, 128)
    o, lse, _, _ = _run(c, q, plan)
    du.assert_case("decode dec_cap", o, lse, du.oracle(c, q), parity_report)


# ---------------------------------------------------------------- (b) fill independence --
@pytest.mark.parametrize("fc", du.FILL_CASES, ids=du.fill_name)
def test_decode_fill_independence(parity_report, fc):
    """What lies in the cache outside the sequences (zeros, NaN, the largest finite value) must
    not reach a single bit of O or LSE."""
    got = {}
    for fill in du.FILLS:
        c, q, plan = du.fill_problem(fc, fill)
        got[fill] = _run(c, q, plan)[:2]
        assert not torch.isnan(got[fill][0]).any(), f"fill {fill}: NaN in O"
        assert not torch.isnan(got[fill][1]).any(), f"fill {fill}: NaN in LSE"
    for fill in ("nan", "big"):
        assert _same(got[fill][0], got["zero"][0]), f"O differs between fills {fill} and zero"
        assert _same(got[fill][1], got["zero"][1]), f"LSE differs between fills {fill} and zero"
    du.assert_case("decode fill " + du.fill_name(fc), *got["nan"], du.oracle(c, q), parity_report)


# ---------------------------------------------------------------- (c) mappings, bitwise --
_problem = du.paged_problem


def _with(plan, hk, b, **knobs):
    """The plan of the same problem under other knobs."""
    k = dict(plan["knobs"], **knobs)
    return du.plan_for(b, hk, du.WIDTH * du.PAGE, plan["num_splits"], k, plan["sq"], plan["group"])


@pytest.mark.parametrize("fp8,mr", [(True, 16), (False, 32)])
def test_decode_mappings_bitwise_hmaj(fp8, mr):
    """At one split count a wave's arithmetic does not depend on which workgroup holds it:
    dec_hmaj 0, 1 and 2 give the same bits."""
    group, sq = (5, 3) if mr == 16 else (7, 3)
    c, q, plan = _problem(du.LENS_EDGE, 8, group, sq, 128, torch.bfloat16, fp8, 61, 8,
                          dict(BASE, dec_bal=0))
    outs = []
    for hm in (0, 1, 2):
        p = _with(plan, 8, len(du.LENS_EDGE), dec_hmaj=hm)
        assert p["hm"] == hm and not p["bal"]
        outs.append(_run(c, q, p))
    for o, lse, kern, _ in outs[1:]:
        assert _same(o, outs[0][0]) and _same(lse, outs[0][1]), kern
    assert not torch.isnan(outs[0][0]).any()


@pytest.mark.parametrize("hm,ns", [(1, 4), (1, 16), (2, 8)])
def test_decode_mappings_bitwise_bal_equal_lengths(hm, ns):
    """Equal lengths: dec_bal gives every sequence num_splits slots, the uniform launch's ranges
    and result (the claim in dec_slot's comment)."""
    lens = [517] * 5
    c, q, plan = _problem(lens, 8, 4, 2, 64, torch.float16, True, 62, ns, dict(BASE, dec_hmaj=hm))
    assert plan["bal"] and plan["splits"] == ns
    a = _run(c, q, plan)
    b = _run(c, q, _with(plan, 8, len(lens), dec_bal=0))
    assert _same(a[0], b[0]) and _same(a[1], b[1])
    assert not torch.isnan(a[0]).any()


@pytest.mark.parametrize("fp8,hm", [(False, 1), (True, 2), (True, 0)])
def test_decode_mappings_bitwise_fold(fp8, hm):
    """dec_fold = 1 (the last split to arrive merges) equals the per-wave combine kernel
    (comb_row = 0) over a ragged cache with an empty sequence, twice in a row."""
    hk = {0: 2, 1: 4, 2: 8}[hm]
    c, q, plan = _problem(du.LENS_UNIFORM, hk, 5, 3, 128, torch.bfloat16, fp8, 63, 8,
                          dict(BASE, dec_hmaj=hm, dec_bal=0, comb_row=0))
    base = _run(c, q, plan)
    fold = _with(plan, hk, len(du.LENS_UNIFORM), dec_fold=1)
    for _ in range(2):
        f = _run(c, q, fold)
        assert _same(f[0], base[0]) and _same(f[1], base[1])
    assert not torch.isnan(base[0]).any() and not torch.isnan(base[1]).any()


def test_decode_mappings_bitwise_table():
    """The permuted block table equals the identity table over the same rows."""
    a = _problem(du.LENS_EDGE, 4, 4, 1, 128, torch.bfloat16, True, 64, 8)
    b = _problem(du.LENS_EDGE, 4, 4, 1, 128, torch.bfloat16, True, 64, 8, identity=True)
    assert not torch.equal(a[0].table, b[0].table)
    ra, rb = _run(*a), _run(*b)
    assert _same(ra[0], rb[0]) and _same(ra[1], rb[1])
    assert not torch.isnan(ra[0]).any()


# ---------------------------------------------------------------- (d) features -----------
@pytest.mark.parametrize("sq", [1, 4])
@pytest.mark.parametrize("window", list(du.WINDOWS))
def test_decode_features_paged_window(parity_report, window, sq):
    """Causal and sliding windows: t_first > 0, and with 4 query positions the per-row limits
    differ inside a tile; sequences shorter than seqlen_q have rows that see no key."""
    w = du.WINDOWS[window]
    c, q, plan = du.window_problem(sq)
    o, lse, _, _ = _run(c, q, plan, window=w)
    du.assert_case(f"decode window {w} sq{sq}", o, lse, du.oracle(c, q, window=w), parity_report)


@pytest.mark.parametrize("name", list(du.FEATURES))
def test_decode_features_paged_alibi_softcap(parity_report, name):
    """ALiBi with per-batch slopes and softcap 15, also over an fp8 cache (the C entry takes what
    the Python wrapper refuses); with a window (100, 7) and 4 query positions."""
    c, q, plan, kw, mult = du.feature_problem(name)
    o, lse, _, _ = _run(c, q, plan, **kw)
    du.assert_case("decode " + name, o, lse, du.oracle(c, q, **kw), parity_report, mult=mult)


@pytest.mark.parametrize("fp8", [False, True], ids=["kv16", "fp8"])
def test_decode_features_leftpad_causal(parity_report, fp8):
    """cache_leftpad values that are no multiples of 8 on a one-page cache, causal with 3 query
    positions: the diagonal counts from the leftpad."""
    c, q, plan = du.fill_problem((fp8, 16, True), "nan", seed=67)
    o, lse, _, _ = _run(c, q, plan, window=(-1, 0))
    du.assert_case(f"decode leftpad causal fp8={fp8}", o, lse, du.oracle(c, q, window=(-1, 0)),
                   parity_report)


# ---------------------------------------------------------------- (e) entries, auto split -
def test_decode_auto_split(parity_report):
    """num_splits = 0 under two dec_wg_per_cu values: the heuristic's split counts are launched
    (multiples of 4, no more with 1 workgroup per CU than with 16) and both are right."""
    c, q, plan = _problem(du.LENS_EDGE, 32, 1, 1, 128, torch.bfloat16, True, 68, 0,
                          dict(BASE, dec_hmaj=2))
    ora, seen = du.oracle(c, q), []
    for wg in (1, 16):
        o, lse, kern, splits = du.run_decode(c, q, 0, dict(plan["knobs"], dec_wg_per_cu=wg), 16,
                                             heads8=True)
        assert splits % 4 == 0 and 4 <= splits <= 16, kern
        seen.append(splits)
        du.assert_case(f"decode auto split wg_per_cu={wg} ({splits} splits)", o, lse, ora, parity_report)
    assert seen[0] <= seen[1], seen


def test_decode_reference_signature(parity_report):
    """The reference-signature fmha_page_kvcache_fwd (no LSE, 16-bit cache) on the poisoned cache."""
    c, q, plan = _problem(du.LENS_EDGE, 4, 7, 3, 64, torch.float16, False, 69, 8)
    o, _, _, _ = _run(c, q, plan, entry="ref")
    ora = du.oracle(c, q)
    assert not torch.isnan(o).any()
    ok, err, bound = orc.parity_ok(o, ora.ref, ora.pt, 3.0, 1e-5)
    parity_report(dict(case="decode reference signature", metric="o", err=err, bound=bound))
    assert ok, f"{err} > {bound}"


def test_decode_python_contiguous_cache(parity_report):
    """flash_attn_with_kvcache on a contiguous [b, max_sk, hk, d] cache whose rows past
    cache_seqlens are NaN: the extension passes it as one page per sequence, so those rows lie
    inside the page the decode kernel reads."""
    import xf_flash_attention_cutlass_amd as xfa
    from xf_flash_attention_cutlass_amd import capi
    lens, hk, d, max_sk = [528, 517, 33, 32, 1], 4, 128, 528
    ks, vs = du.make_kv(lens, hk, d, 70)
    c = du.build_cache(ks, vs, max_sk, 1, False, torch.bfloat16, "nan", seed=70, identity=True)
    b = len(lens)
    assert torch.equal(c.table[:, 0], torch.arange(b, dtype=torch.int32))
    kc, vc = c.kc[:b].contiguous().to(DEV), c.vc[:b].contiguous().to(DEV)
    assert torch.isnan(kc[1, 517:]).all() and torch.isnan(vc[4, 1:]).all()
    q = du.make_q(b, 1, hk * 4, d, torch.bfloat16, 70)
    o, lse = xfa.flash_attn_with_kvcache(q.to(DEV), kc, vc,
                                         cache_seqlens=torch.tensor(lens, dtype=torch.int32).to(DEV),
                                         num_splits=4, return_softmax_lse=True)
    torch.cuda.synchronize()
    kern = capi.lib().fmha_last_kernel().decode()
    assert kern.startswith("fmha_decode_kernel<16 rows>"), kern
    du.assert_case("decode python contiguous cache", o.cpu(), lse.cpu(), du.oracle(c, q), parity_report)
