"""Shared helpers of the backward stress tests (not a conftest: imported explicitly; CPU only).

Every other backward test draws q, k, v and dO as unit randn.  There a row's softmax is flat, O is
an average of hundreds of values and D = rowsum(dO * O) is small beside dP, so a kernel that reads
the wrong D (a neighbour's, none, the LSE half of the slot it shares with the LSE) moves dS little;
a wrongly unmasked score costs P = 1 / sk; and the LSE comes from a forward that never entered
its catch-up branch.  The inputs here put the key-scale patterns of tests/softmax_stress_util.py
on q and k: rows are peaked (O = v_j, |D| = |dP|), masked keys score far above the row's LSE, and
|S c| reaches the hundreds.

* `Case` / `CASES`, `Packed` / `PACKED`: the case tables that tests/test_bwd_stress_util.py (CPU)
  and tests/test_bwd_stress_gpu.py are both generated from.
* `inputs`, `oracle_kw`, `emu_kw`, `case_refs`, `packed_inputs`, `packed_refs`: inputs and cached
  float64 references (shared by the cases that differ in det / slack / knobs only).
* `figures`, `check_stress`: the stress rule.

The stress rule is `bwd_util.check_grads`' two rules with the same multipliers (global: 3, or 5
with ALiBi + softcap; block: 3) and the same `+ 1e-5` and `eps / 2 rms(ref64)` terms.  The one
change: the error of the low-precision estimate is the larger of |pt - ref| and |emu - ref|, where
emu is `bwd_util.emulate_bwd`, on the GPU fed the O and LSE the forward kernel stored (the global
rule takes the max over the tensor, the block rule per (batch, 32-row block, head)).  The second
estimate is needed because a correct kernel takes D from the stored, rounded O, and on peaked rows
that rounding alone exceeds the plain block rule
(tests/test_bwd_util.py::test_stored_o_rounding_on_peaked_rows).

Every report row carries
  widen     = bound_stress / bound_plain of the block (or tensor) the row reports, and
  emu_plain = the emulation's own worst err / bound under the plain rule for that gradient.
`widen_needed = max(1, emu_plain)` is the factor by which the plain bound has to grow before a
correct kernel's arithmetic passes it at all, and it is the figure the caps below are on.  The
per-block `widen` cannot carry them: two low-precision estimates of like size trade places from
block to block, so it is above 1 in about half of all blocks whether or not the plain rule would
have done.  It is bounded through the other figure: emu <= emu_plain * bound_plain in every block,
so widen <= 3 * emu_plain + 1 (10 under the cap of 3).

Two caps, over the whole table (`CASES` and `PACKED` together), asserted by
tests/test_bwd_stress_util.py:
* at most 10 % of the (case, gradient) pairs have `widen_needed` above 1;
* none has it above `NEED_CAP` = 3.
There the emulation runs on its own O and LSE, and the packed cases also on the float64 O and LSE
rounded once (`packed_exact_fwd`); a pair counts with the larger of its two figures.
tests/test_bwd_stress_gpu.py asserts the second cap on the forward kernel's O and LSE, case by
case: a forward that stored a wrong O would raise |emu - ref|, and with it the bound, so the
figure is held down there too.  The seeds (`SEED`, `PACKED_SEED`) are chosen so that the caps hold.
"""
from __future__ import annotations

import itertools
from collections import namedtuple
from functools import lru_cache

import torch

from oracle import attention_ref as orc
from tests import bwd_util as bu
from tests import sink_ref as sr
from tests.softmax_stress_util import PATTERNS, apply_pattern

BF, FP = torch.bfloat16, torch.float16
B, H, HK = 2, 4, 2
SEED = 21
MASKS = {"full": (False, (-1, -1)), "causal": (True, (-1, -1)), "w100_30": (False, (100, 30)),
         "w100_0": (False, (100, 0))}
SOFTCAP = 20.0

# group: inst | cross | slack | doscale | sink.  slack: fwd_slack of the forward (None: the
# session's).  gmul: dO is multiplied by it.  w4: None (a dense launch under the session's fwd_w4;
# at these shapes it splits its keys, so fmha_fwd_kernel and the combine write O and the LSE), 4
# (the D = 128 ping-pong forward) or 0 (fwd_w4 = 0: fmha_fwd_kernel), both as one packed launch of
# b equal sequences, which is single-pass.  sink: a per-head sink at the median LSE.
Case = namedtuple("Case", "group d dtype mask feat det pattern slack gmul w4 sink")
Packed = namedtuple("Packed", "d dtype mask det pattern")
PACKED_LQ = (1, 33, 300, 77, 130)
PACKED_LK = (147, 20, 300, 600, 64)
PACKED_SEED = 4
NEED_CAP = 3.0             # on widen_needed of every (case, gradient) pair
OVER_SHARE = 0.10          # of the pairs may have widen_needed above 1


def shape(d):
    """(sq, sk) of tests/test_bwd_instances_gpu.py: three key blocks with a ragged tail"""
    return (77, 300) if bu.bucket(d) == 256 else (113, 600)


def _mask_name(t: bu.Instance):
    return "causal" if t.causal else ("w%d_%d" % t.window if t.mask else "full")


def _table():
    T, seen = [], set()

    def add(group, d, dtype, mask, feat, det, pattern, slack=None, gmul=1.0, w4=None, sink=False):
        c = Case(group, d, dtype, mask, feat, det, pattern, slack, gmul, w4, sink)
        if c[1:] not in seen:                        # the cross repeats some instance cases
            seen.add(c[1:])
            T.append(c)

    # every instance csrc/fmha_bwd.hip dispatches, one pattern each: i % 5 walks the patterns
    # against det (i % 2), feat, MASK, dtype and the bucket (tests/test_bwd_stress_util.py)
    for i, t in enumerate(bu.instance_table()):
        add("inst", t.d, t.dtype, _mask_name(t), t.feat, t.det, PATTERNS[i % len(PATTERNS)])
    for d in (64, 128):
        for p, m, det in itertools.product(PATTERNS, ("full", "causal", "w100_30"), (False, True)):
            add("cross", d, BF, m, False, det, p)
    # the LSE of a forward at slack 0 / 16; D = 128 on the ping-pong forward and on fmha_fwd_kernel
    for slack, dtype, (m, p) in itertools.product((0, 16), (BF, FP), (("causal", "growing40"),
                                                                      ("w100_30", "late40"))):
        add("slack", 64, dtype, m, False, dtype == FP, p, slack)
        for w4 in (4, 0):
            add("slack", 128, dtype, m, False, dtype == BF, p, slack, w4=w4)
    for det in (False, True):
        add("doscale", 64, FP, "causal", False, det, "growing4", gmul=256.0)     # loss scaling
        add("doscale", 128, FP, "causal", False, det, "growing4", gmul=256.0)
        add("doscale", 64, BF, "full", False, det, "growing4", gmul=2.0 ** 20)
        for d in (64, 128):
            add("sink", d, BF, "causal", False, det, "growing40", sink=True)
    return T


CASES = _table()
PACKED = [Packed(d, dt, m, det, p) for (d, dt), m, det, p in itertools.product(
    ((64, BF), (128, FP)), ("causal", "w100_0"), (False, True), ("growing40", "late40"))]


def _dt(dtype):
    return {BF: "bf16", FP: "fp16"}[dtype]


def case_id(c) -> str:
    if isinstance(c, Packed):
        return f"packed-d{c.d}-{_dt(c.dtype)}-{c.mask}-{c.pattern}-{'det' if c.det else 'atomic'}"
    s = f"{c.group}-d{c.d}-{_dt(c.dtype)}-{c.mask}-{c.pattern}-{'feat' if c.feat else 'plain'}-" \
        f"{'det' if c.det else 'atomic'}"
    if c.slack is not None:
        s += f"-s{c.slack}"
    if c.w4 is not None:
        s += f"-w4_{c.w4}"
    if c.gmul != 1.0:
        s += f"-dOx{c.gmul:g}"
    return s + ("-sink" if c.sink else "")


# ------------------------------------------------------------------ inputs and references -----
@lru_cache(maxsize=None)
def _base(d, dtype, feat, seed=SEED):
    """unit randn (q, k, v, dO, slopes) as tests/test_bwd_instances_gpu.py draws them"""
    sq, sk = shape(d)
    gen = torch.Generator().manual_seed(seed)
    q = torch.randn(B, sq, H, d, generator=gen)
    if feat:
        q = q * 4
    q = q.to(dtype)
    k, v = (torch.randn(B, sk, HK, d, generator=gen).to(dtype) for _ in range(2))
    g = torch.randn(B, sq, H, d, generator=gen).to(dtype)
    slopes = torch.rand(B, H, generator=gen) * 0.3 if feat else None
    return q, k, v, g, slopes


def inputs(c: Case):
    """(q, k, v, dO) of a case on the CPU: the pattern on q and k, dO times gmul"""
    q, k, v, g, _ = _base(c.d, c.dtype, c.feat)
    q, k = apply_pattern(c.pattern, q, k)
    if c.gmul != 1.0:
        g = (g.float() * c.gmul).to(c.dtype)
    return q, k, v, g


def slopes_of(c: Case):
    return _base(c.d, c.dtype, c.feat)[4]


def oracle_kw(c: Case):
    causal, window = MASKS[c.mask]
    kw = dict(causal=causal, window_size=window)
    if c.feat:
        kw.update(softcap=SOFTCAP, attn_bias=orc.alibi_bias(slopes_of(c), *shape(c.d), causal=False))
    return kw


def emu_kw(c: Case):
    """`emulate_bwd`'s arguments.  ALiBi in the frame of the LSE the library returns
    (`orc.alibi_bias_kernel`: causal + slope * key), so that a forward's LSE can take the place
    of the emulation's own; dS does not depend on the frame."""
    causal, window = MASKS[c.mask]
    kw = dict(causal=causal, window=window)
    if c.feat:
        kw.update(softcap=SOFTCAP,
                  attn_bias=orc.alibi_bias_kernel(slopes_of(c), *shape(c.d), causal=causal))
    return kw


def mult_of(c):
    return 5.0 if getattr(c, "feat", False) else 3.0


def sink_at_median(lse_ref):
    """per head, the median finite reference LSE [b, h, sq] -> [h]: the sink then carries weight"""
    per = lse_ref.permute(1, 0, 2).reshape(lse_ref.shape[1], -1)
    return torch.stack([x[torch.isfinite(x)].median() for x in per]).float()


def sink_of(c: Case):
    if not c.sink:
        return None
    q, k, _, _ = inputs(c)
    causal, window = MASKS[c.mask]
    return sink_at_median(orc.attention_lse_ref(q, k, causal=causal, window_size=window))


def input_key(c: Case) -> Case:
    """the case without what changes neither its inputs nor its references"""
    return c._replace(group="", det=False, slack=None, w4=None)


SinkRefs = namedtuple("SinkRefs", "sink ds64 dspt term")


@lru_cache(maxsize=None)
def case_refs(key: Case):
    """(bwd_util.Refs, SinkRefs or None) of `input_key(case)`"""
    q, k, v, g = inputs(key)
    if not key.sink:
        return bu.ref_grads(q, k, v, g, **oracle_kw(key)), None
    causal, window = MASKS[key.mask]
    sink = sink_of(key)
    fn = lambda a, b_, c_, s, reorder_ops: sr.sink_attention(a, b_, c_, s, causal=causal, window=window,
                                                             reorder_ops=reorder_ops)
    refs, ds64, dspt, o64, l64 = sr.grad_refs(fn, q, k, v, g, sink, key.dtype)
    term = sum(sr.dsink_term(sink, l64[i], g[i], o64[i], key.dtype) for i in range(q.shape[0]))
    return refs, SinkRefs(sink, ds64, dspt, term)


def cu(lens):
    return torch.tensor([0] + list(itertools.accumulate(lens)), dtype=torch.int32)


@lru_cache(maxsize=None)
def packed_inputs(d, dtype, pattern, seed=PACKED_SEED):
    """packed (q, k, v, dO), each sequence's keys under the pattern separately"""
    gen = torch.Generator().manual_seed(seed)
    tq, tk = sum(PACKED_LQ), sum(PACKED_LK)
    q = torch.randn(tq, H, d, generator=gen).to(dtype)
    k, v = (torch.randn(tk, HK, d, generator=gen).to(dtype) for _ in range(2))
    g = torch.randn(tq, H, d, generator=gen).to(dtype)
    qs, ks = [], []
    for a, b_ in zip(bu.seq_slices(cu(PACKED_LQ)), bu.seq_slices(cu(PACKED_LK))):
        qq, kk = apply_pattern(pattern, q[a][None], k[b_][None])
        qs.append(qq[0])
        ks.append(kk[0])
    return torch.cat(qs), torch.cat(ks), v, g


@lru_cache(maxsize=None)
def packed_refs(d, dtype, mask, pattern):
    causal, window = MASKS[mask]
    q, k, v, g = packed_inputs(d, dtype, pattern)
    return bu.ref_grads_varlen(q, k, v, g, cu(PACKED_LQ), cu(PACKED_LK), causal=causal,
                               window_size=window)


def packed_exact_fwd(p: Packed):
    """the float64 (O [total_q, h, d], LSE [h, total_q]) of a packed case, rounded to the dtype and
    to fp32: what a forward with no error but the store's rounding leaves behind"""
    causal, window = MASKS[p.mask]
    q, k, v, _ = packed_inputs(p.d, p.dtype, p.pattern)
    o, lse = sr.sink_attention_varlen(q.double(), k.double(), v.double(), None, PACKED_LQ, PACKED_LK,
                                      causal=causal, window=window)
    return o.to(p.dtype), lse.float()


def packed_emulate(p: Packed, o=None, lse=None, defect=None):
    """`emulate_bwd` per sequence of a packed case: a list of (dq, dk, dv) over [1, s_i, h, d];
    o packed [total_q, h, d] and lse [h, total_q] as the library returns them"""
    causal, window = MASKS[p.mask]
    q, k, v, g = packed_inputs(p.d, p.dtype, p.pattern)
    res = []
    for a, b_ in zip(bu.seq_slices(cu(PACKED_LQ)), bu.seq_slices(cu(PACKED_LK))):
        kw = {}
        if o is not None:
            kw = dict(o=o[a][None], lse=lse[:, a][None])
        res.append(bu.emulate_bwd(q[a][None], k[b_][None], v[b_][None], g[a][None], causal, window,
                                  defect=defect, **kw))
    return res


# ------------------------------------------------------------------ the stress rule -----------
def figures(got, refs: bu.Refs, emu, dtype, mult=3.0):
    """The figures of the stress rule for (dq, dk, dv) [b, s, h, d]: a list of rows
    {metric, err, bound, bound_plain, widen, emu_plain, finite[, block]}, two per gradient."""
    rows = []
    for nm, x, e, r64, r, p in zip(bu.NAMES, got, emu, refs.ref64, refs.ref, refs.pt):
        if x.numel() == 0:
            continue
        x, e = x.cpu(), e.cpu()
        assert x.shape == r.shape, f"{nm}: shape {tuple(x.shape)} != {tuple(r.shape)}"
        assert torch.isfinite(e.float()).all(), f"{nm}: the emulation is not finite"
        finite = bool(torch.isfinite(x.float()).all())
        rf = r.float()
        err = (x.float() - rf).abs().max().item() if finite else float("inf")
        e_pt, e_emu = ((y.float() - rf).abs().max().item() for y in (p, e))
        plain = mult * e_pt + 1e-5
        bound = mult * max(e_pt, e_emu) + 1e-5
        rows.append(dict(metric=f"{nm} global", err=err, bound=bound, bound_plain=plain,
                         widen=bound / plain, emu_plain=e_emu / plain, finite=finite))
        floor = 0.5 * bu.EPS[dtype] * bu._block_ms(r64).sqrt() + 1e-5
        b_pt, b_emu = (bu._block_ms(y.double() - r64).sqrt() for y in (p, e))
        bplain = 3.0 * b_pt + floor
        bbound = 3.0 * torch.maximum(b_pt, b_emu) + floor
        if finite:
            berr = bu._block_ms(x.double() - r64).sqrt()
            i = int((berr / bbound).argmax())
            berr = berr.flatten()[i].item()
        else:
            i, berr = 0, float("inf")
        where = [int(y) for y in torch.unravel_index(torch.tensor(i), bbound.shape)]
        bb, bp = bbound.flatten()[i].item(), bplain.flatten()[i].item()
        rows.append(dict(metric=f"{nm} block", err=berr, bound=bb, bound_plain=bp, widen=bb / bp,
                         emu_plain=(b_emu / bplain).max().item(), finite=finite, block=where))
    return rows


def widen_needed(rows):
    """{gradient: the largest emu_plain} of `figures` / `check_stress` rows"""
    need = {}
    for r in rows:
        g = r["metric"].split()[0]
        need[g] = max(need.get(g, 0.0), r["emu_plain"])
    return need


def worst_ratio(rows, factors=None):
    """the largest err / (bound * factor) of `figures` rows"""
    f = factors or {}
    return max(r["err"] / (r["bound"] * (f.get(r["metric"].split()[0], 1.0)
                                         if r["metric"].endswith("block") else 1.0)) for r in rows)


def check_stress(name, got, refs: bu.Refs, emu, dtype, report=None, mult=3.0, block_factor=None,
                 extra=None):
    """Asserts the stress rule on (dq, dk, dv); `report` gets one row per rule and gradient, with
    `extra` merged in.  `block_factor` as `bwd_util.check_grads`'.  Returns the rows."""
    rows = figures(got, refs, emu, dtype, mult)
    failures = []
    for r in rows:
        r["case"] = name
        factor = 1.0
        if r["metric"].endswith("block"):
            factor = r["bound_factor"] = (block_factor or {}).get(r["metric"].split()[0], 1.0)
        r.update(extra or {})
        if report:
            report(r)
        if not r["finite"]:
            failures.append(f"{name} {r['metric']}: non-finite values")
        elif not r["err"] <= r["bound"] * factor:
            failures.append(f"{name} {r['metric']}: err {r['err']:.3g} > {r['bound']:.3g} "
                            f"(plain {r['bound_plain']:.3g}) at {r.get('block', '')}")
    assert not failures, "; ".join(failures)
    return rows
