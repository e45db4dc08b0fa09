"""Shared helpers of the softmax-rescale tests (not a conftest: imported explicitly; CPU only).

The forward kernels keep no exact running max in their key loops: P = exp2(S c - m) against a
reference max m that may lag the true max by `fwd_slack` log2 units, and a rare branch catches up
(DESIGN.md §4).  Unit-scale randn never enters that branch at the default slack (the largest jump
of a row's running max from one 64-key tile to the next is about 4 log2 units), so the inputs
here scale the keys.

* `_option`, `_randn`, `_growing`, `_overflow_margin`, `_rounding_bound`, `_check`: the helpers of
  tests/test_fwd4_redo_gpu.py, which imports them back.
* `PATTERNS` / `apply_pattern`: the key-scale patterns.  q, k, v are unit randn from seeded CPU
  generators; a pattern multiplies k row j by a factor (and, `mixed_rows`, some q rows).
* `tile_jumps`: per (row, 64-key tile) the jump of the masked running max, in log2 units.
* `tiled_softmax_model`: a small torch model of a tiled softmax with a lagging reference max, with
  deliberate faults (`FAULTS`).  Not an oracle: it exists so that tests/test_softmax_stress_util.py
  can show that the pass rules of tests/test_softmax_stress_gpu.py reject wrong kernels.
* `Case`, `CASES`, `inputs`, `refs`, `judge`: the case table both files are generated from, the
  references of one case and the pass rules (the project's own, unchanged).
"""
from __future__ import annotations

import math
from collections import namedtuple
from functools import lru_cache

import torch

from oracle import attention_ref as orc

LSE_ATOL = 1e-3
LSE_RTOL = 1e-5
LOG2E = 1.4426950408889634
BF, FP = torch.bfloat16, torch.float16
F8 = torch.float8_e4m3fn
TILE = 64
INF = float("inf")


def _lib():
    from xf_flash_attention_cutlass_amd import capi
    return capi.lib()


class _option:
    """fmha_set_option for the duration of a block (process-wide knob, restored after)."""

    def __init__(self, name, value):
        self.name, self.value = name.encode(), value

    def __enter__(self):
        L = _lib()
        self.old = L.fmha_get_option(self.name)
        assert L.fmha_set_option(self.name, self.value) == 0

    def __exit__(self, *exc):
        assert _lib().fmha_set_option(self.name, self.old) == 0


def _check(o, lse, q, k, v, causal, what, rtol_lse=0.0, o_atol=None):
    ref, _ = orc.attention_ref(q, k, v, causal=causal)
    pt, _ = orc.attention_ref(q, k, v, causal=causal, upcast=False, reorder_ops=True)
    assert torch.isfinite(o.float()).all(), f"{what}: non-finite output"
    ok, err, bound = orc.parity_ok(o, ref, pt, 2.0)
    assert ok, f"{what}: max|out-ref|={err:.3g} > bound {bound:.3g}"
    if o_atol is not None:
        assert err <= o_atol, f"{what}: max|out-ref|={err:.3g} > {o_atol}"
    lref = orc.attention_lse_ref(q, k, causal=causal)
    fin = torch.isfinite(lref)
    assert torch.equal(torch.isinf(lse), ~fin), f"{what}: empty-row pattern differs"
    tol = LSE_ATOL + rtol_lse * lref[fin].abs()
    lerr = (lse[fin] - lref[fin]).abs()
    assert (lerr <= tol).all(), f"{what}: max|lse-ref|={lerr.max().item():.3g}"


def _randn(shape, seed, dtype):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).to(dtype)


def _scale_keys(k, f):
    return (k.float() * f[None, :, None, None]).to(k.dtype)


def _growing(k, amp):
    """k rows scaled by 1 + amp * j / sk along the key axis (scores grow with the key)."""
    sk = k.shape[1]
    f = 1.0 + amp * torch.arange(sk, dtype=torch.float32) / sk
    return _scale_keys(k, f)


def _late_step(k, amp):
    """k rows scaled by 1 for j < sk - 9, by amp after: the jump sits in the last (ragged,
    right-edge) tile only, and under causal only some rows of a wave see it."""
    sk = k.shape[1]
    f = torch.ones(sk)
    f[max(sk - 9, 0):] = amp
    return _scale_keys(k, f)


def _descending(k, amp):
    """`_growing` reversed: the first tile holds the row max (no rescale ever; later P underflow)."""
    sk = k.shape[1]
    f = 1.0 + amp * torch.arange(sk - 1, -1, -1, dtype=torch.float32) / sk
    return _scale_keys(k, f)


def _mixed_rows(q, k):
    """growing(40) keys; q rows at positions pos % 3 != 0 scaled by 1/16: a wave then holds rows
    that must rescale beside rows that must not."""
    pos = torch.arange(q.shape[1])
    f = torch.where(pos % 3 != 0, torch.tensor(1.0 / 16), torch.tensor(1.0))
    return (q.float() * f[None, :, None, None]).to(q.dtype), _growing(k, 40.0)


PATTERNS = ("growing4", "growing40", "late40", "desc40", "mixed")


def apply_pattern(name, q, k):
    """(q, k) under a key-scale pattern: growing<amp>, late<amp>, desc<amp>, mixed, unit."""
    if name == "unit":
        return q, k
    if name == "mixed":
        return _mixed_rows(q, k)
    for pre, fn in (("growing", _growing), ("late", _late_step), ("desc", _descending)):
        if name.startswith(pre):
            return q, fn(k, float(name[len(pre):]))
    raise ValueError(name)


# ------------------------------------------------------------------ masks and tile jumps ------
MASKS = {"causal": (-1, 0), "full": (-1, -1), "w100_17": (100, 17), "w64_0": (64, 0)}


def mask_of(window, sq, sk):
    """[sq, sk] bool, True where a score is NOT allowed (None: no window at all)."""
    if window[0] < 0 and window[1] < 0:
        return None
    return orc.local_mask(sq, sk, window)


def _packed_scores(q, k, mask, softcap=0.0, bias=None):
    """fp32 scores in log2 units, GQA-packed as the kernels' items are: [b, hk, sq * G, sk], row
    = pos * G + g; masked scores are -inf."""
    b, sq, h, d = q.shape
    sk, hk = k.shape[1], k.shape[2]
    g = h // hk
    s = torch.einsum("bqhd,bkhd->bhqk", q.float(), orc.expand_kv(k.float(), h)) * d ** -0.5
    if softcap > 0:
        s = torch.tanh(s / softcap) * softcap
    if bias is not None:
        s = s + bias
    s = s * LOG2E
    if mask is not None:
        s = s.masked_fill(mask, -INF)
    # [b, h, sq, sk] -> [b, hk, g, sq, sk] -> [b, hk, sq, g, sk]
    return s.view(b, hk, g, sq, sk).permute(0, 1, 3, 2, 4).reshape(b, hk, sq * g, sk)


def _tile_max(s):
    """[.., rows, sk] -> [.., rows, tiles]: the masked max of each 64-key tile"""
    sk = s.shape[-1]
    nt = (sk + TILE - 1) // TILE
    pad = torch.full(s.shape[:-1] + (nt * TILE - sk,), -INF)
    return torch.cat([s, pad], -1).view(*s.shape[:-1], nt, TILE).amax(-1)


def _jumps(q, k, mask, softcap=0.0, bias=None):
    """[.., rows, tiles]: tile max minus the running max of the tiles before it; NaN where the row
    has seen no key yet (its first visible tile and the masked ones before it) or the tile is
    masked"""
    tm = _tile_max(_packed_scores(q, k, mask, softcap, bias))
    run = torch.cummax(tm, -1).values
    prev = torch.cat([torch.full_like(run[..., :1], -INF), run[..., :-1]], -1)
    j = tm - prev
    return torch.where(torch.isfinite(prev) & torch.isfinite(tm), j, torch.full_like(j, math.nan))


def tile_jumps(q, k, mask=None, slack=8.0, softcap=0.0, bias=None):
    """Per row and 64-key tile, the jump of the masked running max in log2 units, counted from
    each row's first visible tile: (the largest jump, the number of (row, tile) pairs above
    `slack`).  (0.0, 0) when no row sees a second tile.  softcap / bias (ALiBi, natural units,
    broadcastable to [b, h, sq, sk]): the score transforms, applied before the walk."""
    j = _jumps(q, k, mask, softcap, bias)
    j = j[~torch.isnan(j)]
    if j.numel() == 0:
        return 0.0, 0
    return max(j.max().item(), 0.0), int((j > slack).sum())


def jumps_between(q, k, mask, lo, hi):
    """number of (row, tile) jumps in (lo, hi]"""
    j = _jumps(q, k, mask)
    j = j[~torch.isnan(j)]
    return int(((j > lo) & (j <= hi)).sum())


def mixed_groups(q, k, mask, slack=8.0, rows=32):
    """number of `rows`-row groups (one wave's rows of the GQA-packed item) in which, at one and
    the same tile, some rows jump by more than `slack` and some visible rows do not"""
    j = _jumps(q, k, mask)                                  # [b, hk, R, nt]
    R = j.shape[2]
    pad = (-R) % rows
    j = torch.cat([j, torch.full(j.shape[:2] + (pad, j.shape[3]), math.nan)], 2)
    j = j.view(j.shape[0], j.shape[1], -1, rows, j.shape[3])
    up = (j > slack).any(3)
    stay = (j <= 0).any(3)
    return int((up & stay).sum())


def _overflow_margin(q, k, causal, window=(-1, -1)):
    """max over rows of (max later score - the max of the row's first visible tile) in log2
    units: > 128 means exp2 against that tile's max overflows fp32, i.e. the kernel cannot be
    right without the rescale.  (A view of the running-max walk `tile_jumps` counts.)"""
    sq, sk = q.shape[1], k.shape[1]
    tm = _tile_max(_packed_scores(q, k, mask_of((window[0], 0) if causal else window, sq, sk)))
    seen = torch.isfinite(tm)
    first = seen.float().argmax(-1, keepdim=True)
    m0 = tm.gather(-1, first)
    t = torch.arange(tm.shape[-1])
    later = torch.where(t > first, tm, torch.full_like(tm, -INF)).amax(-1, keepdim=True)
    d = later - m0
    d = d[torch.isfinite(d)]
    return d.max().item() if d.numel() else -INF


def _rounding_bound(q, k, v, causal, ref=None):
    """A priori bound on |O - O_ref| from the kernel's two roundings: P to the input dtype before
    PV (half an ulp, u = 2^-8 bf16 / 2^-11 fp16, relative per weight: <= u max|v|) and O to the
    output dtype (<= u |O|); 5 % slack for the fp32 sums."""
    u = 2.0 ** -8 if q.dtype == torch.bfloat16 else 2.0 ** -11
    if ref is None:
        ref, _ = orc.attention_ref(q, k, v, causal=causal)
    return 1.05 * u * (v.float().abs().max().item() + ref.float().abs().max().item())


# ------------------------------------------------------------------ the tiled-softmax model ---
FAULTS = ("no_rescale", "alpha_skips_l", "fresh_as_zero", "p_saturates")


def tiled_softmax_model(q, k, v, window=(-1, -1), slack=8.0, fault=None, p_limit=None,
                        p_dtype=None, rows=32, softcap=0.0, bias=None):
    """A tiled softmax with a lagging reference max: fp32 scores, 64-key tiles, P = exp2(S c - m)
    rounded to `p_dtype` (default q's dtype) before PV, the row sum over the unrounded P, and m
    moved to the true running max only when some row of a `rows`-row group exceeds it by more than
    `slack` log2 units (then every row of the group moves).  Returns (out [b, sq, h, d] in q's
    dtype, lse [b, h, sq] fp32; a row without a visible key: O = 0, LSE = +inf).

    Faults: `no_rescale` (m stays at the first visible tile's max), `alpha_skips_l` (O rescaled,
    l not), `fresh_as_zero` (a row whose first tile is masked exponentiates against 0 and never
    records the max it rescaled to), `p_saturates` (P clamped at `p_limit` before rounding)."""
    assert fault in (None,) + FAULTS
    b, sq, h, d = q.shape
    sk, hk = k.shape[1], k.shape[2]
    g = h // hk
    p_dtype = p_dtype or q.dtype
    s = _packed_scores(q, k, mask_of(window, sq, sk), softcap, bias)      # [b, hk, R, sk]
    R = s.shape[2]
    vv = v.float().permute(0, 2, 1, 3)                                      # [b, hk, sk, d]
    m = torch.full((b, hk, R), -INF)
    l = torch.zeros(b, hk, R)
    O = torch.zeros(b, hk, R, d)
    zero_ref = torch.zeros(b, hk, R, dtype=torch.bool)
    grp = (torch.arange(R) // rows)
    ngrp = int(grp.max()) + 1
    for t in range((sk + TILE - 1) // TILE):
        st = s[..., t * TILE:(t + 1) * TILE]
        mx = st.amax(-1)
        if t == 0 and fault == "fresh_as_zero":
            zero_ref = torch.isneginf(mx)
            m = torch.where(zero_ref, torch.zeros_like(m), m)
        want = (mx > m + slack) & torch.isfinite(mx)
        if fault == "no_rescale":
            want = want & torch.isneginf(m)
        move = (torch.zeros(b, hk, ngrp).index_add_(2, grp, want.float()) > 0)[..., grp]
        if fault == "no_rescale":
            move = move & torch.isneginf(m)
        m_new = torch.where(move, torch.maximum(m, mx), m)
        alpha = torch.where(torch.isfinite(m) & torch.isfinite(m_new), torch.exp2(m - m_new),
                            torch.ones_like(m))
        O = O * alpha[..., None]
        if fault != "alpha_skips_l":
            l = l * alpha
        mref = torch.where(torch.isfinite(m_new), m_new, torch.zeros_like(m_new))
        P = torch.exp2(st - mref[..., None])                                # exp2(-inf) = 0
        l = l + P.sum(-1)
        if fault == "p_saturates":
            P = P.clamp(max=p_limit)
        O = O + torch.matmul(P.to(p_dtype).float(), vv[:, :, t * TILE:(t + 1) * TILE])
        # the faulty fresh rows forget the max they moved to: the next tile is taken against 0
        m = torch.where(zero_ref, torch.zeros_like(m_new), m_new)
    dead = torch.isneginf(s.amax(-1))
    out = torch.where(dead[..., None], torch.zeros_like(O), O / l[..., None])
    lse = torch.where(dead, torch.full_like(l, INF), (m + torch.log2(l)) / LOG2E)
    out = out.view(b, hk, sq, g, d).permute(0, 2, 1, 3, 4).reshape(b, sq, h, d)
    lse = lse.view(b, hk, sq, g).permute(0, 1, 3, 2).reshape(b, h, sq)
    return out.to(q.dtype), lse


# ------------------------------------------------------------------ the fp16 edge of the slack --
EDGE_LO, EDGE_HI = 15.99975, 15.99995      # log2(65520) = 15.99965: fp16 rounds P >= 65520 to inf


def fp16_edge_inputs(d=64, row=(0, 0), key=200):
    """Unit randn fp16 (q, k, v) of the usual shape, full mask, with one key row rewritten so that
    one query row's score at it exceeds that row's tile-0 max by a lag inside [EDGE_LO, EDGE_HI]
    log2 units.  No other (row, tile) jumps by more than a few units, so at fwd_slack = 16 nothing
    moves the reference max and that row's P there is 2^lag >= 65520: inf once rounded to fp16.
    Any slack <= 15 rescales first.  The key is q's own direction, rounded to fp16, then single
    elements are moved by whole ulps until the exact (float64) score lands in the window."""
    q, k, v = (x.clone() for x in _base(1, SQ, SK, H, HK, d, FP))
    pos, head = row
    kh = head // (H // HK)
    c = d ** -0.5 * LOG2E
    qr = q[0, pos, head].double()
    m0 = (k[0, :TILE, kh].double() @ qr).max().item() * c
    target = 0.5 * (EDGE_LO + EDGE_HI) + m0
    kk = (qr * (target / c / (qr @ qr).item())).to(FP)
    for _ in range(4):
        for i in torch.argsort(qr.abs(), descending=True).tolist():
            res = target - (kk.double() @ qr).item() * c
            up = torch.nextafter(kk[i], torch.tensor(INF, dtype=FP) * torch.sign(qr[i]).to(FP))
            step = (up.double() - kk[i].double()).item() * qr[i].item() * c     # > 0
            n = int(max(-4, min(4, round(res / step)))) if step > 0 else 0
            for _ in range(abs(n)):
                kk[i] = torch.nextafter(kk[i], torch.tensor(INF if n > 0 else -INF, dtype=FP)
                                        * torch.sign(qr[i]).to(FP))
    k[0, key, kh] = kk
    lag = (kk.double() @ qr).item() * c - m0
    assert EDGE_LO <= lag <= EDGE_HI, lag
    return q, k, v


# ------------------------------------------------------------------ references and rules ------
Refs = namedtuple("Refs", "ref pt lse apriori")


def refs(q, k, v, window=(-1, -1), softcap=0.0, slopes=None, apriori=True) -> Refs:
    """The fp32 oracle, the low-precision estimate and the fp32 LSE of a dense problem, and the a
    priori bound (None with softcap).  slopes: fp32 [b, h] ALiBi (the LSE in the kernel's causal
    frame, oracle.alibi_bias_kernel)."""
    sq, sk = q.shape[1], k.shape[1]
    causal = window == (-1, 0)
    bias = lbias = None
    if slopes is not None:
        bias = orc.alibi_bias(slopes, sq, sk, causal=causal)
        lbias = orc.alibi_bias_kernel(slopes, sq, sk, causal=causal)
    kw = dict(window_size=window, softcap=softcap)
    ref, _ = orc.attention_ref(q, k, v, attn_bias=bias, **kw)
    pt, _ = orc.attention_ref(q, k, v, attn_bias=bias, upcast=False, reorder_ops=True, **kw)
    lse = orc.attention_lse_ref(q, k, attn_bias=lbias, **kw)
    ap = _rounding_bound(q, k, v, False, ref=ref) if apriori and softcap == 0 else None
    return Refs(ref, pt, lse, ap)


def judge(o, lse, r: Refs, mult=2.0, atol=0.0):
    """The pass rules (the project's own): O finite and max|O - ref| <= mult max|pt - ref| + atol;
    where given, max|O - ref| <= the a priori bound too; the LSE's +inf pattern equal to the
    reference's, its finite values within 1e-3 + 1e-5 |ref|.  Returns (ok, figures)."""
    f = dict(finite=bool(torch.isfinite(o.float()).all()), lse_nan=bool(torch.isnan(lse).any()))
    _, f["err"], f["bound"] = orc.parity_ok(o, r.ref, r.pt, mult, atol)
    f["apriori"] = r.apriori
    fin = torch.isfinite(r.lse)
    f["inf_ok"] = bool(torch.equal(torch.isinf(lse) & (lse > 0), ~fin))
    dl = (lse[fin] - r.lse[fin]).abs() - LSE_RTOL * r.lse[fin].abs()
    f["lse_err"] = dl.max().item() if dl.numel() else 0.0       # what the absolute 1e-3 must cover
    f["o_ok"] = f["finite"] and f["err"] <= f["bound"] and (r.apriori is None or f["err"] <= r.apriori)
    f["lse_ok"] = not f["lse_nan"] and f["inf_ok"] and f["lse_err"] <= LSE_ATOL
    return f["o_ok"] and f["lse_ok"], f


def assert_case(name, o, lse, r: Refs, report=None, mult=2.0, atol=0.0, extra=None):
    ok, f = judge(o, lse, r, mult, atol)
    ap = f"{r.apriori:.3e}" if r.apriori is not None else "-"
    print(f"{name}: o err {f['err']:.3e} bound {f['bound']:.3e} a-priori {ap}; "
          f"lse err {f['lse_err']:.3e} bound {LSE_ATOL:.0e}")
    if report is not None:
        row = dict(case=name, metric="o", err=f["err"], bound=f["bound"], ok=bool(f["o_ok"]))
        if r.apriori is not None:
            row["apriori"] = r.apriori
        row.update(extra or {})
        report(row)
        report(dict(case=name, metric="lse", err=f["lse_err"], bound=LSE_ATOL, ok=bool(f["lse_ok"])))
    assert ok, f"{name}: {f}"


# ------------------------------------------------------------------ the case table ------------
SQ, SK, H, HK = 150, 417, 4, 2
SLACKS = (0, 8, 16)
# group: the section of tests/test_softmax_stress_gpu.py; knobs: ((name, value), ...) on top of
# fwd_slack; feat: what the launch adds ("" plain; see that file)
Case = namedtuple("Case", "group d dtype mask pattern slack knobs feat splits b sk")


def _case(group, d, dtype, mask, pattern, slack, knobs=(), feat="", splits=1, b=1, sk=SK):
    return Case(group, d, dtype, mask, pattern, slack, tuple(knobs), feat, splits, b, sk)


def case_id(c: Case) -> str:
    kn = "".join(f"-{n}{v}" for n, v in c.knobs)
    ft = f"-{c.feat}" if c.feat else ""
    sp = f"-x{c.splits}" if c.splits != 1 else ""
    dt = {BF: "bf16", FP: "fp16"}[c.dtype]
    return f"{c.group}-d{c.d}-{dt}-{c.mask}-{c.pattern}-s{c.slack}{kn}{ft}{sp}"


def _table():
    T = []
    masks = list(MASKS)
    diag = [(masks[i % 4], p) for i, p in enumerate(PATTERNS)]
    # A: fmha_fwd_kernel, every D != 128 bucket and D = 128 under fwd_w4 = 0
    for d in (64, 256):
        for m in masks:
            for p in PATTERNS:
                for s in SLACKS:
                    T.append(_case("A", d, BF, m, p, s, b=2 if d == 64 else 1))
        for i, (m, p) in enumerate(diag):
            for s in (0, 16):
                T.append(_case("A", d, FP, masks[(i + 1) % 4], p, s))
    for d in (40, 96, 192, 128):
        w4 = (("fwd_w4", 0),) if d == 128 else ()
        for dt in (BF, FP):
            for i, (m, p) in enumerate(diag):
                T.append(_case("A", d, dt, m, p, SLACKS[(i + (dt == FP)) % 3], w4))
    for pipe in (0, 2):                                        # (1 is the default, above)
        for i, (m, p) in enumerate(diag):
            T.append(_case("A", 64, BF, m, p, 8, (("fwd_pipe", pipe),), b=2))
    # B: the same kernel with score features
    for d in (64, 128):
        w4 = (("fwd_w4", 0),) if d == 128 else ()
        for feat, pat in (("alibi", "growing40"), ("alibi", "growing4"), ("softcap", "growing40"),
                          ("alibi+softcap", "growing40")):
            for m in ("causal", "full"):
                T.append(_case("B", d, BF, m, pat, 8, w4, feat))
        T.append(_case("B", d, FP, "causal", "growing4", 16, w4, "alibi"))
        T.append(_case("B", d, FP, "full", "growing40", 0, w4, "softcap"))
    # C: split-KV and the combines
    for d in (64, 128, 256):
        for n in (3, 7):
            for m, p in (("full", "growing40"), ("causal", "late40")):
                for cr in (0, 1):
                    for sink in ("", "sink"):
                        T.append(_case("C", d, BF, m, p, 8, (("comb_row", cr),), sink, n))
    # D: the D = 128 ping-pong kernels
    for p in ("growing4", "growing40"):
        for s in (8, 0):
            for m in ("w100_17", "w64_0", "full"):
                T.append(_case("D", 128, BF, m, p, s))
            T.append(_case("D", 128, FP, "w100_17", p, s))
            T.append(_case("D", 128, BF, "causal", p, s, feat="alibi"))
            T.append(_case("D", 128, BF, "causal", p, s, feat="softcap"))
            T.append(_case("D", 128, BF, "full", p, s, feat="alibi"))
    # E: sinks, one case per mechanism (sink=combine: the C cases)
    T.append(_case("E", 64, BF, "causal", "growing40", 8, feat="sink"))
    T.append(_case("E", 128, BF, "causal", "growing40", 8, feat="sink"))
    T.append(_case("E", 64, BF, "full", "growing40", 8, feat="sink", splits=3))
    return T


CASES = _table()
SEEDS = (11, 12, 13)


@lru_cache(maxsize=None)
def _base(b, sq, sk, h, hk, d, dtype, seeds=SEEDS):
    return tuple(_randn(s, seed, dtype) for seed, s in
                 zip(seeds, ((b, sq, h, d), (b, sk, hk, d), (b, sk, hk, d))))


def inputs(c: Case, sq=SQ):
    """(q, k, v) of a case, on the CPU.  softcap cases scale q by 4, so that the capped scores
    still jump by more than 8."""
    q, k, v = _base(c.b, sq, c.sk, H, HK, c.d, c.dtype)
    q, k = apply_pattern(c.pattern, q, k)
    if "softcap" in c.feat:
        q = (q.float() * 4).to(q.dtype)
    return q, k, v


SOFTCAP = 50.0


def slopes_of(c: Case):
    """fp32 [b, h] ALiBi slopes in 0.05 .. 0.5, or None"""
    if "alibi" not in c.feat:
        return None
    return torch.linspace(0.05, 0.5, c.b * H).view(c.b, H)


def softcap_of(c: Case):
    return SOFTCAP if "softcap" in c.feat else 0.0


@lru_cache(maxsize=None)
def case_refs(key):
    """Refs of the inputs of a case, shared by the cases that differ in knobs only"""
    c = key
    q, k, v = inputs(c)
    return refs(q, k, v, MASKS[c.mask], softcap_of(c), slopes_of(c))


def input_key(c: Case) -> Case:
    """the case with everything that does not change its inputs or references removed"""
    feat = "+".join(f for f in c.feat.split("+") if f in ("alibi", "softcap"))
    return c._replace(group="", slack=0, knobs=(), feat=feat, splits=1)


# ------------------------------------------------------------------ fp8 forward cases (F) -----
# kind: dense | varlen; knobs on top of fwd_slack.  The kernel a case must run: a left window
# or fp8_w4 = 0 -> fmha_fwd_fp8_kernel<8 waves>, else fmha_fwd8w_kernel.
Fp8Case = namedtuple("Fp8Case", "kind pattern mask out slack knobs")
FP8_LENS = (63, 65, 200, 417)
FP8_SEEDS = (31, 32, 33)       # 11 / 12 / 13 miss the 0.8 condition at sk 417 (growing4: 0.87)


def fp8_case_id(c: Fp8Case) -> str:
    kn = "".join(f"-{n}{v}" for n, v in c.knobs)
    return f"F-{c.kind}-{c.mask}-{c.pattern}-{'fp16' if c.out == FP else 'bf16'}-s{c.slack}{kn}"


def _fp8_table():
    T = []
    w0 = (("fp8_w4", 0),)
    for s in SLACKS:
        T.append(Fp8Case("dense", "growing4", "full", BF, s, ()))
        T.append(Fp8Case("dense", "growing8", "full", FP, s, ()))
        T.append(Fp8Case("dense", "growing8", "causal", BF, s, ()))
        T.append(Fp8Case("dense", "growing8", "w100_17", BF, s, ()))
        T.append(Fp8Case("dense", "growing8", "w64_0", FP, s, ()))
        T.append(Fp8Case("dense", "growing4", "full", FP, s, w0))
        T.append(Fp8Case("dense", "growing8", "causal", BF, s, w0))
        T.append(Fp8Case("varlen", "growing8", "causal", BF, s, ()))
        T.append(Fp8Case("varlen", "growing8", "full", FP, s, w0))
    return T


FP8_CASES = _fp8_table()


@lru_cache(maxsize=None)
def fp8_inputs(kind, pattern, seeds=FP8_SEEDS):
    """Quantised inputs of an fp8 case: dense ((q8, qs), (k8, ks), (v8, vs)) of [1, s, h, 128], or
    packed [total, h, 128] with each sequence's keys scaled separately (lens FP8_LENS, q and k)."""
    if kind == "dense":
        q, k, v = (_randn(s, seed, torch.float32) for seed, s in
                   zip(seeds, ((1, SQ, H, 128), (1, SK, HK, 128), (1, SK, HK, 128))))
        q, k = apply_pattern(pattern, q, k)
    else:
        tot = sum(FP8_LENS)
        q, k, v = (_randn(s, seed, torch.float32) for seed, s in
                   zip(seeds, ((tot, H, 128), (tot, HK, 128), (tot, HK, 128))))
        ks, a = [], 0
        for n in FP8_LENS:
            ks.append(apply_pattern(pattern, None, k[a:a + n][None])[1][0])
            a += n
        k = torch.cat(ks)
    return tuple(orc.quantize_fp8(x) for x in (q, k, v))


def fp8_refs(q8, k8, v8, qs, ks, vs, window, out_dtype):
    """(ref, pt, lse) of one dense fp8 problem: the fp32 oracle over the dequantised inputs, the
    estimate with P rounded to e4m3 (its output rounded to out_dtype) and the fp32 LSE"""
    sk = k8.shape[1]
    qd, kd, vd = q8.float() * qs, k8.float() * ks, v8.float() * vs
    w = (window[0], sk) if window[0] >= 0 and window[1] < 0 else window
    ref, _ = orc.attention_ref(qd, kd, vd, window_size=w)
    pt = orc.attention_fp8_pt(q8, k8, v8, qs, ks, vs, window_size=w).to(out_dtype)
    lse = orc.attention_lse_ref(qd, kd, window_size=w)
    return Refs(ref, pt, lse, None)


def fp8_problems(c: Fp8Case):
    """the dense problems of a case (one; varlen: one per sequence) as (q8, k8, v8) slices with a
    leading batch of 1, and the per-tensor scales"""
    (q8, qs), (k8, ks), (v8, vs) = fp8_inputs(c.kind, c.pattern)
    if c.kind == "dense":
        return [(q8, k8, v8)], (qs, ks, vs)
    out, a = [], 0
    for n in FP8_LENS:
        out.append((q8[a:a + n][None], k8[a:a + n][None], v8[a:a + n][None]))
        a += n
    return out, (qs, ks, vs)


# ------------------------------------------------------------------ caches (B, D, G) ----------
def grown_cache(lens, d, dtype, fp8, pattern, page, width, leftpad=None, seed=80):
    """decode_util.build_cache over unit randn K/V with each sequence's keys under `pattern`; an
    fp8 cache takes the k scale that just fits the scaled keys (no power of two)"""
    from tests import decode_util as du
    ks, vs = du.make_kv(lens, HK, d, seed, leftpad)
    ks = [apply_pattern(pattern, None, x[None])[1][0] for x in ks]
    k_scale = max(x.abs().max().item() for x in ks) / 440.0 if fp8 else du.K_SCALE
    return du.build_cache(ks, vs, page, width, fp8, dtype, "nan", leftpad=leftpad, seed=seed,
                          k_scale=k_scale)


DECODE_LENS = (600, 417)


def decode_problem(d, fp8, pattern):
    """(cache, q) of a decode case: sq 1, two sequences, page 16, 40 pages a row (640 keys: 20
    tiles of 32, so the launch takes up to 8 splits)"""
    from tests import decode_util as du
    c = grown_cache(list(DECODE_LENS), d, BF, fp8, pattern, du.PAGE, 40, seed=90 + d)
    return c, du.make_q(2, 1, H, d, BF, 91)
