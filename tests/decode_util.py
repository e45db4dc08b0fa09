"""Shared helpers of the decode tests (not a conftest: imported explicitly).

* `build_cache`: per-sequence K/V -> a paged cache (16-bit or e4m3fn) behind a random, non-identity
  block table, with everything the kernel must not depend on set to a chosen fill.
* `run_decode`: fmha_page_kvcache_fwd_ex through the C ABI into NaN-filled outputs under a set of
  knobs (restored afterwards); asserts the decode kernel it was meant to run did run.
* `oracle`: per-sequence `orc.attention_ref` / `orc.attention_lse_ref` over the exact cache values.
* `judge` / `assert_case`: the pass rule of the decode tests.
* `tile_range`, `split_range`, `bal_shares`, `host_plan`, `split_tiles`: a Python port of the
  kernel's split arithmetic, used only to choose and check the test shapes.
* `emulate_decode`: a CPU model of a correct split decode with plantable defects, for
  tests/test_decode_util.py.
* `instance_table`, `FILL_CASES`, `WINDOWS`, `FEATURES` and their `*_problem` builders: the cases
  of tests/test_decode_instances_gpu.py, shared with the CPU model tests.
"""
from __future__ import annotations

import itertools
from collections import namedtuple

import torch

from oracle import attention_ref as orc

DEV = "cuda"
TILE = 32                                         # kDecKeys
PAGE = 16
F8 = torch.float8_e4m3fn
FILLS = ("zero", "nan", "big")
DEFECTS = ("v_tail", "k_tail", "drop_last_tile", "second_page", "no_v_scale", "combine_ns")
LSE_ATOL = 1e-3
K_SCALE, V_SCALE = 0.0123, 0.0371                 # not powers of two

Cache = namedtuple("Cache", "kc vc table lens leftpad page width fp8 dtype k_scale v_scale "
                            "kx vx poison")
Oracle = namedtuple("Oracle", "ref ref64 pt lse")


# ---------------------------------------------------------------- the cache --------------
def _fill_pool(shape, fp8, dtype, fill):
    if fp8:
        byte = {"zero": 0x00, "nan": 0x7F, "big": 0x7E}[fill]     # 0x7E = 448, the largest e4m3fn
        return torch.full(shape, byte, dtype=torch.uint8).view(F8)
    val = {"zero": 0.0, "nan": float("nan"), "big": torch.finfo(dtype).max}[fill]
    return torch.full(shape, val, dtype=dtype)


def build_cache(ks, vs, page, width, fp8, dtype, fill, leftpad=None, seed=0, identity=False,
                k_scale=K_SCALE, v_scale=V_SCALE) -> Cache:
    """ks / vs: per-sequence float tensors [n_b, hk, d] (n_b may be 0).  Sequence b occupies the
    logical rows [leftpad[b], leftpad[b] + n_b) of its pages; `lens` (the cache_seqlens) counts the
    leftpad.  The pool holds the pages in use, one poison page every table entry past a sequence's
    last page points at, and two pages no entry names; rows past a sequence's end, rows in front of
    its leftpad and those pages hold `fill`.  `kx` / `vx` are the exact values the kernel is
    defined over, float32(stored) * scale."""
    assert fill in FILLS and page % 16 == 0
    b = len(ks)
    hk, d = ks[0].shape[1:]
    lp = list(leftpad) if leftpad is not None else [0] * b
    lens = [lp[i] + ks[i].shape[0] for i in range(b)]
    used = [(n + page - 1) // page for n in lens]
    assert max(used) <= width
    npages = sum(used) + 3
    gen = torch.Generator().manual_seed(1000 + seed)
    perm = torch.arange(npages) if identity else torch.randperm(npages, generator=gen)
    if not identity and npages > 1 and torch.equal(perm, torch.arange(npages)):
        perm = perm.roll(1)
    poison = int(perm[sum(used)])
    table = torch.full((b, width), poison, dtype=torch.int32)
    kc = _fill_pool((npages, page, hk, d), fp8, dtype, fill)
    vc = _fill_pool((npages, page, hk, d), fp8, dtype, fill)
    kx, vx, nxt = [], [], 0
    for i in range(b):
        table[i, :used[i]] = perm[nxt:nxt + used[i]].int()
        nxt += used[i]
        if fp8:
            k_st = (ks[i].float() / k_scale).clamp(-448, 448).to(F8)
            v_st = (vs[i].float() / v_scale).clamp(-448, 448).to(F8)
            kx.append(k_st.float() * k_scale)
            vx.append(v_st.float() * v_scale)
        else:
            k_st, v_st = ks[i].to(dtype), vs[i].to(dtype)
            kx.append(k_st.float())
            vx.append(v_st.float())
        raw = (lambda x: x.view(torch.uint8)) if fp8 else (lambda x: x)
        r = lp[i] + torch.arange(ks[i].shape[0])
        pg = table[i, r // page].long()
        raw(kc)[pg, r % page] = raw(k_st)
        raw(vc)[pg, r % page] = raw(v_st)
    assert int(table.min()) >= 0 and int(table.max()) < npages      # never outside the pool
    return Cache(kc, vc, table, lens, lp if leftpad is not None else None, page, width, fp8, dtype,
                 k_scale if fp8 else 1.0, v_scale if fp8 else 1.0, kx, vx, poison)


def make_kv(lens, hk, d, seed, leftpad=None):
    """Per-sequence random K/V of lens[b] - leftpad[b] rows."""
    gen = torch.Generator().manual_seed(seed)
    lp = leftpad or [0] * len(lens)
    ks = [torch.randn(n - p, hk, d, generator=gen) for n, p in zip(lens, lp)]
    vs = [torch.randn(n - p, hk, d, generator=gen) for n, p in zip(lens, lp)]
    return ks, vs


def make_q(b, sq, h, d, dtype, seed, mul=1.0):
    gen = torch.Generator().manual_seed(7000 + seed)
    return (torch.randn(b, sq, h, d, generator=gen) * mul).to(dtype)


# ---------------------------------------------------------------- the launch -------------
def run_decode(c: Cache, q, num_splits, knobs, expect_mr, window=(-1, -1), softcap=0.0,
               slopes=None, heads8=False, entry="ex", want_grid=None):
    """One call on a device copy of the cache.  `knobs` maps option names to values; all are put
    back.  Returns (o, lse, kernel, splits) with o / lse on the CPU (lse None for the
    reference-signature entry, which has none)."""
    from xf_flash_attention_cutlass_amd import capi
    L = capi.lib()
    b, sq, h, d = q.shape
    hk = c.kc.shape[2]
    qd, kc, vc = q.to(DEV), c.kc.to(DEV), c.vc.to(DEV)
    tab = c.table.to(DEV)
    lens = torch.tensor(c.lens, dtype=torch.int32).to(DEV)
    lp = torch.tensor(c.leftpad, dtype=torch.int32).to(DEV) if c.leftpad is not None else None
    sl = slopes.to(DEV).contiguous() if slopes is not None else None
    o = torch.full_like(qd, float("nan"))
    lse = torch.full((b, h, sq), float("nan"), dtype=torch.float32, device=DEV)
    old = {n: L.fmha_get_option(n.encode()) for n in knobs}
    try:
        for n, v in knobs.items():
            assert L.fmha_set_option(n.encode(), v) == 0, n
        if entry == "ex":
            L.fmha_page_kvcache_fwd_ex(
                qd.data_ptr(), kc.data_ptr(), vc.data_ptr(), o.data_ptr(), lse.data_ptr(),
                tab.data_ptr(), tab.stride(0), lens.data_ptr(), sq, c.width * c.page, b, h, hk, d,
                c.page, d ** -0.5, window[0], window[1], softcap, capi.ptr(sl),
                sl.stride(0) if sl is not None else 0, num_splits, 1 if c.fp8 else 0,
                c.k_scale, c.v_scale, capi.ptr(lp), q.dtype == torch.float16, capi.stream_handle())
        else:
            assert not c.fp8 and lp is None and sl is None and softcap == 0.0
            L.fmha_page_kvcache_fwd(
                qd.data_ptr(), kc.data_ptr(), vc.data_ptr(), None, None, o.data_ptr(),
                tab.data_ptr(), lens.data_ptr(), c.width * c.page, sq, c.width * c.page, b, h, hk,
                d, c.page, capi.stream_handle(), d ** -0.5, window[0], window[1], num_splits,
                None, None, None, False, False, q.dtype == torch.float16)
        capi.check()
        torch.cuda.synchronize()
        kern = L.fmha_last_kernel().decode()
        splits = L.fmha_last_num_splits()
    finally:
        for n, v in old.items():
            L.fmha_set_option(n.encode(), v)
    want = "fmha_decode_kernel<%d rows%s>" % (expect_mr, ", 8 heads" if heads8 else "")
    assert kern.startswith(want), f"ran {kern!r}, wanted {want!r}"
    if want_grid is not None:
        assert "grid=%dx%dx1 " % want_grid in kern + " ", f"ran {kern!r}, wanted grid {want_grid}"
    return o.cpu(), (lse.cpu() if entry == "ex" else None), kern, splits


# ---------------------------------------------------------------- the oracle -------------
def _oracle_window(window, sk):
    wl, wr = window
    return (wl, sk) if (wl >= 0 and wr < 0) else (wl, wr)


def oracle(c: Cache, q, window=(-1, -1), softcap=0.0, slopes=None) -> Oracle:
    """Per sequence over its len - leftpad keys.  ref: the project's fp32-upcast oracle (in q's
    dtype); ref64: the same in float64; pt: the low-precision twin over the cache rounded to q's
    dtype; lse: fp32 [b, h, sq].  A sequence without keys gives O = 0, LSE = +inf."""
    b, sq, h, d = q.shape
    ref = torch.zeros(b, sq, h, d, dtype=q.dtype)
    pt = torch.zeros(b, sq, h, d, dtype=q.dtype)
    ref64 = torch.zeros(b, sq, h, d, dtype=torch.float64)
    lse = torch.full((b, h, sq), float("inf"), dtype=torch.float32)
    for i in range(b):
        n = c.kx[i].shape[0]
        if n == 0:
            continue
        qi, k, v = q[i:i + 1], c.kx[i][None], c.vx[i][None]
        kw = dict(window_size=_oracle_window(window, n), softcap=softcap)
        bias = orc.alibi_bias(slopes[i:i + 1], sq, n, causal=False) if slopes is not None else None
        ref[i] = orc.attention_ref(qi, k, v, attn_bias=bias, **kw)[0][0]
        ref64[i] = orc.attention_ref(qi.double(), k.double(), v.double(), upcast=False,
                                     attn_bias=bias.double() if bias is not None else None, **kw)[0][0]
        pt[i] = orc.attention_ref(qi, k.to(q.dtype), v.to(q.dtype), attn_bias=bias, upcast=False,
                                  reorder_ops=True, **kw)[0][0]
        lse[i] = orc.attention_lse_ref(qi, k, attn_bias=bias, **kw)[0]
    return Oracle(ref, ref64, pt, lse)


def judge(o, lse, ora: Oracle, mult=3.0, atol=1e-5):
    """The pass rule: no NaN left, max|o - ref| <= mult * max|pt - ref| + atol (the project's
    kvcache rule), the LSE's inf pattern equal to the oracle's and its finite values within
    LSE_ATOL.  Returns (ok, figures)."""
    f = dict(nan_o=int(torch.isnan(o).sum()), nan_lse=int(torch.isnan(lse).sum()))
    _, f["err"], f["bound"] = orc.parity_ok(o, ora.ref, ora.pt, mult, atol)
    f["err64"] = (o.double() - ora.ref64).abs().max().item()
    fin = torch.isfinite(ora.lse)
    f["inf_ok"] = bool(torch.equal(torch.isinf(lse) & (lse > 0), ~fin))
    dl = (lse[fin] - ora.lse[fin]).abs()
    f["lse_err"] = dl.max().item() if dl.numel() else 0.0
    ok = (f["nan_o"] == 0 and f["nan_lse"] == 0 and f["err"] <= f["bound"] and f["inf_ok"]
          and f["lse_err"] <= LSE_ATOL)
    return ok, f


def assert_case(name, o, lse, ora, report=None, mult=3.0, atol=1e-5):
    ok, f = judge(o, lse, ora, mult, atol)
    print(f"{name}: o err {f['err']:.3e} (vs float64 {f['err64']:.3e}) bound {f['bound']:.3e}; "
          f"lse err {f['lse_err']:.3e} bound {LSE_ATOL:.0e}")
    if report is not None:
        report(dict(case=name, metric="o", err=f["err"], bound=f["bound"]))
        report(dict(case=name, metric="lse", err=f["lse_err"], bound=LSE_ATOL))
    assert ok, f"{name}: {f}"


# ---------------------------------------------------------------- split arithmetic -------
def ring_depth(fp8, mr):
    return (3 if mr == 16 else 2) if fp8 else 1


def norm_window(window, max_sk):
    """set_windows of the host: an open side of a half-open window becomes max_seqlen_k."""
    wl, wr = window
    if wl < 0 and wr >= 0:
        wl = max_sk
    if wl >= 0 and wr < 0:
        wr = max_sk
    return wl, wr


def tile_range(sk, sq, group, wl, wr):
    """dec_tile_range: the key tiles [t_first, t_end) some query row of the group can see."""
    rows = sq * group
    diag = sk - sq
    last = (rows - 1) // group if rows > 0 else 0
    k_lo = max(0, diag - wl) if wl >= 0 else 0
    k_hi = min(sk, last + diag + wr + 1) if wr >= 0 else sk
    t_first = k_lo // TILE
    t_end = (k_hi + TILE - 1) // TILE if k_hi > k_lo else t_first
    return t_first, t_end


def split_range(t_first, t_end, nsplit, split):
    per = (t_end - t_first + nsplit - 1) // nsplit
    t_lo = min(t_end, t_first + split * per)
    return t_lo, min(t_end, t_lo + per)


def bal_shares(tiles, slots, cap):
    """dec_slot: the split slots n_b of each sequence, in proportion to its key tiles."""
    total, extra, incl, out = sum(tiles), slots - len(tiles), 0, []
    for tb in tiles:
        incl += tb
        n = 1 + (extra * incl // total - extra * (incl - tb) // total if total > 0 else 0)
        out.append(min(n, cap))
    return out


def host_plan(b, hk, max_sk, num_splits, hmaj=1, bal=1, fold=0):
    """The decode part of the host's run_fwd for an explicit num_splits > 0:
    (splits, dec_hmaj, dec_bal, dec_slots, dec_cap)."""
    tiles = (max_sk + TILE - 1) // TILE
    zs = max(1, min((num_splits + 3) // 4, max(1, tiles // 8)))
    splits = 4 * min(zs, 32)
    hm = 2 if (hmaj == 2 and hk % 8 == 0) else 1 if (hmaj >= 1 and hk % 4 == 0) else 0
    on = bool(bal and not fold and hm >= 1 and 2 <= b <= 64)
    slots = b * splits if on else 0
    return splits, hm, on, slots, min(slots, 128) if on else 0


def split_tiles(eff_lens, sq, group, window, max_sk, splits, bal, slots=0, cap=0):
    """Per sequence: (n_b, [tiles owned by each of its splits])."""
    wl, wr = norm_window(window, max_sk)
    rng = [tile_range(n, sq, group, wl, wr) for n in eff_lens]
    shares = bal_shares([e - f for f, e in rng], slots, cap) if bal else [splits] * len(rng)
    out = []
    for (f, e), nb in zip(rng, shares):
        own = [split_range(f, e, nb, s) for s in range(nb)]
        out.append((nb, [hi - lo for lo, hi in own]))
    return out


# ---------------------------------------------------------------- the CPU model ----------
def _tile_rows(c: Cache, pool, b, t, defect):
    """The 32 rows of tile t of sequence b as the kernel addresses them, float32 of the stored
    values (no scale)."""
    lp = c.leftpad[b] if c.leftpad is not None else 0
    r = lp + t * TILE + torch.arange(TILE)
    pi = (torch.full_like(r, lp + t * TILE) if defect == "second_page" else r) // c.page
    pg = torch.where(pi < c.width, c.table[b, pi.clamp(max=c.width - 1)].long(),
                     torch.full_like(r, c.poison))
    return pool[pg, r % c.page]


def emulate_decode(c: Cache, q, splits, bal=False, slots=0, cap=0, window=(-1, -1), softcap=0.0,
                   slopes=None, defect=None):
    """A correct split decode on the CPU: per-split partials over 32-key tiles with fp32
    accumulation, P rounded to q's dtype, the fp8 scales applied in fp32 to S and O, then the
    combine over each sequence's split count.  `defect` plants one of DEFECTS.  Returns (o, lse)."""
    assert defect is None or defect in DEFECTS
    b, sq, h, d = q.shape
    hk = c.kc.shape[2]
    g = h // hk
    max_sk = c.width * c.page
    wl, wr = norm_window(window, max_sk)
    scale = d ** -0.5
    o = torch.zeros(b, sq, h, d, dtype=q.dtype)
    lse = torch.full((b, h, sq), float("inf"), dtype=torch.float32)
    lps = c.leftpad if c.leftpad is not None else [0] * b
    eff = [n - p for n, p in zip(c.lens, lps)]
    rng = [tile_range(n, sq, g, wl, wr) for n in eff]
    shares = bal_shares([e - f for f, e in rng], slots, cap) if bal else [splits] * b
    pos = torch.arange(sq).view(1, sq, 1)
    kpool, vpool = c.kc.float(), c.vc.float()
    for i in range(b):
        sk, (t_first, t_end), nb = eff[i], rng[i], shares[i]
        qf = q[i].float().permute(1, 0, 2)                       # [h, sq, d]
        diag = sk - sq
        lim_r = torch.clamp(pos + diag + wr + 1, max=sk) if wr >= 0 else torch.full_like(pos, sk)
        if defect == "k_tail":                                   # the end of the sequence not applied
            lim_r = pos + diag + wr + 1 if wr >= 0 else torch.full_like(pos, t_end * TILE)
        lim_l = torch.clamp(pos + diag - wl, min=0) if wl >= 0 else torch.zeros_like(pos)
        parts_o, parts_l = [], []
        for s in range(nb):
            t_lo, t_hi = split_range(t_first, t_end, nb, s)
            if defect == "drop_last_tile" and s == 0 and t_hi > t_lo:
                t_hi -= 1
            m_run = torch.full((h, sq), float("-inf"))
            l_run = torch.zeros(h, sq)
            acc = torch.zeros(h, sq, d)
            for t in range(t_lo, t_hi):
                kt = _tile_rows(c, kpool, i, t, defect).repeat_interleave(g, dim=1)   # [32, h, d]
                vt = _tile_rows(c, vpool, i, t, defect).repeat_interleave(g, dim=1)
                key = (t * TILE + torch.arange(TILE)).view(1, 1, TILE)
                st = torch.einsum("hqd,khd->hqk", qf, kt) * c.k_scale * scale
                if softcap > 0:
                    st = torch.tanh(st / softcap) * softcap
                if slopes is not None:
                    st = st - slopes[i].view(h, 1, 1) * (pos + diag - key).abs().float()
                st = torch.where((key >= lim_r) | (key < lim_l), torch.tensor(float("-inf")), st)
                if defect != "v_tail":
                    vt = torch.where((key.view(TILE, 1, 1) >= sk), torch.tensor(0.0), vt)
                m_new = torch.maximum(m_run, st.amax(-1))
                mref = torch.where(torch.isneginf(m_new), torch.zeros_like(m_new), m_new)
                alpha = torch.exp(m_run - mref)
                p = torch.exp(st - mref[..., None])
                l_run = l_run * alpha + p.sum(-1)
                acc = acc * alpha[..., None] + torch.einsum("hqk,khd->hqd", p.to(q.dtype).float(), vt)
                m_run = m_new
            empty = (l_run == 0) | torch.isnan(l_run)
            vs = 1.0 if defect == "no_v_scale" else c.v_scale
            inv = torch.where(empty, torch.zeros_like(l_run), vs / l_run)
            parts_o.append(acc * inv[..., None])
            parts_l.append(torch.where(empty, torch.tensor(float("-inf")), m_run + torch.log(l_run)))
        if defect == "combine_ns" and bal:
            # the uniform count: partials past it are lost; slots this sequence never wrote are
            # read as they lie in the scratch (modelled as a second copy of its first partial)
            parts_o = (parts_o + [parts_o[0]] * splits)[:splits]
            parts_l = (parts_l + [parts_l[0]] * splits)[:splits]
        po, pl = torch.stack(parts_o), torch.stack(parts_l)      # [ns, h, sq(, d)]
        mx = pl.amax(0)
        sm = torch.where(torch.isneginf(mx), torch.zeros_like(mx),
                         torch.exp(pl - torch.where(torch.isneginf(mx), torch.zeros_like(mx), mx)).sum(0))
        rempty = torch.isneginf(mx) | (sm == 0)
        ls = torch.where(rempty, torch.tensor(float("inf")), torch.log(sm) + mx)
        w = torch.where(rempty[None], torch.zeros_like(pl), torch.exp(pl - ls[None]))
        o[i] = (w[..., None] * po).sum(0).permute(1, 0, 2).to(q.dtype)
        lse[i] = ls
    return o, lse


# ---------------------------------------------------------------- the cases --------------
MAPPINGS = ("hmaj0", "hmaj1", "hmaj2", "bal1", "bal2")
Instance = namedtuple("Instance", "d dtype fp8 mr mapping")
# Uniform launches, 4 splits: the splits of the five sequences own {5,5,5,2}, {4,4,4,3}, {3,3,3,1},
# {1,1,0,0} and {0,0,0,0} tiles - every count r and RING + r of every ring depth.
LENS_UNIFORM = [517, 470, 300, 33, 0]
# dec_bal, 20 slots: shares {6, 7, 4, 2, 1}, whose splits own {5,5,5,5,5,4}, {5,5,5,5,5,5,2},
# {4,4,4,3}, {1,1} and {0} tiles (tests/test_decode_util.py checks both lists with the port).
LENS_BAL = [897, 1016, 455, 33, 0]
NUM_SPLITS = 4
WIDTH = 1024 // PAGE
# The one shape past 1024 keys: a share limited by dec_cap needs more than 128 slots (5 sequences
# x 32 splits, which takes a 2048-key table); the long sequence's 142 slots are cut to 128.
LENS_CAP = [2048, 33, 33, 33, 0]
CAP_WIDTH = 2048 // PAGE


def instance_table():
    return [Instance(*t) for t in itertools.product(
        (64, 128), (torch.bfloat16, torch.float16), (False, True), (16, 32), MAPPINGS)]


def instance_name(t):
    return "d%d-%s-%s-mr%d-%s" % (t.d, str(t.dtype).split(".")[-1], "fp8" if t.fp8 else "kv16",
                                  t.mr, t.mapping)


def mapping_shape(mapping, mr):
    """(hk, group, sq, lens, knobs) of a mapping: 15 query rows (one dead MFMA column) for the
    16-row tile, 21 for the 32-row one; 8 / 4 / 2 kv heads for dec_hmaj 2 / 1 / 0."""
    hm = {"hmaj0": 0, "hmaj1": 1, "hmaj2": 2, "bal1": 1, "bal2": 2}[mapping]
    bal = mapping.startswith("bal")
    hk = {0: 2, 1: 4, 2: 8}[hm]
    group, sq = (5, 3) if mr == 16 else (7, 3)
    knobs = dict(dec_hmaj=hm, dec_bal=int(bal), dec_mr=16, dec_fold=0)
    return hk, group, sq, (LENS_BAL if bal else LENS_UNIFORM), knobs


def launch_grid(b, hk, splits, hm):
    """The decode launch's grid (x, y)."""
    return (b * hk, splits // 4) if hm == 0 else (b * hk // (4 * hm), splits)


def plan_for(b, hk, max_sk, num_splits, knobs, sq, group):
    splits, hm, bal, slots, cap = host_plan(b, hk, max_sk, num_splits, knobs["dec_hmaj"],
                                            knobs["dec_bal"], knobs.get("dec_fold", 0))
    return dict(num_splits=num_splits, splits=splits, hm=hm, bal=bal, slots=slots, cap=cap,
                knobs=knobs, heads8=hm == 2, sq=sq, group=group,
                grid=launch_grid(b, hk, splits, hm))


def instance_problem(t, fill="nan", seed=31):
    """(cache, q, plan) of an instance; plan: what the host makes of the knobs (host_plan), the
    launch grid and the knobs themselves."""
    hk, group, sq, lens, knobs = mapping_shape(t.mapping, t.mr)
    ks, vs = make_kv(lens, hk, t.d, seed)
    c = build_cache(ks, vs, PAGE, WIDTH, t.fp8, t.dtype, fill, seed=seed)
    q = make_q(len(lens), sq, hk * group, t.d, t.dtype, seed)
    return c, q, plan_for(len(lens), hk, WIDTH * PAGE, NUM_SPLITS, knobs, sq, group)


# Fill independence: one case per (cache type, MFMA rows, paged | one page with leftpad).  The
# paged lengths hold a full table, a ragged tail, one key past a tile, exactly one tile and one
# key; the one-page cache (272 rows, a multiple of 16) has leftpads that are no multiples of 8
# and sequences of 269, 187, 32, 40 and 0 keys behind them.
FILL_CASES = list(itertools.product((False, True), (16, 32), (False, True)))
LENS_EDGE = [1024, 517, 33, 32, 1]
ONEPAGE = 272
ONEPAGE_LENS = [272, 200, 77, 45, 13]
ONEPAGE_LEFTPAD = [3, 13, 45, 5, 13]


def fill_name(fc):
    return "%s-mr%d-%s" % ("fp8" if fc[0] else "kv16", fc[1], "onepage_leftpad" if fc[2] else "paged")


def fill_problem(fc, fill, seed=41):
    fp8, mr, onepage = fc
    hk, (group, sq) = 4, ((5, 3) if mr == 16 else (7, 3))
    d = 64 if fp8 == (mr == 16) else 128
    dtype = torch.float16 if onepage else torch.bfloat16
    if onepage:
        lens, lp, page, width, ns = ONEPAGE_LENS, ONEPAGE_LEFTPAD, ONEPAGE, 1, 4
    else:
        lens, lp, page, width, ns = LENS_EDGE, None, PAGE, WIDTH, 8
    ks, vs = make_kv(lens, hk, d, seed, lp)
    c = build_cache(ks, vs, page, width, fp8, dtype, fill, leftpad=lp, seed=seed)
    q = make_q(len(lens), sq, hk * group, d, dtype, seed)
    knobs = dict(dec_hmaj=1, dec_bal=1, dec_mr=16, dec_fold=0)
    return c, q, plan_for(len(lens), hk, width * page, ns, knobs, sq, group)


# Feature cases (windows, ALiBi, softcap) and the bitwise cases: one paged problem builder.  The
# feature lengths hold a full table, a ragged tail, one key past a tile, a sequence shorter than
# seqlen_q = 4 (rows without a visible key) and an empty one.
BASE_KNOBS = dict(dec_hmaj=1, dec_bal=1, dec_mr=16, dec_fold=0)
LENS_FEAT = [1024, 517, 33, 1, 0]
WINDOWS = {"causal": (-1, 0), "w64_0": (64, 0), "w100_7": (100, 7), "w-1_5": (-1, 5)}
# name -> (fp8 cache, ALiBi, softcap); all with the window (100, 7) and 4 query positions
FEATURES = {"alibi": (False, True, 0.0), "softcap": (False, False, 15.0),
            "fp8_alibi_softcap": (True, True, 15.0), "fp8_alibi": (True, True, 0.0)}


def paged_problem(lens, hk, group, sq, d, dtype, fp8, seed, num_splits, knobs=None, identity=False,
                  q_mul=1.0, fill="nan"):
    knobs = knobs or BASE_KNOBS
    ks, vs = make_kv(lens, hk, d, seed)
    c = build_cache(ks, vs, PAGE, WIDTH, fp8, dtype, fill, seed=seed, identity=identity)
    q = make_q(len(lens), sq, hk * group, d, dtype, seed, q_mul)
    return c, q, plan_for(len(lens), hk, WIDTH * PAGE, num_splits, knobs, sq, group)


def window_problem(sq, fill="nan"):
    return paged_problem(LENS_FEAT, 4, 4, sq, 128, torch.bfloat16, False, 65, 8, fill=fill)


def feature_problem(name, fill="nan"):
    """(cache, q, plan, kwargs for run_decode / oracle / emulate_decode, rule multiplier)."""
    fp8, alibi, softcap = FEATURES[name]
    c, q, plan = paged_problem(LENS_FEAT, 4, 4, 4, 64 if fp8 else 128, torch.float16, fp8, 66, 8,
                               q_mul=4.0 if softcap else 1.0, fill=fill)
    slopes = torch.rand(len(LENS_FEAT), 16, generator=torch.Generator().manual_seed(66)) * 0.3
    kw = dict(window=(100, 7), softcap=softcap, slopes=slopes if alibi else None)
    return c, q, plan, kw, (5.0 if softcap else 3.0)
