"""Shared helpers of the forward ownership tests (not a conftest: imported explicitly; CPU only
except `launch`).

A forward call owns the elements of q / k / v it is defined over and the elements of o / LSE it
must write.  Everything else a framework hands it - the rows behind a sequence in a larger
allocation, the rows past `seqused_k` / `cache_seqlens`, the rows in front of `cache_leftpad`, the
columns between head_size and the row pitch, pages no sequence owns, the gaps of a strided `o` -
holds arbitrary bits.  The tests here put a chosen fill there and require that nothing depends on
it and nothing of it is written.

* `Arena`, `strided_arena`, `packed_arena`, `lse_arena`: one flat allocation per tensor with the
  problem as a strided view inside it and a boolean "owned" mask; every other element holds the
  fill (`FILLS`: zero, NaN, dtype max; fp8 bytes 0x00 / 0x7F / 0x7E, decode_util._fill_pool).
  Margins: FRONT rows in front of the first row of every batch, BACK rows (one key tile) behind the
  last, one spare head and a row pitch of the bucket width + 8 for the strided entries.  The packed
  and cache entries take contiguous tensors, so their arenas have the row margins only.  A paged
  cache is decode_util.build_cache's (table entries a sequence does not own name an in-range page
  that holds the fill).
* `Case`, `CASES`, `SPLIT_CASES`, `ISOLATION`: the case tables of tests/test_fwd_own_gpu.py.
* `build`: the `Prob` of a case under one fill; `oracle`: its references (float32-upcast oracle,
  low-precision estimate, LSE) over the owned data only, with the multiplier / atol of the entry.
* `launch`: one call through the C ABI on device copies of the arenas; returns every buffer as it
  is after the call.
* `judge_case` / `check_case`: the five conditions (see `judge_case`).
* `model_launch`: a small tiled float32 forward over the arenas with plantable defects
  (`DEFECTS`), for tests/test_fwd_own_util.py.  Not an oracle.
"""
from __future__ import annotations

import itertools
from collections import namedtuple
from contextlib import ExitStack
from functools import lru_cache
from types import SimpleNamespace

import torch

from oracle import attention_ref as orc
from tests import decode_util as du
from tests import sink_ref as sr
from tests import softmax_stress_util as su
from tests.softmax_stress_util import BF, FP, F8, _option

DEV = "cuda"
FILLS = du.FILLS
FRONT, BACK, LSE_GUARD = 32, 64, 64
TILE_K, TILE_M = 64, 32
INF = float("inf")
NAN = float("nan")
LSE_ATOL, LSE_RTOL = su.LSE_ATOL, su.LSE_RTOL

Arena = namedtuple("Arena", "buf base shape strides owned")
Out = namedtuple("Out", "q k v o lse kern splits")
Oracle = namedtuple("Oracle", "ref pt lse mult atol")


def bucket(d):
    return 64 if d <= 64 else (128 if d <= 128 else 256)


def _bits(t):
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def _fill(n, dtype, fill):
    return du._fill_pool((n,), dtype == F8, dtype, fill)


def view(a: Arena, buf=None):
    """the problem's tensor inside the arena (or inside a copy of its buffer)"""
    return torch.as_strided(a.buf if buf is None else buf, a.shape, a.strides, a.base)


def _arena(buf, base, shape, strides, x, own_rows=None):
    """own_rows: [rows] bool over dimension 1; the rows it leaves out keep the fill"""
    a = Arena(buf, base, tuple(shape), tuple(strides), torch.zeros(buf.numel(), dtype=torch.bool))
    one = x.element_size() == 1                         # fp8: copied as bytes
    tv = torch.as_strided(buf.view(torch.uint8) if one else buf, a.shape, a.strides, a.base)
    xr = x.view(torch.uint8) if one else x
    ov = view(a, a.owned)
    if own_rows is None:
        ov.fill_(True)
        tv.copy_(xr)
    else:
        ov[:, own_rows] = True
        tv[:, own_rows] = xr[:, own_rows]
    return a


def strided_arena(x, fill):
    """x [b, s, heads, d] -> an arena [b, FRONT + s + BACK, heads + 1, bucket(d) + 8]"""
    b, s, hh, d = x.shape
    pitch, heads, rows = bucket(d) + 8, hh + 1, FRONT + s + BACK
    buf = _fill(b * rows * heads * pitch, x.dtype, fill)
    return _arena(buf, FRONT * heads * pitch, x.shape, (rows * heads * pitch, heads * pitch, pitch, 1), x)


def packed_arena(x, fill, own_rows=None):
    """x [rows, heads, d] (contiguous for the entry) -> an arena of FRONT + rows + BACK rows, as
    the 4-D view [1, rows, heads, d]; rows with own_rows False keep the fill"""
    rows, hh, d = x.shape
    buf = _fill((FRONT + rows + BACK) * hh * d, x.dtype, fill)
    return _arena(buf, FRONT * hh * d, (1, rows, hh, d), (0, hh * d, d, 1), x[None], own_rows)


def batched_arena(x, fill):
    """x [b, s, heads, d] contiguous (the cache entries' q and o) with the row margins"""
    b, s, hh, d = x.shape
    buf = _fill((FRONT + b * s + BACK) * hh * d, x.dtype, fill)
    return _arena(buf, FRONT * hh * d, x.shape, (s * hh * d, hh * d, d, 1), x)


def lse_arena(shape, fill):
    """fp32 [b, h, rows] contiguous, NaN inside, LSE_GUARD guard floats of the fill either side"""
    n = shape[0] * shape[1] * shape[2]
    buf = _fill(n + 2 * LSE_GUARD, torch.float32, fill)
    return _arena(buf, LSE_GUARD, shape, (shape[1] * shape[2], shape[2], 1),
                  torch.full(shape, NAN, dtype=torch.float32))


# ------------------------------------------------------------------ the case tables -----------
SHAPES = [(1, 1), (33, 65), (129, 63), (257, 130), (70, 200)]
WINDOWS = {"full": (-1, -1), "causal": (-1, 0), "w100_17": (100, 17), "w64_0": (64, 0),
           "w-1_17": (-1, 17)}
MASKS3 = ("causal", "w100_17", "w64_0")
B, H = 2, 4
# the packed sequences (the backward file's lengths; keys [0, USED) of a slot of LK rows) and one
# sequence without queries, whose slot is poison throughout
LQ = [1, 33, 300, 77, 130, 0]
LK = [147, 20, 300, 600, 64, 50]
USED = [147, 0, 257, 65, 64, 50]
SOFTCAP = 30.0
PAGE = 16

Case = namedtuple("Case", "group entry d dtype hk shape mask feat sink knobs need splits kernel "
                          "body inst extra")


def _case(group, entry, d, dtype, hk, shape, mask, feat="", sink=False, knobs=(), need=(), splits=1,
          kernel="fmha_fwd_kernel<", body=None, inst=None, extra=()):
    return Case(group, entry, d, dtype, hk, shape, mask, feat, sink, tuple(knobs), tuple(need),
                splits, kernel, body, inst, tuple(extra))


def case_id(c: Case) -> str:
    dt = {BF: "bf16", FP: "fp16"}[c.dtype]
    sh = "x".join(str(s) for s in c.shape) if c.shape else "packed"
    kn = "".join(f"-{n}{v}" for n, v in c.knobs)
    parts = [c.group, c.entry, f"d{c.d}", dt, f"hk{c.hk}", sh, c.mask]
    parts += [x for x in (c.feat, "sink" if c.sink else "", f"x{c.splits}" if c.splits != 1 else "")
              if x]
    return "-".join(parts) + kn + "".join(f"-{e}" for e in c.extra)


def _decode_off(sq, hk, d):
    """fwd_decode = 0 where the decode kernel would take a dense launch (the whole GQA group within
    one 32-row tile at a full bucket width)"""
    return (("fwd_decode", 0),) if sq * (H // hk) <= 32 and bucket(d) == d and d <= 128 else ()


def _group_a():
    """fmha_fwd_kernel through fmha_fwd_strided / fmha_fwd_sink: every (NW, MASK, FEAT, sink)
    instantiation of every bucket in both dtypes; the other axes are paired onto the product"""
    T, i = [], 0
    for hd, narrow in ((64, 40), (128, 96), (256, 192)):
        for dt in (BF, FP):
            for nw in ((4, 8) if hd < 256 else (4,)):
                for mask, feat, sink in itertools.product((0, 1), (0, 1), (0, 1)):
                    par = bin(i).count("1") % 2
                    d = narrow if par else hd
                    shape = SHAPES[i % 5]
                    hk = 1 if i % 4 == 3 else 2
                    m = MASKS3[(i // 2) % 3] if mask else "full"
                    # (a sink refuses ALiBi: its FEAT instantiation runs through softcap)
                    ft = "" if not feat else ("softcap" if sink else ("alibi+softcap", "alibi", "softcap")[i % 3])
                    knobs = (("fwd_waves", nw), ("fwd_pipe", i % 3)) + ((("fwd_w4", 0),) if hd == 128 else ())
                    knobs += _decode_off(shape[0], hk, d)
                    T.append(_case("A", "strided", d, dt, hk, shape, m, ft, bool(sink), knobs,
                                   kernel=f"fmha_fwd_kernel<{nw if hd < 256 else 4} waves>",
                                   inst=(hd, nw, bool(mask), bool(feat), bool(sink))))
                    i += 1
    T.append(_case("A", "strided", 160, BF, 2, (129, 63), "causal", "alibi", knobs=(("fwd_waves", 4),),
                   kernel="fmha_fwd_kernel<4 waves>", inst=(256, 4, True, True, False)))
    # fwd_pipe x masks at one narrow d per pipelined bucket, several key tiles
    for hd, d in ((64, 40), (128, 96)):
        for pipe in (0, 1, 2):
            for j, m in enumerate(MASKS3):
                knobs = (("fwd_waves", 8), ("fwd_pipe", pipe)) + ((("fwd_w4", 0),) if hd == 128 else ())
                T.append(_case("A", "strided", d, BF, 2, SHAPES[3 + j % 2], m, knobs=knobs,
                               kernel="fmha_fwd_kernel<8 waves>", inst=(hd, 8, m != "full", False, False),
                               extra=("pipe",)))
    return T


PP_NEED = (("fwd_w4", 4), ("fwd_plain", 1))


def _group_b():
    """the generated D = 128 bodies, dense (strided arenas) and packed, both dtypes"""
    T = []
    # (mask, feature) paired onto (layout, dtype): every body meets both layouts in both dtypes
    plain = [("strided", BF, "causal", ""), ("strided", FP, "w-1_17", ""), ("varlen", BF, "w-1_17", ""),
             ("varlen", FP, "causal", "")]
    full = [("strided", BF, "w64_0", ""), ("varlen", FP, "w64_0", ""), ("strided", FP, "causal", "alibi"),
            ("varlen", BF, "causal", "alibi"), ("strided", BF, "causal", "softcap"),
            ("varlen", FP, "causal", "softcap")]
    m16 = [(e, dt, "full", "") for e in ("strided", "varlen") for dt in (BF, FP)]
    for kern, body, rows in (("fmha_fwdpp_kernel", "plain", plain), ("fmha_fwdpp_kernel", "full", full),
                             ("fmha_fwdpp16_kernel", None, m16)):
        for j, (entry, dt, m, ft) in enumerate(rows):
            T.append(_case("B", entry, 128, dt, 1 if j % 2 else 2, SHAPES[3 + j % 2] if entry == "strided" else (),
                           m, ft, need=PP_NEED, kernel=kern, body=body))
    for dt in (BF, FP):
        T.append(_case("B", "varlen_paged", 128, dt, 2, (), "causal", need=PP_NEED,
                       kernel="fmha_fwdpp_paged_kernel", body="paged"))
        T.append(_case("B", "cache_paged", 128, dt, 2, (33,), "causal", need=PP_NEED,
                       kernel="fmha_fwdpp_paged_kernel", body="paged"))
        # the 4-wave kernel of the variants build (fwd_w4 = 1)
        T.append(_case("B", "strided", 128, dt, 2, SHAPES[4], "causal", knobs=(("fwd_w4", 1),),
                       kernel="fmha_fwd4_kernel", extra=("variants",)))
        T.append(_case("B", "varlen", 128, dt, 2, (), "causal", knobs=(("fwd_w4", 1),),
                       kernel="fmha_fwd4_kernel", extra=("variants",)))
    return T


def _group_c():
    """packed sequences with seqused_k on fmha_fwd_kernel"""
    T = []
    for j, (d, knobs) in enumerate(((64, ()), (256, ()), (128, (("fwd_w4", 0),)))):
        for k, (m, ft) in enumerate((("causal", ""), ("w100_17", ""), ("causal", "alibi"))):
            T.append(_case("C", "varlen", d, (BF, FP)[(j + k) % 2], 2 if k != 1 else 1, (), m, ft,
                           knobs=knobs))
    for d in (64, 256):
        T.append(_case("C", "varlen_paged", d, BF, 2, (), "causal"))
    return T


# cache prefill: 33 query positions x a group of 2 or 4 = 66 / 132 rows, past the decode kernel's 32
ONEPAGE = 272
CACHE_LENS = [272, 200, 77]            # cache_seqlens (leftpad included)
CACHE_LEFTPAD = [3, 13, 45]            # the last keeps 32 keys: under causal, row 0 of 33 sees none
PAGED_LENS = [200, 77, 33]
PAGED_WIDTH = 16                       # 256 keys a table row


def _group_d():
    T = []
    for j, d in enumerate((64, 128, 256)):
        for k, lp in enumerate(("leftpad", "")):
            T.append(_case("D", "cache", d, (BF, FP)[(j + k) % 2], 2 if (j + k) % 2 else 1, (33,),
                           ("causal", "w100_17")[k], extra=(lp,) if lp else ()))
    for d in (64, 256):
        for dt in (BF, FP):
            T.append(_case("D", "cache_paged", d, dt, 2, (33,), "causal" if dt == BF else "w100_17"))
    for d in (64, 128):
        T.append(_case("D", "cache_paged", d, BF, 2, (33,), "causal", extra=("fp8",)))
        T.append(_case("D", "cache", d, FP, 1, (33,), "full", extra=("fp8", "leftpad")))
    return T


def _group_e():
    """fmha_varlen_fwd_fp8 with seqused_k: the 4-wave kernel and the 8-wave one (fp8_w4 = 0, or a
    left window)"""
    T = []
    for dt in (BF, FP):
        T.append(_case("E", "fp8_varlen", 128, dt, 2, (), "causal", need=(("fp8_w4", 1),),
                       kernel="fmha_fwd8w_kernel"))
        T.append(_case("E", "fp8_varlen", 128, dt, 1, (), "full" if dt == BF else "w-1_17",
                       need=(("fp8_w4", 1),), kernel="fmha_fwd8w_kernel"))
        T.append(_case("E", "fp8_varlen", 128, dt, 2, (), "causal", knobs=(("fp8_w4", 0),),
                       kernel="fmha_fwd_fp8_kernel<8 waves>"))
    T.append(_case("E", "fp8_varlen", 128, BF, 2, (), "w100_17", kernel="fmha_fwd_fp8_kernel<8 waves>"))
    return T


def _split_cases():
    """F: fmha_fwd_strided with forced splits; the launch is primed (see the GPU file).  (70, 200)
    under causal: the early rows see keys in the first split only; (33, 325): six key tiles, so
    five splits stay five (the host caps the count at the key tiles: 200 keys give four).
    comb_row is paired on: each head size, split count and mask meets both combines"""
    T = []
    for i, (d, knobs) in enumerate(((64, ()), (128, (("fwd_w4", 0),)))):
        for j, ns in enumerate((2, 5)):
            for k, (m, shape) in enumerate((("full", (33, 325)), ("causal", (70, 200)))):
                cr = (i + j + k) % 2
                T.append(_case("F", "strided", d, BF if cr else FP, 2, shape, m,
                               knobs=knobs + (("comb_row", cr),), splits=ns))
    T.append(_case("F", "strided", 64, BF, 2, (70, 200), "causal", sink=True, knobs=(("comb_row", 1),),
                   splits=5))
    return T


CASES = _group_a() + _group_b() + _group_c() + _group_d() + _group_e()
SPLIT_CASES = _split_cases()


def _isolation():
    """the packed cases whose sequences also run one at a time: one per generated body, and
    fmha_fwd_kernel at d 64, 256 and 128"""
    out, seen = [], set()
    for c in CASES:
        key = (c.kernel, c.body) if c.group == "B" else (c.d, c.mask, c.feat)
        pick = (c.group == "B" and c.need == PP_NEED and c.body != "paged") or (
            c.group == "C" and key in ((64, "causal", ""), (256, "w100_17", ""), (128, "causal", "alibi")))
        if c.entry == "varlen" and pick and key not in seen:
            seen.add(key)
            out.append(c)
    return out


ISOLATION = _isolation()


def expected_splits(c: Case):
    """the host caps a forced split count at the key tiles"""
    return min(c.splits, (c.shape[1] + TILE_K - 1) // TILE_K) if c.splits > 1 else 1


# ------------------------------------------------------------------ problems -------------------
def _data_key(c: Case):
    """what the values of a case depend on"""
    return (c.entry, c.d, c.dtype, c.hk, c.shape, c.feat, c.extra)


@lru_cache(maxsize=None)
def _dense_data(d, dtype, hk, shape, softcap):
    sq, sk = shape
    q, k, v = (su._randn(s, 100 + i, dtype) for i, s in
               enumerate(((B, sq, H, d), (B, sk, hk, d), (B, sk, hk, d))))
    if softcap:
        q = (q.float() * 4).to(dtype)
    return q, k, v


@lru_cache(maxsize=None)
def _packed_data(d, dtype, hk, softcap, fp8=False):
    dt = torch.float32 if fp8 else dtype
    q, k, v = (su._randn(s, 200 + i, dt) for i, s in
               enumerate(((sum(LQ), H, d), (sum(LK), hk, d), (sum(LK), hk, d))))
    if softcap:
        q = (q.float() * 4).to(dt)
    return q, k, v


def _slopes(c: Case, b):
    if "alibi" not in c.feat:
        return None
    return torch.linspace(0.05, 0.5, b * H).view(b, H)


def _own_k_rows(lq, lk, used):
    own = torch.zeros(sum(lk), dtype=torch.bool)
    a = 0
    for nq, n, u in zip(lq, lk, used):
        if nq > 0:
            own[a:a + u] = True
        a += n
    return own


def _cu(lens):
    return torch.tensor([0] + list(itertools.accumulate(lens)), dtype=torch.int32)


def build(c: Case, fill: str, only=None) -> SimpleNamespace:
    """The problem of a case with `fill` everywhere it does not own.  only = i: sequence i of a
    packed case alone (same max_seqlen arguments)."""
    assert fill in FILLS
    p = SimpleNamespace(case=c, fill=fill, entry=c.entry, d=c.d, dtype=c.dtype, h=H, hk=c.hk,
                        window=WINDOWS[c.mask], softcap=SOFTCAP if "softcap" in c.feat else 0.0,
                        sink=sr.sink_values(H) if c.sink else None, splits=c.splits, cache=None,
                        fp8=c.entry == "fp8_varlen", scales=None)
    o_nan = lambda shape: torch.full(shape, NAN, dtype=c.dtype)       # noqa: E731
    if c.entry == "strided":
        q, k, v = _dense_data(c.d, c.dtype, c.hk, c.shape, bool(p.softcap))
        p.b, (p.sq, p.sk) = B, c.shape
        p.slopes = _slopes(c, B)
        p.q, p.k, p.v = (strided_arena(x, fill) for x in (q, k, v))
        p.o = strided_arena(o_nan(q.shape), fill)
        p.lse = lse_arena((B, H, p.sq), fill)
        p.data = (q, k, v)
    elif c.entry in ("varlen", "varlen_paged", "fp8_varlen"):
        q, k, v = _packed_data(c.d, c.dtype, c.hk, bool(p.softcap), p.fp8)
        lq, lk, used = list(LQ), list(LK), list(USED)
        slopes = _slopes(c, len(LQ))
        if only is not None:
            sl_q, sl_k = sr.seq_slices(LQ)[only], sr.seq_slices(LK)[only]
            q, k, v = q[sl_q], k[sl_k], v[sl_k]
            lq, lk, used = [LQ[only]], [LK[only]], [USED[only]]
            slopes = slopes[only:only + 1] if slopes is not None else None
        if p.fp8:
            assert only is None
            (q, qs), (k, ks), (v, vs) = (orc.quantize_fp8(x) for x in (q, k, v))
            p.scales = (qs, ks, vs)
        p.b, p.lq, p.lk, p.used, p.slopes = len(lq), lq, lk, used, slopes
        p.max_sq, p.max_sk = max(LQ), max(LK)
        p.q = packed_arena(q, fill)
        p.o = packed_arena(o_nan(q.shape), fill)
        p.lse = lse_arena((1, H, sum(lq)), fill)
        if c.entry == "varlen_paged":
            ks_ = [k[s][:u].float() if nq > 0 else k[s][:0].float()
                   for s, u, nq in zip(sr.seq_slices(lk), used, lq)]
            vs_ = [v[s][:u].float() if nq > 0 else v[s][:0].float()
                   for s, u, nq in zip(sr.seq_slices(lk), used, lq)]
            p.cache = du.build_cache(ks_, vs_, PAGE, (max(LK) + PAGE - 1) // PAGE, False, c.dtype, fill,
                                     seed=7)
            p.max_sk = p.cache.width * PAGE
            p.k = p.v = None
        else:
            own = _own_k_rows(lq, lk, used)
            p.k, p.v = packed_arena(k, fill, own), packed_arena(v, fill, own)
        p.data = (q, k, v)
    else:                                               # cache, cache_paged
        fp8, leftpad = "fp8" in c.extra, "leftpad" in c.extra
        sq = c.shape[0]
        if c.entry == "cache":
            lens, lp, page, width = CACHE_LENS, (CACHE_LEFTPAD if leftpad else None), ONEPAGE, 1
        else:
            lens, lp, page, width = PAGED_LENS, None, PAGE, PAGED_WIDTH
        ks_, vs_ = du.make_kv(lens, c.hk, c.d, 300 + c.d, lp)
        p.cache = du.build_cache(ks_, vs_, page, width, fp8, c.dtype, fill, leftpad=lp, seed=c.d)
        q = du.make_q(len(lens), sq, H, c.d, c.dtype, 301)
        p.b, p.sq, p.max_sk, p.slopes = len(lens), sq, width * page, None
        p.q = batched_arena(q, fill)
        p.o = batched_arena(o_nan(q.shape), fill)
        p.lse = lse_arena((p.b, H, sq), fill)
        p.k = p.v = None
        p.data = (q, None, None)
    return p


def _norm_window(window, sk):
    wl, wr = window
    return (wl, sk) if (wl >= 0 and wr < 0) else (wl, wr)


def _dense_refs(q, k, v, window, softcap, slopes, sink):
    """(ref, pt, lse) of one dense problem: the project's references of the entry"""
    w = _norm_window(window, k.shape[1])
    if sink is not None:
        r = sr.fwd_refs(q, k, v, sink, window=w, softcap=softcap)
        return r.ref64.float(), r.pt, r.lse64.float()
    r = su.refs(q, k, v, w, softcap, slopes, apriori=False)
    return r.ref, r.pt, r.lse


def _oracle(p) -> Oracle:
    c = p.case
    if c.entry == "strided":
        q, k, v = p.data
        return Oracle(*_dense_refs(q, k, v, p.window, p.softcap, p.slopes, p.sink), 2.0, 0.0)
    if c.entry in ("cache", "cache_paged"):
        t = p.cache
        if t.fp8:
            # the prefill kernel dequantises while staging: its operand is dtype(float(fp8) * scale),
            # the conversion tests/test_fwd_gpu.py's fp8 cache oracle is defined over (the decode
            # kernel applies the scales in fp32 to S and O instead)
            t = t._replace(kx=[x.to(c.dtype).float() for x in t.kx], vx=[x.to(c.dtype).float() for x in t.vx])
        o = du.oracle(t, p.data[0], p.window, p.softcap, p.slopes)
        return Oracle(o.ref, o.pt, o.lse, 3.0, 1e-5)
    q, k, v = p.data
    tq = q.shape[0]
    odt = torch.float32
    ref, pt = torch.zeros(1, tq, H, c.d, dtype=odt), torch.zeros(1, tq, H, c.d, dtype=odt)
    lse = torch.full((1, H, tq), INF)
    for i, (sq_, sk_) in enumerate(zip(sr.seq_slices(p.lq), sr.seq_slices(p.lk))):
        n = p.used[i]
        if p.lq[i] == 0 or n == 0:
            continue
        if p.fp8:
            w = _norm_window(p.window, n)
            r = su.fp8_refs(q[sq_][None], k[sk_][:n][None], v[sk_][:n][None], *p.scales, w, c.dtype)
            rr, pp, ll = r.ref, r.pt, r.lse
        elif p.cache is not None:
            kx, vx = p.cache.kx[i][None].to(c.dtype), p.cache.vx[i][None].to(c.dtype)
            rr, pp, ll = _dense_refs(q[sq_][None], kx, vx, p.window, p.softcap,
                                     p.slopes[i:i + 1] if p.slopes is not None else None, None)
        else:
            rr, pp, ll = _dense_refs(q[sq_][None], k[sk_][:n][None], v[sk_][:n][None], p.window, p.softcap,
                                     p.slopes[i:i + 1] if p.slopes is not None else None, None)
        ref[0, sq_], pt[0, sq_], lse[0, :, sq_] = rr[0].float(), pp[0].float(), ll[0]
    return Oracle(ref, pt, lse, 3.0 if p.fp8 else 2.0, 1e-3 if p.fp8 else 0.0)


_ORACLES = {}


def oracle(c: Case) -> Oracle:
    """once per problem: the cases that differ in knobs only share it"""
    key = (_data_key(c), c.mask, c.sink)
    if key not in _ORACLES:
        _ORACLES[key] = _oracle(build(c, "zero"))
    return _ORACLES[key]


# ------------------------------------------------------------------ the launch -----------------
def session_skip(c: Case, L=None):
    """the `_need` rule: the reason to skip when the session's knobs (XFA_TEST_OPTIONS) send the
    launch to another kernel than the one the case asserts, else None"""
    from xf_flash_attention_cutlass_amd import capi
    L = L or capi.lib()
    for name, value in c.need:
        have = L.fmha_get_option(name.encode())
        if name not in dict(c.knobs) and have != value:
            return f"the kernel this case asserts needs {name} = {value}; the session runs {name} = {have}"
    return None


class _lib_option:
    """`_option` on another build of the library (the variants build's own knob table)"""

    def __init__(self, L, name, value):
        self.L, self.name, self.value = L, name.encode(), value

    def __enter__(self):
        self.old = self.L.fmha_get_option(self.name)
        assert self.L.fmha_set_option(self.name, self.value) == 0

    def __exit__(self, *exc):
        assert self.L.fmha_set_option(self.name, self.old) == 0


def _ptr(a: Arena, dbuf):
    return dbuf.data_ptr() + a.base * dbuf.element_size()


def launch(p, L=None) -> Out:
    """One call of the case's entry on device copies of the arenas, under the case's knobs (restored
    afterwards).  Returns every buffer as it is after the call, on the CPU."""
    import ctypes

    from xf_flash_attention_cutlass_amd import capi
    c = p.case
    own_lib = L is not None
    L = L or capi.lib()
    dev = {n: getattr(p, n).buf.to(DEV) for n in ("q", "k", "v", "o", "lse") if getattr(p, n) is not None}
    ptr = {n: _ptr(getattr(p, n), t) for n, t in dev.items()}
    fp16 = c.dtype == FP
    wl, wr = p.window
    sl = p.slopes.to(DEV).contiguous() if p.slopes is not None else None
    sink = p.sink.to(DEV) if p.sink is not None else None
    scale = c.d ** -0.5
    stream = capi.stream_handle()
    cache = p.cache
    if cache is not None:
        dev["k"], dev["v"] = cache.kc.to(DEV), cache.vc.to(DEV)
        ptr["k"], ptr["v"] = dev["k"].data_ptr(), dev["v"].data_ptr()
        tab = cache.table.to(DEV)
    before = {n: dev[n].clone() for n in "qkv"}
    with ExitStack() as st:
        for n, v in c.knobs:
            st.enter_context(_lib_option(L, n, v) if own_lib else _option(n, v))
        if c.entry == "strided":
            strides = (ctypes.c_int64 * 12)(*[s for n in "qkvo" for s in getattr(p, n).strides[:3]])
            args = [ptr["q"], ptr["k"], ptr["v"], ptr["o"], capi.ptr(sl), ptr["lse"], p.sq, p.sk, p.b, H,
                    c.hk, c.d, strides, scale, wl, wr, p.softcap, fp16, p.splits, stream, 0.0, None]
            if sink is None:
                L.fmha_fwd_strided(*args)
            else:
                L.fmha_fwd_sink(*args, sink.data_ptr())
        elif c.entry in ("varlen", "varlen_paged", "fp8_varlen"):
            cu_q = _cu(p.lq).to(DEV)
            used = torch.tensor(p.used, dtype=torch.int32).to(DEV)
            tq = sum(p.lq)
            if c.entry == "fp8_varlen":
                cu_k = _cu(p.lk).to(DEV)
                L.fmha_varlen_fwd_fp8(ptr["q"], ptr["k"], ptr["v"], ptr["o"], ptr["lse"], cu_q.data_ptr(),
                                      cu_k.data_ptr(), used.data_ptr(), *p.scales, p.max_sq, p.max_sk, tq,
                                      p.b, H, c.hk, c.d, scale, wl, wr, fp16, stream)
            elif cache is None:
                cu_k = _cu(p.lk).to(DEV)
                L.fmha_varlen_fwd_ex(ptr["q"], ptr["k"], ptr["v"], ptr["o"], ptr["lse"], cu_q.data_ptr(),
                                     cu_k.data_ptr(), used.data_ptr(), None, 0, 0, capi.ptr(sl), H,
                                     p.max_sq, p.max_sk, tq, p.b, H, c.hk, c.d, scale, wl, wr, p.softcap,
                                     fp16, stream, 0.0, None)
            else:
                lens = torch.tensor(cache.lens, dtype=torch.int32).to(DEV)
                L.fmha_varlen_fwd_ex(ptr["q"], ptr["k"], ptr["v"], ptr["o"], ptr["lse"], cu_q.data_ptr(),
                                     None, lens.data_ptr(), tab.data_ptr(), tab.stride(0), cache.page,
                                     capi.ptr(sl), H, p.max_sq, p.max_sk, tq, p.b, H, c.hk, c.d, scale, wl,
                                     wr, p.softcap, fp16, stream, 0.0, None)
        else:
            lens = torch.tensor(cache.lens, dtype=torch.int32).to(DEV)
            lp = torch.tensor(cache.leftpad, dtype=torch.int32).to(DEV) if cache.leftpad is not None else None
            L.fmha_page_kvcache_fwd_ex(ptr["q"], ptr["k"], ptr["v"], ptr["o"], ptr["lse"], tab.data_ptr(),
                                       tab.stride(0), lens.data_ptr(), p.sq, p.max_sk, p.b, H, c.hk, c.d,
                                       cache.page, scale, wl, wr, p.softcap, capi.ptr(sl), H, p.splits,
                                       1 if cache.fp8 else 0, cache.k_scale, cache.v_scale, capi.ptr(lp),
                                       fp16, stream)
        assert L.fmha_last_status() == 0, L.fmha_last_error().decode()
        torch.cuda.synchronize()
        kern, splits = L.fmha_last_kernel().decode(), L.fmha_last_num_splits()
    if cache is not None:
        assert torch.equal(tab.cpu(), cache.table)
    # the inputs are compared on the device and come back only where they changed
    ins = [b if torch.equal(_bits(dev[n]), _bits(before[n])) else dev[n].cpu()
           for n, b in zip("qkv", _inputs_before(p))]
    return Out(*ins, dev["o"].cpu(), dev["lse"].cpu(), kern, splits)


# ------------------------------------------------------------------ the conditions -------------
def _inputs_before(p):
    """(q, k, v) buffers as handed to the call"""
    if p.cache is not None:
        return p.q.buf, p.cache.kc, p.cache.vc
    return p.q.buf, p.k.buf, p.v.buf


def expected_name(c: Case):
    """(prefix, required substrings, suffix) of fmha_last_kernel()"""
    subs = [f" body={c.body}"] if c.body else []
    suffix = ""
    if c.sink:
        suffix = " sink=combine" if c.splits > 1 else (" sink=epilogue" if c.kernel.startswith("fmha_fwd_kernel") else " sink=pass")
    return c.kernel + ("" if c.kernel.endswith("<") else " "), subs, suffix


def name_ok(c: Case, kern: str, splits: int):
    pre, subs, suffix = expected_name(c)
    if not (kern + " ").startswith(pre) or not all(s in kern + " " for s in [x + " " for x in subs]):
        return False
    if suffix and not kern.endswith(suffix):
        return False
    if not c.body and " body=" in kern:
        return False
    return splits == expected_splits(c)


def judge_case(c: Case, probs, outs, ora: Oracle, rows=None):
    """The conditions of one problem under the three fills; returns the failures as
    (fill, condition, text).

      1  O and LSE over the owned region hold no NaN and no Inf, except LSE = +inf exactly on the
         rows the oracle leaves without a key, where O is exactly 0
      2  O and LSE under `nan` and `big` are bit-identical to those under `zero`
      3  every element of the o arena outside the view and of the LSE guards keeps its bits, and
         so do the q / k / v arenas
      4  the `nan` run meets the entry's rule against the oracle over the owned data
      5  the kernel name, its body= field and the split count are the ones the case names
    """
    fails, res = [], {}
    dead = torch.isinf(ora.lse) & (ora.lse > 0)                      # [b, h, rows]
    for fill in FILLS:
        p, out = probs[fill], outs[fill]
        o, lse = view(p.o, out.o), view(p.lse, out.lse)
        res[fill] = (o, lse)
        of = o.float()
        dead_o = dead.permute(0, 2, 1)
        if not torch.isfinite(of).all():
            fails.append((fill, 1, f"{int((~torch.isfinite(of)).sum())} non-finite O values"))
        elif bool((of[dead_o] != 0).any()):
            fails.append((fill, 1, "O is not 0 on a row without a key"))
        if torch.isnan(lse).any() or bool(torch.isneginf(lse).any()):
            fails.append((fill, 1, "LSE holds NaN or -inf"))
        elif not torch.equal(torch.isinf(lse), dead):
            fails.append((fill, 1, "the LSE's +inf rows are not the rows without a key"))
        stray = (_bits(out.o) != _bits(p.o.buf)) & ~p.o.owned
        if bool(stray.any()):
            fails.append((fill, 3, f"{int(stray.sum())} elements of the o arena outside the view were written"))
        if bool(((_bits(out.lse) != _bits(p.lse.buf)) & ~p.lse.owned).any()):
            fails.append((fill, 3, "an LSE guard was written"))
        for name, after, before in zip("qkv", (out.q, out.k, out.v), _inputs_before(p)):
            if not torch.equal(_bits(after).flatten(), _bits(before).flatten()):
                fails.append((fill, 3, f"the {name} arena changed"))
        if not name_ok(c, out.kern, out.splits):
            fails.append((fill, 5, f"ran {out.kern!r} with {out.splits} splits, wanted {expected_name(c)} "
                                   f"with {expected_splits(c)}"))
    for fill in ("nan", "big"):
        for what, a, b in zip(("O", "LSE"), res[fill], res["zero"]):
            if not torch.equal(_bits(a), _bits(b)):
                n = int((_bits(a) != _bits(b)).sum())
                fails.append((fill, 2, f"{what} differs from the zero fill's in {n} elements"))
    o, lse = res["nan"]
    _, err, bound = orc.parity_ok(o, ora.ref, ora.pt, ora.mult, ora.atol)
    fin = ~dead
    dl = (lse[fin] - ora.lse[fin]).abs() - LSE_RTOL * ora.lse[fin].abs()
    lse_err = dl.max().item() if dl.numel() else 0.0
    if not err <= bound:
        fails.append(("nan", 4, f"max|O - ref| = {err:.3e} > {bound:.3e}"))
    if not lse_err <= LSE_ATOL:
        fails.append(("nan", 4, f"LSE off by {lse_err:.3e} > {LSE_ATOL:.0e}"))
    if rows is not None:
        kn = outs["nan"].kern.split(" persistent=")[0]
        rows.append(dict(case=case_id(c), group=c.group, metric="o", err=err, bound=bound, kernel=kn,
                         ok=bool(err <= bound)))
        rows.append(dict(case=case_id(c), group=c.group, metric="lse", err=lse_err, bound=LSE_ATOL,
                         kernel=kn, ok=bool(lse_err <= LSE_ATOL)))
    return fails


def check_case(c: Case, run, report=None, builder=build):
    """`run(problem) -> Out` under the three fills of one problem; asserts the five conditions"""
    probs = {f: builder(c, f) for f in FILLS}
    outs = {f: run(probs[f]) for f in FILLS}
    rows = []
    fails = judge_case(c, probs, outs, oracle(c), rows)
    for r in rows:
        print(f"{r['case']} {r['metric']}: err {r['err']:.3e} bound {r['bound']:.3e} [{r['kernel']}]")
        if report is not None:
            report(r)
    assert not fails, f"{case_id(c)}: {fails}"
    return outs


# ------------------------------------------------------------------ the CPU model --------------
DEFECTS = ("v_tail", "slot_limit", "k_bucket", "leftpad_rows", "o_tile", "stale_partial")


def _gather(buf, idx):
    assert int(idx.min()) >= 0 and int(idx.max()) < buf.numel(), "the model left its arena"
    return buf[idx].float()


def _row_index(a: Arena, b, rows, head):
    """flat element indices [len(rows)] of (b, row, head, 0)"""
    return a.base + b * a.strides[0] + rows * a.strides[1] + head * a.strides[2]


def model_launch(p, defect=None) -> Out:
    """A tiled float32 forward of the problem, read from the arenas as a kernel does: whole 64-key
    tiles and whole 32-row tiles of the GQA-packed rows, whatever lies there, then the predicates.
    The split scratch starts as the problem's fill.  defect, one of DEFECTS:
      v_tail         V rows at or past the key limit are not zeroed (their scores are masked)
      slot_limit     the key limit is the slot length / the cache capacity, not seqused_k
      k_bucket       K chunks are read out to the bucket width (Q is zero there)
      leftpad_rows   the rows in front of cache_leftpad are included
      o_tile         the whole 32-row tile of O is stored
      stale_partial  the partial of a split without a visible key stays as the scratch held it
    No ALiBi, softcap, sink or fp8: the model exists to show what the conditions reject."""
    assert defect is None or defect in DEFECTS
    c = p.case
    assert not p.softcap and p.slopes is None and p.sink is None and not p.fp8
    d, G = c.d, H // c.hk
    W = bucket(d) if defect == "k_bucket" else d
    cache = p.cache
    assert cache is None or not cache.fp8
    packed = c.entry.startswith("varlen")
    nb = p.b
    o_buf, lse_buf = p.o.buf.clone(), p.lse.buf.clone()
    o_flat = o_buf.float()
    stored = torch.zeros_like(p.o.owned)
    wl, wr = p.window
    max_sk = p.sk if c.entry == "strided" else p.max_sk
    if wl < 0 <= wr:
        wl = max_sk
    if wr < 0 <= wl:
        wr = max_sk
    cu_q = _cu(p.lq).tolist() if packed else None
    cu_k = _cu(p.lk).tolist() if packed and cache is None else None
    ns = expected_splits(c)
    scratch_val = {"zero": 0.0, "nan": NAN, "big": torch.finfo(torch.float32).max}[p.fill]
    cols = torch.arange(W)
    for b in range(nb):
        if packed:
            q_off, sq = cu_q[b], p.lq[b]
        else:
            q_off, sq = 0, p.sq
        lp = 0
        if cache is not None:
            sk = cache.lens[b]
            lp = cache.leftpad[b] if cache.leftpad is not None else 0
            cap = cache.width * cache.page
            if defect == "slot_limit":
                sk = cap
            if defect == "leftpad_rows":
                lp = 0
            sk -= lp
        elif packed:
            sk = (p.lk[b] if defect == "slot_limit" else p.used[b])
        else:
            sk = p.sk
        if sq == 0:
            continue
        rows_total, diag = sq * G, sk - sq
        qb = 0 if packed else b
        for kh in range(c.hk):
            for t0 in range(0, rows_total, TILE_M):
                r = t0 + torch.arange(TILE_M)
                pos, g = r // G, r % G
                head = kh * G + g
                row_ok = r < rows_total
                # the whole row tile of Q, d columns, zero-padded to W; rows past the end are zero
                qi = _row_index(p.q, qb, q_off + pos, head)
                qt = _gather(p.q.buf, qi[:, None] + torch.arange(d)[None])
                qt = torch.where(row_ok[:, None], qt, torch.zeros_like(qt))
                qt = torch.cat([qt, torch.zeros(TILE_M, W - d)], 1)
                lim_r = torch.clamp(pos + diag + wr + 1, max=sk) if wr >= 0 else torch.full_like(pos, sk)
                lim_l = torch.clamp(pos + diag - wl, min=0) if wl >= 0 else torch.zeros_like(pos)
                pos_lo, pos_hi = t0 // G, (min(t0 + TILE_M, rows_total) - 1) // G
                n_lo = max(0, pos_lo + diag - wl) if wl >= 0 else 0
                n_hi = min(sk, pos_hi + diag + wr + 1) if wr >= 0 else sk
                t_lo = n_lo // TILE_K
                t_hi = (n_hi + TILE_K - 1) // TILE_K if n_hi > n_lo else t_lo
                per = (t_hi - t_lo + ns - 1) // ns
                po = torch.full((ns, TILE_M, d), scratch_val)
                pl = torch.full((ns, TILE_M), scratch_val)
                for s in range(ns):
                    s_lo = min(t_lo + s * per, t_hi) if ns > 1 else t_lo
                    s_hi = min(t_hi, s_lo + per) if ns > 1 else t_hi
                    m = torch.full((TILE_M,), -INF)
                    l = torch.zeros(TILE_M)
                    acc = torch.zeros(TILE_M, d)
                    for t in range(s_lo, s_hi):
                        key = t * TILE_K + torch.arange(TILE_K)
                        if cache is not None:
                            rr = lp + key
                            pi = (rr // cache.page).clamp(max=cache.width - 1)
                            pg = cache.table[b, pi].long()
                            ki = ((pg * cache.page + rr % cache.page) * c.hk + kh) * d
                            kt = _gather(cache.kc.flatten(), ki[:, None] + cols[None])
                            vt = _gather(cache.vc.flatten(), ki[:, None] + torch.arange(d)[None])
                        else:
                            k_off = cu_k[b] if packed else 0
                            ki = _row_index(p.k, qb if packed else b, k_off + key, kh)
                            vi = _row_index(p.v, qb if packed else b, k_off + key, kh)
                            kt = _gather(p.k.buf, ki[:, None] + cols[None])
                            vt = _gather(p.v.buf, vi[:, None] + torch.arange(d)[None])
                        st = (qt @ kt.T) * d ** -0.5
                        dead = (key[None] >= lim_r[:, None]) | (key[None] < lim_l[:, None]) | ~row_ok[:, None]
                        st = torch.where(dead, torch.tensor(-INF), st)
                        if defect != "v_tail":
                            vt = torch.where((key >= sk)[:, None], torch.zeros_like(vt), vt)
                        m_new = torch.maximum(m, st.amax(-1))
                        mref = torch.where(torch.isneginf(m_new), torch.zeros_like(m_new), m_new)
                        alpha = torch.where(torch.isneginf(m), torch.ones_like(m), torch.exp(m - mref))
                        pr = torch.exp(st - mref[:, None])
                        l = l * alpha + pr.sum(-1)
                        acc = acc * alpha[:, None] + pr.to(c.dtype).float() @ vt
                        m = m_new
                    empty = (l == 0) | torch.isnan(l)
                    part_o = acc / torch.where(empty, torch.ones_like(l), l)[:, None]
                    part_l = torch.where(empty, torch.tensor(-INF), m + torch.log(l))
                    if defect == "stale_partial" and ns > 1:
                        keep = (l == 0)
                        part_o = torch.where(keep[:, None], po[s], part_o)
                        part_l = torch.where(keep, pl[s], part_l)
                    po[s], pl[s] = part_o, part_l
                if ns > 1:
                    mx = pl.amax(0)
                    safe = torch.where(torch.isneginf(mx), torch.zeros_like(mx), mx)
                    sm = torch.exp(pl - safe[None]).sum(0)
                    none = torch.isneginf(mx) | (sm == 0)
                    ls = torch.where(none, torch.tensor(INF), torch.log(sm) + safe)
                    w = torch.where(none[None], torch.zeros_like(pl), torch.exp(pl - ls[None]))
                    ot = (w[..., None] * po).sum(0)
                else:
                    ot = po[0]
                    ls = torch.where(torch.isneginf(pl[0]), torch.tensor(INF), pl[0])
                store = torch.ones_like(row_ok) if defect == "o_tile" else row_ok
                oi = _row_index(p.o, qb, q_off + pos, head)[store]
                idx = oi[:, None] + torch.arange(d)[None]
                assert int(idx.min()) >= 0 and int(idx.max()) < o_flat.numel(), "the model left its arena"
                o_flat[idx] = ot[store]
                stored[idx] = True
                li = p.lse.base + qb * p.lse.strides[0] + head[row_ok] * p.lse.strides[1] + (q_off + pos[row_ok])
                lse_buf[li] = ls[row_ok]
    # only what the model stored is converted: everything else keeps its bits
    o_buf = torch.where(stored, o_flat.to(c.dtype), o_buf)
    qb_, kb_, vb_ = _inputs_before(p)
    pre, subs, suffix = expected_name(c)
    kern = pre.rstrip() + (">" if pre.endswith("<") else "") + "".join(subs) + " persistent=0" + suffix
    return Out(qb_.clone(), kb_.clone(), vb_.clone(), o_buf, lse_buf, kern, ns)
