"""Shared helpers of the MLA prefill tests (not a conftest: imported explicitly).

MLA prefill (the un-absorbed form): q and k carry 192 features a head, v and the output 128;
S = scale q K^T over all 192, O = softmax(S) V, LSE = logsumexp(S).

* `make_packed`: unit-randn packed q / k / v of given per-sequence lengths.
* `oracle`: per sequence `orc.attention_ref` / `orc.attention_lse_ref` (they take a V of another
  width and scale by q.shape[-1]); the low-precision twin is `upcast=False, reorder_ops=True`.  A
  scale other than 192^-1/2 is carried by q pre-multiplied with `q_mul` (a power of two: exact).
* `judge_each` / `assert_case`: the project's forward rule (`softmax_stress_util.judge`: max|o - ref|
  <= 2 max|pt - ref|, the LSE within LSE_ATOL + LSE_RTOL |ref| with the oracle's +inf pattern, no
  NaN) PER SEQUENCE, so a short sequence cannot hide a long one.
* `emulate`: the kernel's arithmetic on the CPU, tile by tile (64-key tiles, fp32 accumulation, P
  rounded to the dtype, deferred rescale), with the defects of DEFECTS plantable.
* `run_varlen` / `run_dense`: one call through the C ABI into NaN-filled outputs (or the caller's
  views); asserts the kernel id.
"""
from __future__ import annotations

import ctypes as C
import itertools
import math
from collections import namedtuple

import torch

from oracle import attention_ref as orc
from tests import softmax_stress_util as su

DEV = "cuda"
DQK, DV = 192, 128
TILE = 64
KERNEL = "fmha_fwd_mla_kernel"
ROWS = 256                                   # query rows (positions x group) of one work item
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
DEFECTS = ("v_from_k", "qk128", "scale128", "topleft", "no_dtile3")
# the smallest lengths that reach every path of a 64-key-tile, 256-row-item kernel: 6 tiles (a full
# ring, a remainder and a ragged last tile), sk > sq, sk >> sq = 1, and an empty sequence
LENS_Q = [300, 113, 1, 31]
LENS_K = [333, 203, 147, 0]
LENS_K_REV = [113, 300, 0, 147]              # sk < sq under causal: rows that see no key

Seq = namedtuple("Seq", "ref pt lse")        # of one sequence: [1, sq, h, 128] x 2, [1, h, sq]


def cu(lens):
    return torch.tensor([0] + list(itertools.accumulate(lens)), dtype=torch.int32)


def make_packed(lens_q, lens_k, h, hk, dtype, seed=0):
    g = torch.Generator().manual_seed(1200 + seed)
    q = torch.randn(sum(lens_q), h, DQK, generator=g).to(dtype)
    k = torch.randn(sum(lens_k), hk, DQK, generator=g).to(dtype)
    v = torch.randn(sum(lens_k), hk, DV, generator=g).to(dtype)
    return q, k, v


def window_of(causal, window):
    return (-1, 0) if causal else tuple(window)


def oracle_one(q, k, v, window=(-1, -1), q_mul=1.0) -> Seq:
    """q [sq, h, 192], k [sk, hk, 192], v [sk, hk, 128] of one sequence."""
    sq, h, _ = q.shape
    if k.shape[0] == 0 or sq == 0:
        return Seq(torch.zeros(1, sq, h, DV, dtype=q.dtype), torch.zeros(1, sq, h, DV, dtype=q.dtype),
                   torch.full((1, h, sq), float("inf")))
    qi = (q[None].float() * q_mul).to(q.dtype)
    kw = dict(window_size=tuple(window))
    ref, _ = orc.attention_ref(qi, k[None], v[None], **kw)
    pt, _ = orc.attention_ref(qi, k[None], v[None], upcast=False, reorder_ops=True, **kw)
    lse = orc.attention_lse_ref(qi, k[None], **kw)
    return Seq(ref, pt, lse)


def oracle(q, k, v, lens_q, lens_k, window=(-1, -1), q_mul=1.0, used_k=None):
    """Packed inputs -> [Seq per sequence]; used_k: seqused_k (the first used_k[i] keys of i)."""
    out, a, b = [], 0, 0
    for i, (nq, nk) in enumerate(zip(lens_q, lens_k)):
        n = nk if used_k is None else used_k[i]
        out.append(oracle_one(q[a:a + nq], k[b:b + n], v[b:b + n], window, q_mul))
        a, b = a + nq, b + nk
    return out


def judge_each(o, lse, seqs, lens_q):
    """o [total_q, h, 128], lse [h, total_q] (CPU) against [Seq].  Returns (all ok, [figures])."""
    figs, good, a = [], True, 0
    for s, nq in zip(seqs, lens_q):
        if nq == 0:
            continue
        ok, f = su.judge(o[a:a + nq][None], lse[:, a:a + nq][None], su.Refs(s.ref, s.pt, s.lse, None))
        f["ok"] = ok
        f["ratio"] = f["err"] / f["bound"] if f["bound"] > 0 else (0.0 if f["err"] == 0 else float("inf"))
        figs.append(f)
        good = good and ok
        a += nq
    return good, figs


def assert_case(name, o, lse, seqs, lens_q, report=None):
    ok, figs = judge_each(o, lse, seqs, lens_q)
    worst = max(figs, key=lambda f: f["ratio"])
    lse_err = max(f["lse_err"] for f in figs)
    print(f"{name}: worst o err / bound {worst['ratio']:.3f} ({worst['err']:.3e} / {worst['bound']:.3e}); "
          f"lse err {lse_err:.3e}")
    if report is not None:
        report(dict(case=name, metric="o", err=worst["err"], bound=worst["bound"], ok=bool(ok)))
        report(dict(case=name, metric="lse", err=lse_err, bound=su.LSE_ATOL, ok=bool(ok)))
    assert ok, f"{name}: {[(i, f) for i, f in enumerate(figs) if not f['ok']]}"
    return worst["ratio"]


# ------------------------------------------------------------------ the kernel's arithmetic ----
def emulate_one(q, k, v, window=(-1, -1), scale=None, slack=8.0, defect=None):
    """One sequence as the kernel computes it: per 64-key tile S = K Q^T accumulated in fp32,
    X = S c - m with c = scale log2(e) and the running max m moved only when some score of the
    tile exceeds it by more than `slack` (or at the row's first visible key), P = exp2(X) summed
    in fp32 and rounded to the dtype for the PV product, O accumulated in fp32, one division at the
    end; LSE = (m + log2 l) ln 2; a row without a visible key gives 0 and +inf.
    Returns (o [sq, h, 128] in the dtype, lse [h, sq] fp32)."""
    assert defect is None or defect in DEFECTS
    sq, h, _ = q.shape
    sk, hk, _ = k.shape
    g = h // hk
    dqk = 128 if defect == "qk128" else DQK
    c = (scale if scale is not None else DQK ** -0.5) * math.log2(math.e)
    if defect == "scale128":
        c = 128 ** -0.5 * math.log2(math.e)
    wl, wr = window
    diag = 0 if defect == "topleft" else sk - sq
    pos = torch.arange(sq).view(-1, 1)
    qf = q.float()[..., :dqk].permute(1, 0, 2)                          # [h, sq, d]
    kf = k.float()[..., :dqk].repeat_interleave(g, dim=1).permute(1, 0, 2)
    vsrc = k[..., :DV] if defect == "v_from_k" else v
    vf = vsrc.float().repeat_interleave(g, dim=1).permute(1, 0, 2)      # [h, sk, 128]
    m = torch.full((h, sq), float("-inf"))
    l = torch.zeros(h, sq)
    acc = torch.zeros(h, sq, DV)
    for n0 in range(0, sk, TILE):
        n1 = min(sk, n0 + TILE)
        key = torch.arange(n0, n1).view(1, -1)
        vis = torch.ones(sq, n1 - n0, dtype=torch.bool)
        if wr >= 0:
            vis &= key <= pos + diag + wr
        if wl >= 0:
            vis &= key >= pos + diag - wl
        s = torch.matmul(qf, kf[:, n0:n1].transpose(1, 2))             # fp32 accumulation
        x = torch.where(vis[None], s * c, torch.full_like(s, float("-inf")))
        mx = x.max(dim=-1).values
        fresh = torch.isinf(m) & (m < 0)
        m_new = torch.where(fresh, mx, torch.where(mx > m + slack, mx, m))
        alpha = torch.where(torch.isinf(m) | torch.isinf(m_new), torch.ones_like(m), torch.exp2(m - m_new))
        l, acc, m = l * alpha, acc * alpha[..., None], m_new
        mref = torch.where(torch.isinf(m), torch.zeros_like(m), m)
        p = torch.exp2(x - mref[..., None])
        l = l + p.sum(-1)
        acc = acc + torch.matmul(p.to(q.dtype).float(), vf[:, n0:n1])
    empty = l == 0
    o = torch.where(empty[..., None], torch.zeros_like(acc), acc / torch.where(empty, torch.ones_like(l), l)[..., None])
    if defect == "no_dtile3":
        o[..., 96:] = 0
    lse = torch.where(empty, torch.full_like(l, float("inf")), (m + torch.log2(l)) * math.log(2.0))
    return o.permute(1, 0, 2).to(q.dtype).contiguous(), lse


def emulate(q, k, v, lens_q, lens_k, window=(-1, -1), defect=None):
    """Packed -> (o [total_q, h, 128], lse [h, total_q])."""
    os_, ls, a, b = [], [], 0, 0
    for nq, nk in zip(lens_q, lens_k):
        o, l = emulate_one(q[a:a + nq], k[b:b + nk], v[b:b + nk], window, defect=defect)
        os_.append(o)
        ls.append(l)
        a, b = a + nq, b + nk
    return torch.cat(os_), torch.cat(ls, dim=1)


# ------------------------------------------------------------------ launches -------------------
def _check_kernel(L):
    from xf_flash_attention_cutlass_amd import capi
    capi.check()
    kern = L.fmha_last_kernel().decode()
    assert kern.startswith(KERNEL + " persistent="), f"ran {kern!r}, wanted {KERNEL}"
    assert "block=512" in kern, kern
    assert L.fmha_last_num_splits() == 1
    return kern


def run_varlen(q, k, v, lens_q, lens_k, h, hk, window=(-1, -1), scale=None, used_k=None, o=None, lse=None,
               sync=True, cus=None):
    """fmha_varlen_fwd_mla on device tensors (views are fine).  o / lse: device tensors to write
    (lse contiguous [h, total_q]); else NaN-filled ones are made.  cus: (cu_seqlens_q, cu_seqlens_k)
    already on the device (a call under graph capture must not copy them there).  Returns
    (o, lse, kernel)."""
    from xf_flash_attention_cutlass_amd import capi
    L = capi.lib()
    total_q = sum(lens_q)
    if o is None:
        o = torch.full((total_q, h, DV), float("nan"), dtype=q.dtype, device=DEV)
    if lse is None:
        lse = torch.full((h, total_q), float("nan"), dtype=torch.float32, device=DEV)
    cq, ck = cus if cus is not None else (cu(lens_q).to(DEV), cu(lens_k).to(DEV))
    used = None if used_k is None else torch.tensor(used_k, dtype=torch.int32, device=DEV)
    st = (C.c_int64 * 8)(q.stride(0), q.stride(1), k.stride(0), k.stride(1), v.stride(0), v.stride(1),
                         o.stride(0), o.stride(1))
    L.fmha_varlen_fwd_mla(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr(),
                          cq.data_ptr(), ck.data_ptr(), capi.ptr(used), max(lens_q), max(lens_k), total_q,
                          len(lens_q), h, hk, DQK, DV, st, DQK ** -0.5 if scale is None else scale,
                          window[0], window[1], q.dtype == torch.float16, capi.stream_handle())
    kern = _check_kernel(L)
    if sync:
        torch.cuda.synchronize()
    return o, lse, kern


def run_dense(q, k, v, window=(-1, -1), scale=None, o=None, lse=None):
    """fmha_fwd_mla on device tensors [b, s, h, d] (views are fine).  Returns (o, lse, kernel)."""
    from xf_flash_attention_cutlass_amd import capi
    L = capi.lib()
    b, sq, h, _ = q.shape
    sk, hk = k.shape[1], k.shape[2]
    if o is None:
        o = torch.full((b, sq, h, DV), float("nan"), dtype=q.dtype, device=DEV)
    if lse is None:
        lse = torch.full((b, h, sq), float("nan"), dtype=torch.float32, device=DEV)
    st = (C.c_int64 * 12)(*q.stride()[:3], *k.stride()[:3], *v.stride()[:3], *o.stride()[:3])
    L.fmha_fwd_mla(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr(), sq, sk, b, h, hk,
                   DQK, DV, st, DQK ** -0.5 if scale is None else scale, window[0], window[1],
                   q.dtype == torch.float16, capi.stream_handle())
    kern = _check_kernel(L)
    torch.cuda.synchronize()
    return o, lse, kern


def dense_as_packed(o, lse):
    """[b, sq, h, 128], [b, h, sq] -> the packed forms judge_each takes."""
    b, sq, h, d = o.shape
    return o.reshape(b * sq, h, d), lse.permute(1, 0, 2).reshape(h, b * sq)
