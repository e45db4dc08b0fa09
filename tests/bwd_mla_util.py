"""Shared helpers of the MLA prefill backward tests (not a conftest: imported explicitly).

The gradient of the (192, 128) attention: q, k, dq, dk carry 192 features a head,
v, o, dO, dv 128.

* `CASES`: the case table the GPU test and the CPU test share.  Every case is a list of sequences
  (a dense case is `b` equal ones), generated packed: q [total_q, h, 192], k [total_k, hk, 192],
  v [total_k, hk, 128], g = dO [total_q, h, 128].
* `refs`: `bwd_util.ref_grads` per sequence (float64, the fp32-upcast oracle and its low-precision
  twin; `orc.attention_ref` takes the narrower V and scales by 192^-1/2).
* `emulate_bwd_mla`: a correct kernel's arithmetic on the CPU for one sequence - fp32 accumulation,
  O, P and dS rounded to the dtype, D from the stored O over its 128 columns - with the two-width
  defects of DEFECTS plantable.
* `check_case`: `bwd_util.check_grads` (global rule mult 3, block rule) and `assert_exact_zeros`
  per sequence.
* Runners: the C ABI on `bwd_util.Arena` operands (v and dv as strided views of [tokens, hk, 256]
  buffers, the kv-projection layout), the C ABI on any device tensors, pybind and the wrappers.
"""
from __future__ import annotations

import ctypes as C
import itertools
from collections import namedtuple

import torch

from oracle import attention_ref as orc
from tests import bwd_util as bu

DEV = bu.DEV
DQK, DV = 192, 128
KV_PITCH = 256                               # the kv-projection buffer: [tokens, hk, 128 nope-k | 128 v]
KERNELS = "fmha_bwd_mla_pre_kernel+fmha_bwd_mla_dkdv_kernel+fmha_bwd_mla_dq_kernel"
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
LENS_Q = [300, 113, 1, 31]
LENS_K = [333, 203, 147, 0]                  # an empty-key sequence, a 1-row sequence
LENS_K_REV = [113, 300, 0, 147]              # sk < sq under causal: rows that see no key

Case = namedtuple("Case", "name lens_q lens_k h hk causal window q_mul packed")


def _dense(name, sq, sk, causal=False, window=(-1, -1), h=6, hk=2, q_mul=1.0, b=2):
    return Case(name, [sq] * b, [sk] * b, h, hk, causal, window, q_mul, False)


def _packed(name, lens_k, causal):
    return Case(name, LENS_Q, lens_k, 6, 2, causal, (-1, -1), 1.0, True)


# The smallest shapes at which a 128-key-block / 32-row-tile dK/dV kernel and a 128-row-block /
# 64-key-tile dQ kernel can go wrong: 113 x 300 is 3 ragged key blocks x 4 ragged query tiles (one
# ragged row block x 5 key tiles); 300 x 113 causal leaves 187 rows without a key; 64 x 400 with the
# window (20, 0) leaves key blocks 0 and 1 unseen; 64 x 1100 runs the dQ key loop 18 tiles and the
# dK/dV grid 9 blocks.
CASES = [
    _dense("d113x300_full", 113, 300),
    _dense("d113x300_causal", 113, 300, causal=True),
    _dense("d300x113_causal", 300, 113, causal=True),
    _dense("d257x333_w37_0", 257, 333, window=(37, 0)),
    _dense("d257x333_w-1_20", 257, 333, window=(-1, 20)),
    _dense("d257x333_w100_30", 257, 333, window=(100, 30)),
    _dense("d64x400_w20_0", 64, 400, window=(20, 0)),
    _dense("d113x300_qx4", 113, 300, q_mul=4.0),
    _dense("d113x300_g1", 113, 300, causal=True, h=3, hk=3),
    _dense("d64x1100_full", 64, 1100),
    _packed("p_causal", LENS_K, True),
    _packed("p_full", LENS_K, False),
    _packed("p_rev_causal", LENS_K_REV, True),
    _packed("p_rev_full", LENS_K_REV, False),
]
CASE = {c.name: c for c in CASES}


def cu(lens):
    return torch.tensor([0] + list(itertools.accumulate(lens)), dtype=torch.int32)


def window_of(case):
    return bu.norm_window(case.causal, case.window)


_INPUTS = {}


def make(case, dtype):
    """Packed host q, k, v, g of a case (cached: the tests share them and leave them unchanged)."""
    key = (case.name, dtype)
    if key not in _INPUTS:
        gen = torch.Generator().manual_seed(1300 + CASES.index(case))
        tq, tk = sum(case.lens_q), sum(case.lens_k)
        q = (torch.randn(tq, case.h, DQK, generator=gen) * case.q_mul).to(dtype)
        k = torch.randn(tk, case.hk, DQK, generator=gen).to(dtype)
        v = torch.randn(tk, case.hk, DV, generator=gen).to(dtype)
        g = torch.randn(tq, case.h, DV, generator=gen).to(dtype)
        _INPUTS[key] = (q, k, v, g)
    return _INPUTS[key]


def split(x, lens):
    """packed [total, h, d] -> [[1, s_i, h, d]]"""
    return [x[s][None] for s in bu.seq_slices(cu(lens))]


_REFS = {}


def refs(case, dtype):
    """[bwd_util.Refs per sequence] of a case's inputs, computed once."""
    key = (case.name, dtype)
    if key not in _REFS:
        q, k, v, g = make(case, dtype)
        _REFS[key] = bu.ref_grads_varlen(q, k, v, g, cu(case.lens_q), cu(case.lens_k),
                                         window_size=window_of(case))
    return _REFS[key]


def check_case(name, got, case, dtype, report=None):
    """got: packed (dq, dk, dv).  Every sequence under check_grads (global rule mult 3 and the block
    rule) and assert_exact_zeros."""
    per = [split(x, lens) for x, lens in zip(got, (case.lens_q, case.lens_k, case.lens_k))]
    worst = bu.WorstRows()
    for i, r in enumerate(refs(case, dtype)):
        one = tuple(p[i] for p in per)
        if one[0].shape[1] and one[1].shape[1]:
            bu.check_grads(f"{name} seq{i}", one, r, dtype, worst)
        else:
            assert all(not x.float().abs().sum().item() > 0 for x in one), f"{name} seq{i}: an empty sequence's gradient != 0"
        bu.assert_exact_zeros(f"{name} seq{i}", one, case.causal, case.window)
    ratio = max((row["err"] / row["bound"] for row in worst.rows.values()), default=0.0)
    print(f"{name}: worst err / bound {ratio:.3f}")
    if report is not None:
        worst.flush(report)
    return ratio


# ------------------------------------------------------------------ the kernels' arithmetic ----
DEFECTS = ("dk_rope", "dq_rope", "dp_from_k", "d_wide_o", "scale128", "no_dv_tile3", "topleft",
           "dq_last_tile")


def emulate_fwd_mla(q, k, v, window=(-1, -1), scale=None):
    """[1, s, h, d] -> (O [1, sq, h, 128] in the dtype, LSE [1, h, sq] fp32, +inf on a row without
    a visible key): what `emulate_bwd_mla` takes D and P from when it is given none."""
    scale = DQK ** -0.5 if scale is None else scale
    h = q.shape[2]
    s = torch.einsum("bthd,bshd->bhts", q.float(), orc.expand_kv(k, h).float()) * scale
    if window[0] >= 0 or window[1] >= 0:
        s = s.masked_fill(orc.local_mask(q.shape[1], k.shape[1], window), float("-inf"))
    lse = torch.logsumexp(s, -1, keepdim=True)
    lse = torch.where(torch.isneginf(lse), torch.full_like(lse, float("inf")), lse)
    p16 = torch.exp(s - lse).to(q.dtype).float()
    o = torch.einsum("bhts,bshd->bthd", p16, orc.expand_kv(v, h).float())
    return o.to(q.dtype), lse.squeeze(-1)


def emulate_bwd_mla(q, k, v, g, window=(-1, -1), defect=None, o=None, lse=None, scale=None):
    """One sequence ([1, s, h, d]: q, k 192 wide, v, g 128 wide) as correct kernels compute it: fp32
    accumulation, P = exp(S - LSE) and dS = P (dP - D) rounded to the dtype before they feed a
    product, D = rowsum(dO * O) from the stored (rounded) O over its 128 columns, results rounded to
    the dtype.  `o` / `lse`: a forward's stored O [1, sq, h, 128] and LSE [1, h, sq] in place of the
    emulation's own.  `defect` plants one two-width bug (DEFECTS):
      dk_rope       dK's rotary columns 128..191 dropped
      dq_rope       dQ's columns 128..191 dropped
      dp_from_k     dP taken against K's first 128 columns instead of V
      d_wide_o      D summed over 192 columns: 64 more of dO and O, which a 192-wide read finds
                    in the next head's first 64
      scale128      the scale of a 128-wide head
      no_dv_tile3   dV d-tile 3 (columns 96..127) dropped
      topleft       the window aligned top-left (diag = 0) when sk != sq
      dq_last_tile  the last 64-key tile missing from dQ
    Returns (dq, dk, dv) [1, s, h(k), d] in the dtype."""
    assert defect is None or defect in DEFECTS, defect
    dt = q.dtype
    _, sq, h, _ = q.shape
    sk, hk = k.shape[1], k.shape[2]
    G = h // hk
    scale = DQK ** -0.5 if scale is None else scale
    if defect == "scale128":
        scale = DV ** -0.5
    if o is None or lse is None:
        o, lse = emulate_fwd_mla(q, k, v, window)
    qf, gf = q.float(), g.float()
    kf, vf = orc.expand_kv(k, h).float(), orc.expand_kv(v, h).float()
    s = torch.einsum("bthd,bshd->bhts", qf, kf) * scale
    if window[0] >= 0 or window[1] >= 0:
        if defect == "topleft":                       # local_mask of a square problem: diag = 0
            masked = orc.local_mask(max(sq, sk), max(sq, sk), window)[:sq, :sk]
        else:
            masked = orc.local_mask(sq, sk, window)
        s = s.masked_fill(masked, float("-inf"))
    p = torch.exp(s - lse.float().unsqueeze(-1))                       # [1, h, sq, sk]
    p = torch.where(torch.isnan(p), torch.zeros_like(p), p)            # (-inf) - (+inf rows): 0
    p16 = p.to(dt).float()
    of = o.float()
    dsum = (gf * of).sum(-1)                                           # [1, sq, h]
    if defect == "d_wide_o":
        dsum = dsum + (gf.roll(-1, 2)[..., :DQK - DV] * of.roll(-1, 2)[..., :DQK - DV]).sum(-1)
    dsum = dsum.permute(0, 2, 1).unsqueeze(-1)                         # [1, h, sq, 1]
    dp = torch.einsum("bthd,bshd->bhts", gf, kf[..., :DV] if defect == "dp_from_k" else vf)
    ds16 = (p * (dp - dsum)).to(dt).float()
    ds_dq = ds16
    if defect == "dq_last_tile":
        ds_dq = ds16.clone()
        ds_dq[..., (sk - 1) // 64 * 64:] = 0
    dq = torch.einsum("bhts,bshd->bthd", ds_dq, kf) * scale
    dk = (torch.einsum("bhts,bthd->bshd", ds16, qf) * scale).view(1, sk, hk, G, DQK).sum(3)
    dv = torch.einsum("bhts,bthd->bshd", p16, gf).view(1, sk, hk, G, DV).sum(3)
    if defect == "dk_rope":
        dk[..., DV:] = 0
    if defect == "dq_rope":
        dq[..., DV:] = 0
    if defect == "no_dv_tile3":
        dv[..., 96:] = 0
    return dq.to(dt), dk.to(dt), dv.to(dt)


def emulate_case(case, dtype, defect=None):
    """Packed (dq, dk, dv) of a case from `emulate_bwd_mla` per sequence."""
    q, k, v, g = make(case, dtype)
    parts = [split(x, lens) for x, lens in zip((q, k, v, g), (case.lens_q, case.lens_k, case.lens_k, case.lens_q))]
    outs = []
    for qs, ks, vs, gs in zip(*parts):
        if qs.shape[1] == 0 or ks.shape[1] == 0:
            outs.append((torch.zeros_like(qs), torch.zeros_like(ks), torch.zeros_like(vs)))
        else:
            outs.append(emulate_bwd_mla(qs, ks, vs, gs, window_of(case), defect))
    return tuple(torch.cat([o[i][0] for o in outs]) for i in range(3))


# ------------------------------------------------------------------ launches -------------------
def as_dense(case, x):
    """packed [b * s, h, d] -> [b, s, h, d] of a dense case (a view)"""
    return x.view(len(case.lens_q), -1, *x.shape[1:])


def forward(xfa, case, q, k, v, scale=None):
    """The forward's (out, lse) of packed device q, k, v through `paged_attn.fwd_mla` /
    `varlen_fwd_mla`: out packed [total_q, h, 128]; lse [h, total_q] (packed) or [b, h, sq]."""
    scale = DQK ** -0.5 if scale is None else scale
    wl, wr = window_of(case)
    if case.packed:
        return xfa.paged_attn.varlen_fwd_mla(q, k, v, None, cu(case.lens_q).to(DEV), cu(case.lens_k).to(DEV), None,
                                             max(case.lens_q), max(case.lens_k), scale, False, wl, wr)
    out, lse = xfa.paged_attn.fwd_mla(as_dense(case, q), as_dense(case, k), as_dense(case, v), None, scale,
                                      False, wl, wr)
    return out.view(-1, case.h, DV), lse


def capi_call(case, t, scale=None, cus=None, softmax_d=None, pair=(DQK, DV)):
    """fmha_bwd_mla / fmha_varlen_bwd_mla on device tensors t = {dout, q, k, v, out, lse, dq, dk,
    dv} (packed [total, h, d]; views are fine), by their own strides.  cus: (cu_seqlens_q,
    cu_seqlens_k) already on the device.  Returns (status, message, kernel record); no sync."""
    from xf_flash_attention_cutlass_amd import capi
    L = capi.lib()
    scale = DQK ** -0.5 if scale is None else scale
    wl, wr = window_of(case)
    order = ("q", "k", "v", "out", "dout", "dq", "dk", "dv")
    strides = lambda x: (0, 0) if x is None else x.stride()[:2]      # noqa: E731  (a NULL tensor: refused)
    ptrs = [capi.ptr(t[n]) for n in ("dout", "q", "k", "v", "out", "lse", "dq", "dk", "dv")] + [capi.ptr(softmax_d)]
    fp16 = t["q"].dtype == torch.float16
    if case.packed:
        cq, ck = cus if cus is not None else (cu(case.lens_q).to(DEV), cu(case.lens_k).to(DEV))
        st = (C.c_int64 * 16)(*itertools.chain.from_iterable(strides(t[n]) for n in order))
        L.fmha_varlen_bwd_mla(*ptrs, cq.data_ptr(), ck.data_ptr(), max(case.lens_q), max(case.lens_k),
                              sum(case.lens_q), sum(case.lens_k), len(case.lens_q), case.h, case.hk, *pair, st,
                              scale, wl, wr, fp16, capi.stream_handle())
    else:
        b, sq, sk = len(case.lens_q), case.lens_q[0], case.lens_k[0]
        st = (C.c_int64 * 24)(*itertools.chain.from_iterable(
            (strides(t[n])[0] * (sq if n in ("q", "out", "dout", "dq") else sk), *strides(t[n])) for n in order))
        L.fmha_bwd_mla(*ptrs, sq, sk, b, case.h, case.hk, *pair, st, scale, wl, wr, fp16, capi.stream_handle())
    return L.fmha_last_status(), L.fmha_last_error().decode(), L.fmha_last_kernel().decode()


def run_capi_arena(xfa, case, dtype, fill=0xFF, scale=None):
    """The C entry of a case on `bwd_util.Arena` operands (4 KiB guards, every byte `fill`): q, k,
    out, dout, lse, dq, dk (and the cu_seqlens) contiguous, v and dv the first 128 columns of
    [total_k, hk, 256] buffers.  Checks the status, the kernel record, the guards, that every dq /
    dk / dv element was written (fill 0xFF: an unwritten element is a NaN) and that columns
    128..255 beside v and dv still hold the fill.  Returns host packed (dq, dk, dv)."""
    q, k, v, g = make(case, dtype)
    tq, tk, h, hk, nb = q.shape[0], k.shape[0], case.h, case.hk, len(case.lens_q)
    qd, kd, vd = (x.to(DEV) for x in (q, k, v))
    out, lse = forward(xfa, case, qd, kd, vd, scale)
    ar = bu.Arena({"q": (q.shape, dtype), "k": (k.shape, dtype), "vbuf": ((tk, hk, KV_PITCH), dtype),
                   "out": (g.shape, dtype), "dout": (g.shape, dtype), "lse": (lse.shape, torch.float32),
                   "dq": (q.shape, dtype), "dk": (k.shape, dtype), "dvbuf": ((tk, hk, KV_PITCH), dtype),
                   "cu_q": ((nb + 1,), torch.int32), "cu_k": ((nb + 1,), torch.int32)}, fill)
    t = {n: ar[n] for n in ("q", "k", "out", "dout", "lse", "dq", "dk")}
    t["v"], t["dv"] = ar["vbuf"][..., :DV], ar["dvbuf"][..., :DV]
    for nm, src in (("q", qd), ("k", kd), ("v", vd), ("out", out), ("dout", g.to(DEV)), ("lse", lse)):
        t[nm].copy_(src)
    ar["cu_q"].copy_(cu(case.lens_q))
    ar["cu_k"].copy_(cu(case.lens_k))
    status, msg, kern = capi_call(case, t, scale, cus=(ar["cu_q"], ar["cu_k"]))
    torch.cuda.synchronize()
    what = f"{case.name} {dtype} fill={fill:#x}"
    assert status == 0, (what, msg)
    assert kern.startswith(KERNELS + " "), (what, kern)
    ar.assert_guards(what)
    res = []
    for nm in bu.NAMES:
        assert torch.isfinite(t[nm].float()).all(), f"{what}: {nm} has elements the kernels never wrote"
        res.append(t[nm].cpu().clone())
    for nm in ("vbuf", "dvbuf"):
        beside = ar[nm][..., DV:].contiguous().view(torch.uint8)
        assert bool((beside == fill).all()), f"{what}: columns 128..255 of {nm} changed"
    return tuple(res)


def run_pybind(xfa, case, dtype, scale=None):
    """`paged_attn.bwd_mla` / `varlen_bwd_mla` with the op's own outputs.  Host packed (dq, dk, dv)."""
    q, k, v, g = (x.to(DEV) for x in make(case, dtype))
    scale = DQK ** -0.5 if scale is None else scale
    out, lse = forward(xfa, case, q, k, v, scale)
    wl, wr = window_of(case)
    if case.packed:
        res = xfa.paged_attn.varlen_bwd_mla(g, q, k, v, out, lse, None, None, None, cu(case.lens_q).to(DEV),
                                            cu(case.lens_k).to(DEV), max(case.lens_q), max(case.lens_k), scale,
                                            False, wl, wr)
    else:
        res = xfa.paged_attn.bwd_mla(*(as_dense(case, x) for x in (g, q, k, v, out)), lse, None, None, None,
                                     scale, False, wl, wr)
    return tuple(x.reshape(-1, *x.shape[-2:]).cpu() for x in res[:3])


def run_wrapper(xfa, case, dtype, scale=None):
    """`flash_attn_mla_func` / `flash_attn_mla_varlen_func` and `torch.autograd.grad`.  Returns host
    packed (out, dq, dk, dv)."""
    q, k, v, g = (x.to(DEV) for x in make(case, dtype))
    q, k, v = (x.requires_grad_(True) for x in (q, k, v))
    kw = dict(causal=case.causal, window_size=case.window, softmax_scale=scale)
    if case.packed:
        out = xfa.flash_attn_mla_varlen_func(q, k, v, cu(case.lens_q).to(DEV), cu(case.lens_k).to(DEV),
                                             max(case.lens_q), max(case.lens_k), **kw)
        grads = torch.autograd.grad(out, (q, k, v), g)
    else:
        qd, kd, vd = (as_dense(case, x) for x in (q, k, v))
        out = xfa.flash_attn_mla_func(qd, kd, vd, **kw)
        grads = torch.autograd.grad(out, (q, k, v), as_dense(case, g))
    return (out.detach().reshape(-1, case.h, DV).cpu(),) + tuple(x.cpu() for x in grads)
