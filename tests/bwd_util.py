"""Shared helpers of the backward tests (not a conftest: imported explicitly).

* `ref_grads` / `ref_grads_varlen`: float64 oracle gradients plus the project's two existing
  references (fp32-upcast oracle and its low-precision twin).
* `check_grads`: the global gradient rule of tests/test_bwd_gpu.py and a per-block rms rule.
* `assert_exact_zeros`: rows without a visible key / keys no row sees are exactly 0.
* `Arena`: every operand of a C-ABI call as an interior slice of one poisoned byte arena.
* `capi_bwd`, `capi_varlen_bwd`: fmha_bwd / fmha_varlen_bwd on arena operands with a workspace that
  holds a chosen number of dQ slices.
* `emulate_bwd` / `emulate_fwd`: a CPU model of a correct kernel (fp32 accumulation, P and dS
  rounded to the input dtype) with plantable defects, for tests/test_bwd_util.py; given a forward's
  stored O and LSE it is the second estimate of tests/bwd_stress_util.py.
* `instance_table`: the (bucket, dtype, mask, feat, deterministic) cases of
  tests/test_bwd_instances_gpu.py.
"""
from __future__ import annotations

import itertools
from collections import namedtuple

import torch

from oracle import attention_ref as orc

DEV = "cuda"
BLOCK = 32                                        # rows / keys per block of the block rule
EPS = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
NAMES = ("dq", "dk", "dv")

Refs = namedtuple("Refs", "ref64 ref pt")         # each a (dq, dk, dv) tuple


# ---------------------------------------------------------------- references -------------
def _grads(q, k, v, g, upcast, reorder, **kw):
    qq, kk, vv = (x.clone().requires_grad_(True) for x in (q, k, v))
    out, _ = orc.attention_ref(qq, kk, vv, upcast=upcast, reorder_ops=reorder, **kw)
    return torch.autograd.grad(out, (qq, kk, vv), g.to(out.dtype))


def ref_grads(q, k, v, g, **kw) -> Refs:
    """Gradients of `orc.attention_ref` for [b, s, h, d] inputs: in float64 (`.double()` inputs,
    upcast=False), and the two references of the project's global rule (fp32-upcast oracle and
    its low-precision twin, both in the input dtype)."""
    kw64 = dict(kw)
    if kw64.get("attn_bias") is not None:
        kw64["attn_bias"] = kw64["attn_bias"].double()
    ref64 = _grads(q.double(), k.double(), v.double(), g.double(), False, False, **kw64)
    return Refs(ref64, _grads(q, k, v, g, True, False, **kw), _grads(q, k, v, g, False, True, **kw))


def _zeros_refs(q, k):
    z = (torch.zeros_like(q), torch.zeros_like(k), torch.zeros_like(k))
    return Refs(tuple(x.double() for x in z), z, z)


def seq_slices(cu):
    cu = [int(x) for x in cu]
    return [slice(cu[i], cu[i + 1]) for i in range(len(cu) - 1)]


def ref_grads_varlen(q, k, v, g, cu_q, cu_k, slopes=None, **kw):
    """`ref_grads` per sequence of packed [total, h, d] inputs: a list of Refs over [1, s_i, h, d]
    tensors.  `slopes` [b, h]: ALiBi as `orc.alibi_bias` of each sequence's own (sq_i, sk_i).
    An empty sequence (no queries or no keys) has all-zero gradients."""
    res = []
    for i, (sq_, sk_) in enumerate(zip(seq_slices(cu_q), seq_slices(cu_k))):
        qs, gs, ks, vs = q[sq_][None], g[sq_][None], k[sk_][None], v[sk_][None]
        if qs.shape[1] == 0 or ks.shape[1] == 0:
            res.append(_zeros_refs(qs, ks))
            continue
        kws = dict(kw)
        if slopes is not None:
            kws["attn_bias"] = orc.alibi_bias(slopes[i:i + 1], qs.shape[1], ks.shape[1], causal=False)
        res.append(ref_grads(qs, ks, vs, gs, **kws))
    return res


# ---------------------------------------------------------------- pass rules -------------
def _block_ms(x):
    """[b, s, h, d] float64 -> mean square over (rows of the block, d): [b, nblocks, h]; the
    ragged last block is averaged over its actual rows."""
    b, s, h, d = x.shape
    nb = -(-s // BLOCK)
    e = (x * x).sum(-1)                                             # [b, s, h]
    e = torch.nn.functional.pad(e, (0, 0, 0, nb * BLOCK - s)).view(b, nb, BLOCK, h).sum(2)
    rows = torch.full((nb,), float(BLOCK), dtype=torch.float64)
    rows[-1] = s - (nb - 1) * BLOCK
    return e / (rows.view(1, nb, 1) * d)


def block_rule(got, ref64, pt, dtype):
    """Worst block of rms(got - ref64) / (3 rms(pt - ref64) + eps/2 rms(ref64) + 1e-5) over the
    (batch, head, 32-row block)s of a [b, s, h, d] gradient: (ratio, err, bound, (b, block, h))."""
    got, pt = got.double().cpu(), pt.double().cpu()
    err = _block_ms(got - ref64).sqrt()
    bound = 3.0 * _block_ms(pt - ref64).sqrt() + 0.5 * EPS[dtype] * _block_ms(ref64).sqrt() + 1e-5
    ratio = err / bound
    i = int(ratio.argmax())
    where = tuple(int(x) for x in torch.unravel_index(torch.tensor(i), ratio.shape))
    return ratio.flatten()[i].item(), err.flatten()[i].item(), bound.flatten()[i].item(), where


def check_grads(name, got, refs: Refs, dtype, report=None, mult=3.0, block_factor=None):
    """Asserts, for each of dq / dk / dv ([b, s, h, d]):
    the global rule max|got - ref| <= mult * max|pt - ref| + 1e-5 (tests/test_bwd_gpu.py), and
    the block rule per (batch, head, 32-row block).  `report` gets one row per rule.
    `block_factor` {"dq": f}: a case class whose block bound is widened by a measured, explained
    factor (stated by the test that passes it and recorded in the report row)."""
    failures = []
    for nm, x, r64, r, p in zip(NAMES, got, refs.ref64, refs.ref, refs.pt):
        if x.numel() == 0:
            continue
        x = x.cpu()
        assert x.shape == r.shape, f"{name} {nm}: shape {tuple(x.shape)} != {tuple(r.shape)}"
        if not torch.isfinite(x.float()).all():
            failures.append(f"{name} {nm}: non-finite values")
            continue
        ok, err, bound = orc.parity_ok(x, r, p, mult, 1e-5)
        if report:
            report({"case": name, "metric": f"{nm} global", "err": err, "bound": bound})
        if not ok:
            failures.append(f"{name} {nm}: global max|d-ref|={err:.3g} > {bound:.3g}")
        ratio, berr, bbound, where = block_rule(x, r64, p, dtype)
        factor = (block_factor or {}).get(nm, 1.0)
        if report:
            report({"case": name, "metric": f"{nm} block", "err": berr, "bound": bbound,
                    "block": list(where), "bound_factor": factor})
        if not ratio <= factor:
            failures.append(f"{name} {nm}: block (b, blk, h)={where} rms err {berr:.3g} > "
                            f"{bbound:.3g} (ratio {ratio:.2f})")
    assert not failures, "; ".join(failures)


class WorstRows:
    """A `report` that keeps, per metric, the row with the largest err / bound of the sub-cases
    of one test (sequences, sweep points); `flush` passes those on to the session's report."""

    def __init__(self):
        self.rows = {}

    def __call__(self, row):
        old = self.rows.get(row["metric"])
        if old is None or row["err"] / row["bound"] > old["err"] / old["bound"]:
            self.rows[row["metric"]] = row

    def flush(self, report):
        for row in self.rows.values():
            report(row)


def norm_window(causal=False, window=(-1, -1)):
    return (int(window[0]), 0) if causal else (int(window[0]), int(window[1]))


def visibility(sq, sk, causal=False, window=(-1, -1)):
    """(row_sees_a_key [sq], key_seen_by_a_row [sk]) from `orc.local_mask`; windows must be
    non-negative or -1 (off)."""
    w = norm_window(causal, window)
    if sq == 0 or sk == 0:
        return torch.zeros(sq, dtype=torch.bool), torch.zeros(sk, dtype=torch.bool)
    if w[0] < 0 and w[1] < 0:
        return torch.ones(sq, dtype=torch.bool), torch.ones(sk, dtype=torch.bool)
    vis = ~orc.local_mask(sq, sk, w)
    return vis.any(1), vis.any(0)


def assert_exact_zeros(name, got, causal=False, window=(-1, -1)):
    """No tolerance: dQ rows without a visible key and dK / dV rows of keys no row sees are
    exactly 0 ([b, s, h, d] gradients of one dense problem or one sequence)."""
    dq, dk, dv = (x.cpu() for x in got)
    rows, keys = visibility(dq.shape[1], dk.shape[1], causal, window)
    assert not dq[:, ~rows].float().abs().sum().item() > 0, f"{name}: dq != 0 on a row without keys"
    assert not dk[:, ~keys].float().abs().sum().item() > 0, f"{name}: dk != 0 on an unseen key"
    assert not dv[:, ~keys].float().abs().sum().item() > 0, f"{name}: dv != 0 on an unseen key"
    for nm, x, m in (("dq", dq, rows), ("dk", dk, keys), ("dv", dv, keys)):
        assert torch.isfinite(x[:, ~m].float()).all(), f"{name}: {nm} not finite on a masked row"


# ---------------------------------------------------------------- arena ------------------
class Arena:
    """One uint8 device buffer filled with `fill`; every operand is an interior, 256-byte-aligned
    slice with at least `guard` untouched bytes on each side.  `assert_guards` checks that every
    byte outside the operands still holds `fill`."""

    def __init__(self, specs, fill=0xFF, guard=4096, device=DEV):
        self.fill, self.guard = fill, guard
        self.spans, cur = {}, 0
        for name, (shape, dtype) in specs.items():
            n = torch.empty(0, dtype=dtype).element_size()
            for s in shape:
                n *= s
            start = -(-(cur + guard) // 256) * 256
            self.spans[name] = (start, n, tuple(shape), dtype)
            cur = start + n
        total = cur + guard
        self.buf = torch.full((total + 256,), fill, dtype=torch.uint8, device=device)
        self.base = (-self.buf.data_ptr()) % 256            # align the arena's own origin
        self.total = total

    def __getitem__(self, name):
        start, n, shape, dtype = self.spans[name]
        return self.buf[self.base + start:self.base + start + n].view(dtype).view(shape)

    def ptr(self, name):
        p = self.buf.data_ptr() + self.base + self.spans[name][0]
        assert p % 256 == 0
        return p

    def nbytes(self, name):
        return self.spans[name][1]

    def assert_guards(self, what=""):
        owned = torch.zeros(self.buf.numel(), dtype=torch.bool, device=self.buf.device)
        for start, n, _, _ in self.spans.values():
            assert start - self.guard >= 0
            owned[self.base + start:self.base + start + n] = True
        bad = (~owned) & (self.buf != self.fill)
        if bad.any():
            at = int(bad.nonzero()[0]) - self.base
            near = min(self.spans, key=lambda k: min(abs(at - self.spans[k][0]),
                                                     abs(at - self.spans[k][0] - self.spans[k][1])))
            raise AssertionError(f"{what}: {int(bad.sum())} guard bytes overwritten, first at arena "
                                 f"offset {at} (next to '{near}' at {self.spans[near][0]}, "
                                 f"{self.spans[near][1]} bytes)")


def _ws_bytes(size_fn, dims, tokens, h, deterministic, n_slices):
    """Workspace bytes for `n_slices` dQ slices (None: what the library asks for).  Layout
    (fmha_api.cpp, bwd_ws_bytes): [dQ slices][D = rowsum(dO O)][lse_fix], the two tails each
    tokens * h floats rounded up to 256 bytes."""
    one, full = size_fn(*dims, False), size_fn(*dims, True)
    tail = -(-(tokens * h * 4) // 256) * 256
    acc = one - 2 * tail
    assert acc > 0 and (full - one) % acc == 0
    n_dev = 1 + (full - one) // acc
    if not deterministic:
        return one, 1
    if n_slices is None:
        return full, n_dev
    assert n_dev >= n_slices, f"the device picks {n_dev} slices, the case wants {n_slices}"
    return one + (n_slices - 1) * acc, n_slices


def _finish(ar, what):
    torch.cuda.synchronize()
    ar.assert_guards(what)
    res = []
    for nm in NAMES:
        x = ar[nm]
        assert torch.isfinite(x.float()).all(), f"{what}: {nm} has elements the kernels never wrote"
        res.append(x.cpu().clone())
    return res


def capi_bwd(xfa, q, k, v, g, *, causal=False, window=(-1, -1), deterministic=False,
             n_slices=None, ws_fill=0xFF, fill=0xFF):
    """fmha_bwd through the C ABI on arena operands; q/g [b, sq, h, d], k/v [b, sk, hk, d] (host).
    The forward (O, LSE) comes from the extension.  Returns host (dq, dk, dv) after checking the
    guard bytes and that every output element was written."""
    from xf_flash_attention_cutlass_amd import capi
    L = capi.lib()
    b, sq, h, d = q.shape
    sk, hk = k.shape[1], k.shape[2]
    assert d % 8 == 0
    wl, wr = norm_window(causal, window)
    scale = d ** -0.5
    qd, kd, vd = (x.to(DEV) for x in (q, k, v))
    fw = xfa.paged_attn.fwd(qd, kd, vd, None, None, 0.0, scale, causal, wl, wr, 0.0, False, None)
    out, lse = fw[4], fw[5]
    nbytes, n = _ws_bytes(L.fmha_bwd_workspace_size, (sq, sk, b, h, hk, d), b * sq, h,
                          deterministic, n_slices)
    dt = q.dtype
    ar = Arena({"q": (q.shape, dt), "k": (k.shape, dt), "v": (v.shape, dt), "out": (q.shape, dt),
                "dout": (q.shape, dt), "lse": ((b, h, sq), torch.float32), "dq": (q.shape, dt),
                "dk": (k.shape, dt), "dv": (k.shape, dt), "ws": ((nbytes,), torch.uint8)}, fill)
    for nm, src in (("q", qd), ("k", kd), ("v", vd), ("out", out), ("dout", g.to(DEV)), ("lse", lse)):
        ar[nm].copy_(src)
    ar["ws"].fill_(ws_fill)
    L.fmha_bwd(ar.ptr("dout"), ar.ptr("q"), ar.ptr("k"), ar.ptr("v"), ar.ptr("out"), ar.ptr("lse"),
               ar.ptr("dq"), ar.ptr("dk"), ar.ptr("dv"), None, None, sq, sk, b, h, hk, d, 0.0, scale,
               wl, wr, 0.0, deterministic, dt == torch.float16, capi.stream_handle(),
               ar.ptr("ws"), nbytes)
    capi.check()
    return _finish(ar, f"fmha_bwd det={deterministic} slices={n} ws_fill={ws_fill:#x}")


def capi_varlen_bwd(xfa, q, k, v, g, lq, lk, *, causal=False, window=(-1, -1),
                    deterministic=False, n_slices=None, ws_fill=0xFF, fill=0xFF):
    """fmha_varlen_bwd on arena operands (cu_seqlens included); packed q/g [total_q, h, d],
    k/v [total_k, hk, d] (host), sequence lengths lq / lk (zeros allowed)."""
    from xf_flash_attention_cutlass_amd import capi
    L = capi.lib()
    tq, h, d = q.shape
    tk, hk = k.shape[0], k.shape[1]
    nb = len(lq)
    assert d % 8 == 0 and sum(lq) == tq and sum(lk) == tk
    wl, wr = norm_window(causal, window)
    scale = d ** -0.5
    cu_q = torch.tensor([0] + list(itertools.accumulate(lq)), dtype=torch.int32)
    cu_k = torch.tensor([0] + list(itertools.accumulate(lk)), dtype=torch.int32)
    qd, kd, vd = (x.to(DEV) for x in (q, k, v))
    fw = xfa.paged_attn.varlen_fwd(qd, kd, vd, None, cu_q.to(DEV), cu_k.to(DEV), None, None, None,
                                   max(lq), max(lk), 0.0, scale, False, causal, wl, wr, 0.0, False,
                                   None)
    out, lse = fw[4], fw[5]
    nbytes, n = _ws_bytes(L.fmha_varlen_bwd_workspace_size, (tq, max(lk), nb, h, hk, d), tq, h,
                          deterministic, n_slices)
    dt = q.dtype
    ar = Arena({"q": (q.shape, dt), "k": (k.shape, dt), "v": (v.shape, dt), "out": (q.shape, dt),
                "dout": (q.shape, dt), "lse": ((h, tq), torch.float32), "dq": (q.shape, dt),
                "dk": (k.shape, dt), "dv": (k.shape, dt), "cu_q": ((nb + 1,), torch.int32),
                "cu_k": ((nb + 1,), torch.int32), "ws": ((nbytes,), torch.uint8)}, fill)
    for nm, src in (("q", qd), ("k", kd), ("v", vd), ("out", out), ("dout", g.to(DEV)), ("lse", lse),
                    ("cu_q", cu_q.to(DEV)), ("cu_k", cu_k.to(DEV))):
        ar[nm].copy_(src)
    ar["ws"].fill_(ws_fill)
    L.fmha_varlen_bwd(ar.ptr("dout"), ar.ptr("q"), ar.ptr("k"), ar.ptr("v"), ar.ptr("out"),
                      ar.ptr("lse"), ar.ptr("dq"), ar.ptr("dk"), ar.ptr("dv"), ar.ptr("cu_q"),
                      ar.ptr("cu_k"), None, 0, max(lq), max(lk), tq, tk, nb, h, hk, d, scale, wl, wr,
                      0.0, deterministic, dt == torch.float16, capi.stream_handle(), ar.ptr("ws"),
                      nbytes, None, 0.0)
    capi.check()
    return _finish(ar, f"fmha_varlen_bwd det={deterministic} slices={n} ws_fill={ws_fill:#x}")


# ---------------------------------------------------------------- CPU emulation ----------
DEFECT_ROWS = slice(32, 64)                       # the query rows the D / mask defects touch
DEFECTS = ("dk_block", "dq_tail", "dq_twice", "dv_lastkey",
           "d_neighbour", "d_zero", "unmasked_block", "lse_as_d")


def _emulate_scores(q, k, causal, window, softcap, attn_bias, sink):
    """fp32 scores of the emulation: (s masked, s before the mask, d softcap / d s, lse
    [b, h, sq, 1] with +inf on rows without a visible key).  sink [h]: joins the LSE only."""
    b, sq, h, d = q.shape
    sk = k.shape[1]
    scale = d ** -0.5
    qf, kf = q.float(), orc.expand_kv(k, h).float()
    s = torch.einsum("bthd,bshd->bhts", qf, kf) * scale
    dcap = 1.0
    if softcap > 0:
        t = torch.tanh(s / softcap)
        s, dcap = t * softcap, 1.0 - t * t
    if attn_bias is not None:
        s = s + attn_bias
    w = norm_window(causal, window)
    masked = torch.zeros(sq, sk, dtype=torch.bool)
    if w[0] >= 0 or w[1] >= 0:
        masked = orc.local_mask(sq, sk, w)
    raw = s
    s = s.masked_fill(masked, float("-inf"))
    lse = torch.logsumexp(s, -1, keepdim=True)
    if sink is not None:
        dead = torch.isneginf(lse)
        lse = torch.logaddexp(lse, sink.float().view(1, h, 1, 1).expand_as(lse))
        lse = torch.where(dead, torch.full_like(lse, float("-inf")), lse)
    lse = torch.where(torch.isneginf(lse), torch.full_like(lse, float("inf")), lse)
    return s, raw, dcap, lse


def emulate_fwd(q, k, v, causal=False, window=(-1, -1), softcap=0.0, attn_bias=None, sink=None):
    """The (O in the input dtype, LSE [b, h, sq] fp32) that `emulate_bwd` takes D and P from when
    it is given none."""
    s, _, _, lse = _emulate_scores(q, k, causal, window, softcap, attn_bias, sink)
    p16 = torch.exp(s - lse).to(q.dtype).float()
    o = torch.einsum("bhts,bshd->bthd", p16, orc.expand_kv(v, q.shape[2]).float())
    return o.to(q.dtype), lse.squeeze(-1)


def emulate_bwd(q, k, v, g, causal=False, window=(-1, -1), defect=None, softcap=0.0,
                attn_bias=None, exact_d=False, o=None, lse=None, sink=None):
    """A correct kernel's arithmetic on the CPU: fp32 accumulation, O / P / dS rounded to the
    input dtype before they feed a product, results rounded to the dtype.  `defect` plants one
    bug (DEFECTS): the tiling ones 'dk_block', 'dq_tail', 'dq_twice', 'dv_lastkey'
    (tests/test_bwd_util.py), and on query rows 32..63 'd_neighbour' (D of row r - 1), 'd_zero'
    (D ignored), 'lse_as_d' (the row's LSE in D's place) and, causal only, 'unmasked_block' (the
    32 x 32 block at keys sk - sq + 64 .. + 95 visible in P against the masked LSE)
    (tests/test_bwd_stress_util.py).
    D = rowsum(dO * O) uses the forward's O as stored, i.e. rounded to the dtype, as every
    flash-attention backward does; `exact_d` takes the unrounded O instead (to size that term).
    `o` [b, sq, h, d] / `lse` [b, h, sq]: a forward's stored O and LSE in place of the
    emulation's own, in D and in P = exp(S - LSE) (`emulate_fwd` gives the defaults).  `sink`
    [h]: a per-head sink logit in the LSE."""
    dt = q.dtype
    b, sq, h, d = q.shape
    sk, hk = k.shape[1], k.shape[2]
    G = h // hk
    scale = d ** -0.5
    qf, gf = q.float(), g.float()
    kf, vf = orc.expand_kv(k, h).float(), orc.expand_kv(v, h).float()
    s, raw, dcap, own_lse = _emulate_scores(q, k, causal, window, softcap, attn_bias, sink)
    lse = own_lse if lse is None else lse.float().unsqueeze(-1)
    p = torch.exp(s - lse)                                           # [b, h, sq, sk]
    R = DEFECT_ROWS
    if defect == "unmasked_block":
        assert causal, "unmasked_block needs a causal mask"
        c0 = sk - sq + 64
        p = p.clone()
        p[:, :, R, c0:c0 + 32] = torch.exp(raw[:, :, R, c0:c0 + 32] - lse[:, :, R])
    p16 = p.to(dt).float()
    if o is None:
        o = torch.einsum("bhts,bshd->bthd", p16, vf)
        if not exact_d:
            o = o.to(dt).float()
    else:
        o = o.float()
    dsum = (gf * o).sum(-1).permute(0, 2, 1).unsqueeze(-1)           # [b, h, sq, 1]
    if defect in ("d_neighbour", "d_zero", "lse_as_d"):
        dsum = dsum.clone()
        n = dsum[:, :, R].shape[2]                # (fewer than 32 where the rows end inside)
        dsum[:, :, R] = {"d_neighbour": dsum[:, :, R.start - 1:R.start - 1 + n].clone(),
                         "d_zero": torch.zeros_like(dsum[:, :, R]), "lse_as_d": lse[:, :, R]}[defect]
    dp = torch.einsum("bthd,bshd->bhts", gf, vf)
    ds16 = (p * (dp - dsum) * dcap).to(dt).float()
    bn = 128 if d > 128 else 256
    p_dv, ds_dk, ds_dq = p16, ds16, ds16
    if defect == "dk_block":                      # one 32 x 32 dS block missing from dK
        ds_dk = ds16.clone()
        ds_dk[0, 0, 32:64, 64:96] = 0
    elif defect == "dq_tail":                     # tail key block missing from the tail query tile
        ds_dq = ds16.clone()
        ds_dq[:, :, (sq - 1) // BLOCK * BLOCK:, (sk - 1) // bn * bn:] = 0
    elif defect == "dv_lastkey":                  # the last key's P column missing from dV
        p_dv = p16.clone()
        p_dv[..., sk - 1] = 0
    elif defect is not None and defect not in DEFECTS:
        raise ValueError(defect)
    dq = torch.einsum("bhts,bshd->bthd", ds_dq, kf)
    if defect == "dq_twice":                      # one key block added twice into one dQ tile
        dq[:, 32:64, 0] += torch.einsum("bts,bsd->btd", ds16[:, 0, 32:64, bn:2 * bn], kf[:, bn:2 * bn, 0])
    dq = dq * scale
    dk = torch.einsum("bhts,bthd->bshd", ds_dk, qf) * scale
    dv = torch.einsum("bhts,bthd->bshd", p_dv, gf)
    dk = dk.view(b, sk, hk, G, d).sum(3)
    dv = dv.view(b, sk, hk, G, d).sum(3)
    return dq.to(dt), dk.to(dt), dv.to(dt)


# ---------------------------------------------------------------- the instance table -----
Instance = namedtuple("Instance", "d dtype mask feat det causal window")


def instance_table():
    """Every (head-dim bucket, dtype, MASK, FEAT, deterministic) instance that
    csrc/fmha_bwd.hip dispatches: 3 x 2 x 2 x 2 x 2 = 48.  MASK = on alternates causal and the
    window (100, 30) across the table."""
    rows = []
    for d, dtype, mask, feat, det in itertools.product(
            (64, 128, 256), (torch.bfloat16, torch.float16), (False, True), (False, True),
            (False, True)):
        # each (feat, det) pair meets causal at one dtype and the window at the other
        causal = mask and (d // 64 + (dtype == torch.float16) + feat + det) % 2 == 0
        window = (100, 30) if mask and not causal else (-1, -1)
        rows.append(Instance(d, dtype, mask, feat, det, causal, window))
    return rows


def bucket(d):
    return 64 if d <= 64 else 128 if d <= 128 else 256
