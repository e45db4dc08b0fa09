"""Torch-side restatements for the fp8 end-to-end tests (test-only, CPU tensors): the quantiser
fmha_quantize_fp8 is specified by, per-head input scaling, and the (batch, head) slices the
parity rule is applied to."""
from __future__ import annotations

import torch

E4M3_MAX = 448.0


def quantize_ref(x, granularity="tensor", group=1, cu_seqlens=None):
    """(x8, descale) as include/paged_attn.h states them for fmha_quantize_fp8:
    amax = max |float(x)| over the scale's set, descale = amax / 448 in fp32 (1.0 where amax == 0
    or the set is empty), byte = e4m3fn(clamp(float(x) * (1 / descale), -448, 448)).

    x [b, s, h, d], or with cu_seqlens (a list of b + 1 offsets) packed [total, h, d];
    "tensor": descale [1]; "head": descale [b, h // group]."""
    xf = x.float()
    h = x.shape[-2]
    if granularity == "tensor":
        amax = xf.abs().max().reshape(1) if xf.numel() else torch.zeros(1)
        ds = torch.where(amax == 0, torch.ones_like(amax), amax / E4M3_MAX)
        x8 = (xf * (1 / ds)).clamp(-E4M3_MAX, E4M3_MAX).to(torch.float8_e4m3fn)
        return x8, ds
    ng = h // group
    if cu_seqlens is None:
        b = x.shape[0]
        g = xf.reshape(b, x.shape[1], ng, group * x.shape[-1])
        amax = g.abs().amax(dim=(1, 3)) if x.shape[1] else torch.zeros(b, ng)
        ds = torch.where(amax == 0, torch.ones_like(amax), amax / E4M3_MAX)              # [b, ng]
        inv = (1 / ds).repeat_interleave(group, dim=1)[:, None, :, None]
        return (xf * inv).clamp(-E4M3_MAX, E4M3_MAX).to(torch.float8_e4m3fn), ds
    b = len(cu_seqlens) - 1
    ds = torch.ones(b, ng)
    x8 = torch.empty(x.shape, dtype=torch.float8_e4m3fn)
    for i in range(b):
        lo, hi = int(cu_seqlens[i]), int(cu_seqlens[i + 1])
        if hi > lo:
            x8[lo:hi], d = (t[0] for t in quantize_ref(x[None, lo:hi], "head", group))
            ds[i] = d
    return x8, ds


def scale_groups(x, hk, factors=(1.0, 1.0 / 16, 8.0), shift=0):
    """x [b, s, h, d] with its (batch, kv head) groups (h // hk consecutive heads each) multiplied
    by the factors in turn: group (b, g) takes factors[(b * hk + g + shift) % len(factors)]."""
    b, s, h, d = x.shape
    idx = (torch.arange(b * hk) + shift) % len(factors)
    f = torch.tensor(factors)[idx].view(b, 1, hk, 1).repeat_interleave(h // hk, dim=2)
    return x * f


def per_head(descale, h):
    """[b, hk] descales -> [b, 1, h, 1], each kv head's value for its h // hk query heads (the
    shape that broadcasts against [b, s, h, d])."""
    b, hk = descale.shape
    return descale.repeat_interleave(h // hk, dim=1).view(b, 1, h, 1)


def slice_parity(out, ref, pt, mult=3.0, atol=1e-3):
    """The parity rule max|out - ref| <= mult * max|pt - ref| + atol on every (batch, head) slice
    of [b, s, h, d] tensors on its own (a wrong scale on a small head does not hide under a large
    head's error).  Returns the failing slices as (b, h, err, bound)."""
    bad = []
    for bi in range(out.shape[0]):
        for hi in range(out.shape[2]):
            err = (out[bi, :, hi].float() - ref[bi, :, hi].float()).abs().max().item()
            bound = mult * (pt[bi, :, hi].float() - ref[bi, :, hi].float()).abs().max().item() + atol
            if not err <= bound:
                bad.append((bi, hi, err, bound))
    return bad
