"""Python wrappers over the `paged_attn` module, mirroring the reference's test.py:41-245.

Signatures and argument mapping follow the reference wrappers (softmax_scale default
D^-0.5, `maybe_contiguous`, int `cache_seqlens` broadcast to an int32 tensor), extended with
autograd: the backward runs the gfx950 bwd kernels through `paged_attn.bwd` /
`paged_attn.varlen_bwd` (the reference's `bwd` binding is commented out, export.cpp:1761).
"""
from __future__ import annotations

from typing import Optional, Union

import torch

from . import paged_attn


def _maybe_contiguous(x):
    return x.contiguous() if x is not None and x.stride(-1) != 1 else x


def _sink_f32(sink, q):
    """The sink as the ops take it: fp32 [h], contiguous, on q's device."""
    if sink.dim() != 1 or sink.shape[0] != q.shape[-2]:
        raise ValueError(f"sink must have shape (num_heads,) = ({q.shape[-2]},), got {tuple(sink.shape)}")
    if not sink.is_floating_point():
        raise TypeError("sink must be a floating-point tensor")
    return sink.detach().to(device=q.device, dtype=torch.float32).contiguous()


def _check_sink_args(q, dropout_p, alibi_slopes):
    if q.dtype == torch.float8_e4m3fn:
        raise NotImplementedError("fp8 q/k/v: an attention sink is not supported")
    if alibi_slopes is not None:
        raise NotImplementedError("an attention sink does not support ALiBi")
    if dropout_p != 0.0:
        raise NotImplementedError("an attention sink does not support dropout")


def _sink_grad(ctx, lse, softmax_d, s32, varlen):
    """dsink in the sink's dtype when the sink wants a gradient (`sink_bwd`), else None"""
    if s32 is None or not ctx.needs_input_grad[3]:
        return None
    return paged_attn.sink_bwd(lse, softmax_d, s32, varlen).to(ctx.sink_dtype)


class _FlashAttnFunc(torch.autograd.Function):
    """sink: a per-head logit tensor or None.  With one, `fwd_sink`, the unchanged `bwd` (given the
    sink forward's out and lse it is already the sink softmax's backward) and `sink_bwd` for dsink."""

    @staticmethod
    def forward(ctx, q, k, v, sink, dropout_p, softmax_scale, causal, window_size, softcap,
                alibi_slopes, deterministic, return_softmax):
        q, k, v = (_maybe_contiguous(x) for x in (q, k, v))
        args = (q, k, v, None, alibi_slopes, dropout_p, softmax_scale, causal, window_size[0],
                window_size[1], softcap, return_softmax and dropout_p > 0, None)
        s32 = None if sink is None else _sink_f32(sink, q)
        out, q_p, k_p, v_p, out_p, lse, s_dmask, rng = (
            paged_attn.fwd(*args) if sink is None else paged_attn.fwd_sink(*args, s32))
        ctx.save_for_backward(q_p, k_p, v_p, out_p, lse, rng, *(() if sink is None else (s32,)))
        ctx.args = (dropout_p, softmax_scale, causal, window_size, softcap, alibi_slopes,
                    deterministic, q.shape[-1])
        ctx.sink_dtype = None if sink is None else sink.dtype
        return out, lse, s_dmask

    @staticmethod
    def backward(ctx, dout, *_):
        q, k, v, out, lse, rng, *s32 = ctx.saved_tensors
        dropout_p, scale, causal, window, softcap, alibi, deterministic, d_og = ctx.args
        dq, dk, dv, softmax_d = paged_attn.bwd(_maybe_contiguous(dout), q, k, v, out, lse, None,
                                               None, None, alibi, dropout_p, scale, causal,
                                               window[0], window[1], softcap, deterministic, None,
                                               rng)
        dsink = _sink_grad(ctx, lse, softmax_d, s32[0] if s32 else None, False)
        dq, dk, dv = dq[..., :d_og], dk[..., :d_og], dv[..., :d_og]
        return (dq, dk, dv, dsink) + (None,) * 8


def _mla_prefill(q, k, v, packed, dropout_p, softmax_scale, causal, window_size, softcap,
                 alibi_slopes, sink, block_table=None):
    """`flash_attn_func` / `flash_attn_varlen_func` with v narrower than q: MLA prefill in its
    un-absorbed form, q and k with 192 features a head (128 "nope" + 64 rotary), v with 128
    (`paged_attn.fwd_mla` / `varlen_fwd_mla`, one HIP launch, no padded copy of v and no slice of
    the output).  `packed`: () or (cu_seqlens_q, cu_seqlens_k, seqused_k, max_seqlen_q,
    max_seqlen_k).  Forward only; every argument the kernel has no code for is refused by name.
    Returns (out [..., h, 128], lse)."""
    pair = (q.shape[-1], v.shape[-1])
    if pair != (192, 128) or k.shape[-1] != 192:
        raise NotImplementedError("q/k/v head sizes: v narrower or wider than q is supported for MLA "
                                  f"prefill at (192, 128) only (got q {q.shape[-1]}, k {k.shape[-1]}, "
                                  f"v {v.shape[-1]})")
    if q.dtype == torch.float8_e4m3fn:
        raise NotImplementedError("fp8 q/k/v: MLA prefill (192, 128) takes bf16 or fp16")
    if dropout_p != 0.0:
        raise NotImplementedError(f"dropout_p={dropout_p}: MLA prefill (192, 128) has no dropout")
    if alibi_slopes is not None:
        raise NotImplementedError("alibi_slopes: MLA prefill (192, 128) has no ALiBi")
    if softcap != 0.0:
        raise NotImplementedError(f"softcap={softcap}: MLA prefill (192, 128) has no softcap")
    if sink is not None:
        raise NotImplementedError("sink: MLA prefill (192, 128) has no attention sink")
    if block_table is not None:
        raise NotImplementedError("block_table: MLA prefill (192, 128) reads no paged K/V")
    if torch.is_grad_enabled():
        for name, x in (("q", q), ("k", k), ("v", v)):
            if x.requires_grad:
                raise NotImplementedError(f"{name}.requires_grad: MLA prefill (192, 128) has no backward "
                                          "here (use flash_attn_mla_func / flash_attn_mla_varlen_func, "
                                          "or call it under torch.no_grad())")
    op = paged_attn.varlen_fwd_mla if packed else paged_attn.fwd_mla
    with torch.no_grad():
        out, lse = op(q.detach(), k.detach(), v.detach(), None, *packed, float(softmax_scale),
                      bool(causal), int(window_size[0]), int(window_size[1]))
    return out, lse


def _mla_dout(dout):
    """dout as the backward kernels read it: unit-stride last dimension, 16-byte aligned rows"""
    ok = (dout.stride(-1) == 1 and dout.data_ptr() % 16 == 0 and
          all(s % 8 == 0 for n, s in zip(dout.shape[:-1], dout.stride()[:-1]) if n != 1))
    return dout if ok else dout.contiguous()


def _check_mla_func(q, k, v):
    pair = (q.shape[-1], k.shape[-1], v.shape[-1])
    if pair != (192, 192, 128):
        raise NotImplementedError("flash_attn_mla_func: head sizes (q, k, v) = (192, 192, 128) only "
                                  f"(got {pair})")
    if q.dtype not in (torch.bfloat16, torch.float16):
        raise NotImplementedError(f"q.dtype={q.dtype}: MLA prefill (192, 128) takes bf16 or fp16")


class _FlashAttnMlaFunc(torch.autograd.Function):
    """MLA prefill (192, 128) with its gradient, dense or packed: the unchanged `fwd_mla` /
    `varlen_fwd_mla` forward, `bwd_mla` / `varlen_bwd_mla` by the tensors' own strides.
    `packed`: () or (cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k)."""

    @staticmethod
    def forward(ctx, q, k, v, packed, softmax_scale, causal, window_size):
        if packed:
            cu_q, cu_k, max_q, max_k = packed
            out, lse = paged_attn.varlen_fwd_mla(q, k, v, None, cu_q, cu_k, None, max_q, max_k,
                                                 softmax_scale, causal, *window_size)
            ctx.save_for_backward(q, k, v, out, lse, cu_q, cu_k)
        else:
            out, lse = paged_attn.fwd_mla(q, k, v, None, softmax_scale, causal, *window_size)
            ctx.save_for_backward(q, k, v, out, lse)
        ctx.args = (packed[2:], softmax_scale, causal, window_size)
        ctx.mark_non_differentiable(lse)
        return out, lse

    @staticmethod
    def backward(ctx, dout, *_):
        q, k, v, out, lse, *cu = ctx.saved_tensors
        maxes, scale, causal, window = ctx.args
        op = paged_attn.varlen_bwd_mla if cu else paged_attn.bwd_mla
        dq, dk, dv, _ = op(_mla_dout(dout), q, k, v, out, lse, None, None, None, *cu, *maxes, scale,
                           causal, *window)
        return dq, dk, dv, None, None, None, None


def flash_attn_mla_func(q, k, v, causal=False, window_size=(-1, -1), softmax_scale=None,
                        deterministic=False, return_attn_probs=False):
    """MLA prefill in its un-absorbed form, differentiable: q [b, sq, h, 192], k [b, sk, hk, 192]
    (128 "nope" + 64 rotary features a head), v [b, sk, hk, 128] -> out [b, sq, h, 128]; bf16 or
    fp16, views are fine (last dimension contiguous, 16-byte aligned, no copies).

    The forward is `flash_attn_func`'s at this shape, bit for bit.  The backward is three HIP
    launches without atomics (`paged_attn.bwd_mla`): dq, dk [.., 192] and dv [.., 128], no padding
    of v / out / dout to 192 and no slices.  deterministic is accepted and has no effect: every
    gradient element has one writer and one summation order, so results are always bitwise
    reproducible.  softmax_scale defaults to q.shape[-1] ** -0.5.  With return_attn_probs the
    result is (out, lse, None); the LSE carries no gradient."""
    _check_mla_func(q, k, v)
    if softmax_scale is None:
        softmax_scale = q.shape[-1] ** (-0.5)
    out, lse = _FlashAttnMlaFunc.apply(q, k, v, (), float(softmax_scale), bool(causal),
                                       tuple(int(w) for w in window_size))
    return out if not return_attn_probs else (out, lse, None)


def flash_attn_mla_varlen_func(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k,
                               causal=False, window_size=(-1, -1), softmax_scale=None,
                               deterministic=False, return_attn_probs=False):
    """`flash_attn_mla_func` over packed sequences: q [total_q, h, 192], k [total_k, hk, 192],
    v [total_k, hk, 128], cu_seqlens int32 [b + 1] -> out [total_q, h, 128]; the LSE is
    [h, total_q].  Backward: `paged_attn.varlen_bwd_mla`."""
    _check_mla_func(q, k, v)
    if softmax_scale is None:
        softmax_scale = q.shape[-1] ** (-0.5)
    packed = (cu_seqlens_q, cu_seqlens_k, int(max_seqlen_q), int(max_seqlen_k))
    out, lse = _FlashAttnMlaFunc.apply(q, k, v, packed, float(softmax_scale), bool(causal),
                                       tuple(int(w) for w in window_size))
    return out if not return_attn_probs else (out, lse, None)


def flash_attn_func(q, k, v, dropout_p=0.0, causal=False, window_size=(-1, -1), softcap=0.0,
                    alibi_slopes=None, deterministic=False, return_attn_probs=False, *,
                    softmax_scale=None, q_descale=None, k_descale=None, v_descale=None,
                    out_dtype=torch.bfloat16, sink=None):
    """q [b, sq, h, d], k/v [b, sk, hk, d] -> out [b, sq, h, d] (test.py:41-72).

    Extension: float8_e4m3fn q/k/v (with per-tensor descales, value = stored x descale) run the
    fp8-MFMA forward (forward only, d = 128, no ALiBi / softcap / dropout); out is `out_dtype`.

    sink: a per-head logit [h] (any float dtype; gpt-oss's learned sinks) that joins each row's
    softmax denominator and carries no value, in the units of the scaled scores; its gradient is
    returned in sink's dtype.  Not with ALiBi, dropout or fp8 q/k/v; with return_attn_probs the
    third result is None.

    MLA prefill: q and k [.., 192], v [.., 128] (v.shape[-1] != q.shape[-1]) run the (192, 128)
    forward (`_mla_prefill`): out [b, sq, h, 128]; forward only, no dropout / ALiBi / softcap /
    sink; the default scale is still q.shape[-1] ** -0.5."""
    if softmax_scale is None:
        softmax_scale = q.shape[-1] ** (-0.5)
    if v.shape[-1] != q.shape[-1]:
        out, lse = _mla_prefill(q, k, v, (), dropout_p, softmax_scale, causal, window_size, softcap,
                                alibi_slopes, sink)
        return out if not return_attn_probs else (out, lse, None)
    if sink is not None:
        _check_sink_args(q, dropout_p, alibi_slopes)
    if q.dtype == torch.float8_e4m3fn:
        # the fp8 forward has no dropout / softcap / ALiBi: refuse instead of dropping them
        if dropout_p != 0.0 or softcap != 0.0 or alibi_slopes is not None:
            raise NotImplementedError("fp8 q/k/v: dropout, softcap and ALiBi are not supported "
                                      f"(dropout_p={dropout_p}, softcap={softcap}, "
                                      f"alibi={'set' if alibi_slopes is not None else None})")
        out, lse = flash_attn_fp8_func(q, k, v, q_descale, k_descale, v_descale, softmax_scale,
                                       causal, window_size, out_dtype, return_lse=True)
        return out if not return_attn_probs else (out, lse, None)
    out, lse, s_dmask = _FlashAttnFunc.apply(q, k, v, sink, dropout_p, softmax_scale, causal,
                                             tuple(int(w) for w in window_size), softcap,
                                             alibi_slopes, deterministic, return_attn_probs)
    return out if not return_attn_probs else (out, lse, s_dmask)


def merge_attn_states(outs, lses, *, sink=None, packed=False, out=None, lse_out=None):
    """Merge partial attention results of the same queries over different keys into the result
    over all of them: one HIP launch (`paged_attn.merge_states`), no copies.

    outs: 1 to 16 tensors [b, rows, h, d] (packed=True: [total_q, h, d]), bf16 or fp16, of one
    shape and one stride set (views are fine: last dimension contiguous, 16-byte aligned);
    lses: their fp32 log-sum-exps [b, h, rows] (packed: [h, total_q]), as `flash_attn_func(...,
    return_attn_probs=True)`, `flash_attn_with_kvcache(..., return_softmax_lse=True)` and the
    fp8 functions return them.  Per row: w_i = exp(lse_i - max lse), O = sum w_i O_i / sum w_i in
    fp32 rounded once, LSE = max + log(sum w_i).  A part whose LSE is +inf (this library's "no
    visible key") or -inf (other libraries') is absent for that row and its O is ignored; a row
    with no part present gets O = 0 and LSE = +inf.

    sink: a per-head logit [h] that joins the merged denominator (as `flash_attn_func`'s sink):
    pass it HERE and not to the partial calls, so that it is counted once.
    out / lse_out: tensors to write into; they may be outs[0] / lses[0] themselves (in-place
    accumulation) and must not overlap any other part.  Returns (out, lse).

    Not differentiable: the results carry no grad.  `flash_attn_func` does not propagate a
    gradient into its LSE output, so a differentiable merge could not be chained through the
    partial calls anyway; the differentiable path over K/V chunks is `sharding.ring_attention`,
    which runs the backward kernels on each chunk with the merged out and LSE."""
    outs, lses = list(outs), list(lses)
    if not outs:
        raise ValueError("merge_attn_states needs at least one part")
    s32 = None if sink is None else _sink_f32(sink, outs[0])
    with torch.no_grad():
        o, lse = paged_attn.merge_states([x.detach() for x in outs], [x.detach() for x in lses],
                                         s32, bool(packed), out, lse_out)
    return o, lse


mla_fp8_cache_row_bytes = 656      # one token of an fp8 latent cache (flash_mla_with_kvcache)


def flash_mla_with_kvcache(q, kv_cache, block_table, cache_seqlens, head_dim_v=512,
                           softmax_scale=None, causal=False, num_splits=0, out=None, *, indices=None):
    """Decode attention for multi-head latent attention (DeepSeek-V2/V3/R1, Kimi) in its absorbed
    form, over a paged latent KV cache: one HIP launch (`paged_attn.mla_decode`) plus the split
    combine, no copies.

    q: [b, seqlen_q, h, 576] bf16 or fp16 (a view is fine: last dimension contiguous, 16-byte
    aligned); kv_cache: [num_blocks, page_block_size, 1, 576] contiguous, page_block_size a
    multiple of 16; block_table: int32 [b, max_blocks_per_seq]; cache_seqlens: int32 [b].
    Every head attends over the one shared 576-wide latent row per token (512 compressed-KV
    features + 64 rotary features); the value is its first head_dim_v = 512 features.
    softmax_scale defaults to q.shape[-1] ** -0.5 (pass the model's own: DeepSeek's is not that);
    causal is bottom-right aligned, as in `flash_attn_with_kvcache`.  A row without a visible key
    gives out = 0 and softmax_lse = +inf.  num_splits: 0 chooses, 1 forces a single pass.

    An fp8 cache - kv_cache of dtype uint8 or float8_e4m3fn with a last dimension of 656 bytes
    (`mla_fp8_cache_row_bytes`): 512 e4m3fn latent features, four fp32 descales (one per 128
    features) and the 64 rotary features in q's dtype, FlashMLA's fp8 KV cache / vLLM's
    `fp8_ds_mla`, as `mla_cache_append_fp8` writes it - takes `paged_attn.mla_decode_fp8`: the
    latent features are dequantised to q's dtype (one fp32 product, rounded once) and everything
    else is as above.

    indices (keyword only; FlashMLA's argument of that name, DeepSeek-V3.2's sparse attention):
    int32 [b, seqlen_q, topk], last dimension contiguous.  Query (b, pos) then attends over exactly
    the cache rows at the valid entries of indices[b, pos, :], in that order, gathered inside the
    kernel (`paged_attn.mla_decode_sparse` / `mla_decode_sparse_fp8`).  An entry is a physical
    slot, block * page_block_size + row (what `mla_cache_append_fp8`'s slot_mapping holds); any
    value outside [0, num_blocks * page_block_size) - -1 is the usual padding - contributes
    nothing, and the kernel checks every entry, so no host sync is needed.  block_table and
    cache_seqlens are not read and may be None; causal=True raises (visibility is the indexer's
    choice).  A position whose entries are all invalid gives out = 0 and softmax_lse = +inf.

    Returns (out [b, seqlen_q, h, 512], softmax_lse fp32 [b, h, seqlen_q]).  Not differentiable."""
    if softmax_scale is None:
        softmax_scale = q.shape[-1] ** (-0.5)
    fp8 = kv_cache.dtype in (torch.uint8, torch.float8_e4m3fn) and kv_cache.shape[-1] == mla_fp8_cache_row_bytes
    if indices is not None:
        if causal:
            raise ValueError("flash_mla_with_kvcache: causal=True cannot be combined with indices "
                             "(the indexer decides what a position sees)")
        op = paged_attn.mla_decode_sparse_fp8 if fp8 else paged_attn.mla_decode_sparse
        with torch.no_grad():
            o, lse = op(q.detach(), kv_cache.detach(), indices, int(head_dim_v), float(softmax_scale),
                        int(num_splits), out)
        return o, lse
    op = paged_attn.mla_decode_fp8 if fp8 else paged_attn.mla_decode
    with torch.no_grad():
        o, lse = op(q.detach(), kv_cache.detach(), block_table, cache_seqlens, int(head_dim_v),
                    float(softmax_scale), bool(causal), int(num_splits), out)
    return o, lse


def mla_cache_append_fp8(latent, k_pe, kv_cache, slot_mapping):
    """Append tokens to an fp8 paged latent KV cache (the layout `flash_mla_with_kvcache` reads:
    rows of `mla_fp8_cache_row_bytes` = 656 bytes), one HIP launch, no host sync.

    latent: [tokens, 512] and k_pe: [tokens, 64], bf16 or fp16 (views are fine - typically the two
    parts of one [tokens, 576] tensor: last dimension contiguous, 16-byte aligned rows); k_pe is
    already rotated and is copied.  kv_cache: uint8 or float8_e4m3fn [num_blocks, page_block_size,
    1, 656], page_block_size a multiple of 16, written in place.  slot_mapping: int64 [tokens],
    slot = block * page_block_size + row (vLLM's `concat_and_cache_mla`); a negative or
    out-of-range slot is skipped.  Each 128-feature group of a latent row gets its own scale:
    descale = amax / 448 (1.0 for an all-zero group), bytes = e4m3fn(clamp(x * (1 / descale)))."""
    with torch.no_grad():
        paged_attn.mla_cache_append_fp8(latent.detach(), k_pe.detach(), kv_cache, slot_mapping)


_GRANULARITY = {"tensor": 0, "head": 1}


def quantize_fp8(x, granularity="tensor", group=1, cu_seqlens=None, *, max_seqlen=None):
    """bf16 / fp16 x [b, s, h, d] (any strides, last dimension contiguous) or, with cu_seqlens
    (int32 [b + 1]), packed [total, h, d] -> (x8, descale): x8 float8_e4m3fn of x's shape,
    descale fp32 with x ~ x8 * descale.  One HIP call of two passes over x, no host sync.

    granularity "tensor": one scale, descale [1]; "head": one per (batch or sequence, group of
    `group` consecutive heads), descale [b, h // group] - group = h // hk for q (the fp8 forward
    takes q's descale per kv head), 1 for k and v.  descale = amax / 448 (1.0 for an all-zero or
    empty set).  max_seqlen (packed): the longest sequence if known; the default bounds it by
    `total`, so no length is read on the host."""
    if granularity not in _GRANULARITY:
        raise ValueError(f"granularity must be 'tensor' or 'head' (got {granularity!r})")
    x8, descale = paged_attn.quantize_fp8(x, _GRANULARITY[granularity], int(group), cu_seqlens,
                                          0 if max_seqlen is None else int(max_seqlen))
    return x8, descale


def _as_device_descale(x, device):
    if x is None:
        return torch.ones(1, dtype=torch.float32, device=device)
    if isinstance(x, torch.Tensor):
        return x.to(device=device, dtype=torch.float32)
    return torch.full((1,), float(x), dtype=torch.float32, device=device)


def _quantize_qkv(q, k, v, quantize, descales, cu_q=None, cu_k=None, max_q=None, max_k=None):
    """quantize= of the fp8 functions: bf16 / fp16 q, k, v -> fp8 with device descales (q's per kv
    head under "head")."""
    if quantize not in _GRANULARITY:
        raise ValueError(f"quantize must be None, 'tensor' or 'head' (got {quantize!r})")
    if any(x is not None for x in descales):
        raise ValueError("quantize= computes the descales: do not pass q/k/v_descale with it")
    if q.dtype not in (torch.bfloat16, torch.float16) or k.dtype != q.dtype or v.dtype != q.dtype:
        raise TypeError("quantize= needs bf16 or fp16 q, k and v of one dtype")
    group = q.shape[-2] // k.shape[-2]
    q8, qd = quantize_fp8(q, quantize, group, cu_q, max_seqlen=max_q)
    k8, kd = quantize_fp8(k, quantize, 1, cu_k, max_seqlen=max_k)
    v8, vd = quantize_fp8(v, quantize, 1, cu_k, max_seqlen=max_k)
    return q8, k8, v8, qd, kd, vd


def _fp8_forward(op, q, k, v, packed, descales, softmax_scale, causal, window_size, out_dtype,
                 quantize):
    """What the two fp8 functions share: the refusals, the default scale, quantize= and the
    descale dispatch.  `op`: "fwd_fp8" / "varlen_fwd_fp8"; `packed`: () or (cu_seqlens_q,
    cu_seqlens_k, seqused_k, max_seqlen_q, max_seqlen_k), the op's arguments between `out` and
    the descales.  When any descale is a CUDA tensor all three go to the op's _ex twin as device
    tensors (one element or [batch, heads_k]) and nothing is read on the host; otherwise they are
    passed by value.  Returns (out, lse)."""
    if q.requires_grad or k.requires_grad or v.requires_grad:
        raise NotImplementedError("the fp8 forward has no backward")
    if out_dtype not in (torch.bfloat16, torch.float16):
        raise ValueError("out_dtype must be bfloat16 or float16")
    if softmax_scale is None:
        softmax_scale = q.shape[-1] ** (-0.5)
    if quantize is not None:
        cu_q, cu_k, _, max_q, max_k = packed or (None,) * 5
        q, k, v, *descales = _quantize_qkv(q, k, v, quantize, descales, cu_q, cu_k, max_q, max_k)
    q, k, v = (_maybe_contiguous(x) for x in (q, k, v))
    if any(isinstance(x, torch.Tensor) and x.is_cuda for x in descales):
        op, descales = op + "_ex", [_as_device_descale(x, q.device) for x in descales]
    else:
        descales = [1.0 if x is None else float(x) for x in descales]
    return getattr(paged_attn, op)(q, k, v, None, *packed, *descales, softmax_scale, causal,
                                   int(window_size[0]), int(window_size[1]),
                                   out_dtype == torch.float16)


def flash_attn_fp8_func(q, k, v, q_descale=None, k_descale=None, v_descale=None,
                        softmax_scale=None, causal=False, window_size=(-1, -1),
                        out_dtype=torch.bfloat16, return_lse=False, *, quantize=None):
    """fp8 e4m3fn q [b, sq, h, 128], k/v [b, sk, hk, 128] with descales (value = stored x
    descale; None = 1.0): both GEMMs on the gfx950 fp8 MFMA.  Forward only.

    Descales: Python floats or CPU tensors (one element) are passed by value; CUDA tensors of one
    element or of shape [b, hk] (FA3's layout; q's per kv head) are read by the kernel, with no
    host sync.  quantize="tensor" | "head": q, k, v are bf16 / fp16 and are quantised first
    (`quantize_fp8`, three calls), all on the device."""
    out, lse = _fp8_forward("fwd_fp8", q, k, v, (), (q_descale, k_descale, v_descale),
                            softmax_scale, causal, window_size, out_dtype, quantize)
    return (out, lse) if return_lse else out


def flash_attn_kvpacked_func(q, kv, dropout_p=0.0, softmax_scale=None, causal=False,
                             window_size=(-1, -1), softcap=0.0, alibi_slopes=None,
                             deterministic=False, return_softmax=False, *, sink=None):
    """kv [b, sk, 2, hk, d] (test.py:74-100)."""
    return flash_attn_func(q, kv[:, :, 0], kv[:, :, 1], dropout_p, causal, window_size, softcap,
                           alibi_slopes, deterministic, return_softmax,
                           softmax_scale=softmax_scale, sink=sink)


class _FlashAttnVarlenFunc(torch.autograd.Function):
    """sink: as _FlashAttnFunc (`varlen_fwd_sink`, the unchanged `varlen_bwd`, `sink_bwd`)."""

    @staticmethod
    def forward(ctx, q, k, v, sink, cu_q, cu_k, max_q, max_k, dropout_p, softmax_scale, causal,
                window_size, softcap, alibi_slopes, deterministic, return_softmax, block_table):
        q, k, v = (_maybe_contiguous(x) for x in (q, k, v))
        args = (q, k, v, None, cu_q, cu_k, None, block_table, alibi_slopes, max_q, max_k, dropout_p,
                softmax_scale, False, causal, window_size[0], window_size[1], softcap,
                return_softmax and dropout_p > 0, None)
        s32 = None if sink is None else _sink_f32(sink, q)
        out, q_p, k_p, v_p, out_p, lse, s_dmask, rng = (
            paged_attn.varlen_fwd(*args) if sink is None else paged_attn.varlen_fwd_sink(*args, s32))
        ctx.save_for_backward(q_p, k_p, v_p, out_p, lse, cu_q, cu_k, rng,
                              *(() if sink is None else (s32,)))
        ctx.args = (max_q, max_k, dropout_p, softmax_scale, causal, window_size, softcap,
                    alibi_slopes, deterministic, q.shape[-1], block_table is not None)
        ctx.sink_dtype = None if sink is None else sink.dtype
        return out, lse, s_dmask

    @staticmethod
    def backward(ctx, dout, *_):
        q, k, v, out, lse, cu_q, cu_k, rng, *s32 = ctx.saved_tensors
        (max_q, max_k, dropout_p, scale, causal, window, softcap, alibi, deterministic, d_og,
         paged) = ctx.args
        if paged:
            raise RuntimeError("backward through a paged K/V cache is not supported")
        dq, dk, dv, softmax_d = paged_attn.varlen_bwd(
            _maybe_contiguous(dout), q, k, v, out, lse, None, None, None, cu_q, cu_k, alibi, max_q,
            max_k, dropout_p, scale, False, causal, window[0], window[1], softcap, deterministic,
            None, rng)
        dsink = _sink_grad(ctx, lse, softmax_d, s32[0] if s32 else None, True)
        dq, dk, dv = dq[..., :d_og], dk[..., :d_og], dv[..., :d_og]
        return (dq, dk, dv, dsink) + (None,) * 13


def flash_attn_varlen_fp8_func(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k,
                               q_descale=None, k_descale=None, v_descale=None,
                               softmax_scale=None, causal=False, window_size=(-1, -1),
                               out_dtype=torch.bfloat16, return_lse=False, seqused_k=None, *,
                               quantize=None):
    """Packed fp8 e4m3fn q [total_q, h, 128], k/v [total_k, hk, 128], cu_seqlens int32 [b + 1],
    descales (None = 1.0), optional seqused_k int32 [b]: the fp8-MFMA forward over
    variable-length sequences.  Forward only; the LSE is [h, total_q].

    Descales and quantize= as `flash_attn_fp8_func`; a [b, hk] descale is indexed by (sequence,
    kv head)."""
    packed = (cu_seqlens_q, cu_seqlens_k, seqused_k, int(max_seqlen_q), int(max_seqlen_k))
    out, lse = _fp8_forward("varlen_fwd_fp8", q, k, v, packed, (q_descale, k_descale, v_descale),
                            softmax_scale, causal, window_size, out_dtype, quantize)
    return (out, lse) if return_lse else out


def flash_attn_varlen_func(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k,
                           dropout_p=0.0, softmax_scale=None, causal=False,
                           window_size=(-1, -1), softcap=0.0, alibi_slopes=None,
                           deterministic=False, return_attn_probs=False, block_table=None, *,
                           q_descale=None, k_descale=None, v_descale=None,
                           out_dtype=torch.bfloat16, sink=None):
    """Packed q [total_q, h, d], k/v [total_k, hk, d], cu_seqlens int32 (test.py:102-149).

    Extension: float8_e4m3fn q/k/v (with per-tensor descales) run the fp8-MFMA varlen forward
    (forward only, d = 128, no ALiBi / softcap / dropout / block_table); out is `out_dtype`.

    sink: as `flash_attn_func`.

    MLA prefill: q and k [.., 192], v [.., 128] run the (192, 128) forward as in `flash_attn_func`
    (out [total_q, h, 128], LSE [h, total_q]; no block_table)."""
    if softmax_scale is None:
        softmax_scale = q.shape[-1] ** (-0.5)
    if v.shape[-1] != q.shape[-1]:
        packed = (cu_seqlens_q, cu_seqlens_k, None, int(max_seqlen_q), int(max_seqlen_k))
        out, lse = _mla_prefill(q, k, v, packed, dropout_p, softmax_scale, causal, window_size,
                                softcap, alibi_slopes, sink, block_table)
        return out if not return_attn_probs else (out, lse, None)
    if sink is not None:
        _check_sink_args(q, dropout_p, alibi_slopes)
    if q.dtype == torch.float8_e4m3fn:
        # refuse what the fp8 forward lacks instead of dropping it
        if dropout_p != 0.0 or softcap != 0.0 or alibi_slopes is not None or block_table is not None:
            raise NotImplementedError("fp8 q/k/v: dropout, softcap, ALiBi and block_table are not "
                                      f"supported (dropout_p={dropout_p}, softcap={softcap}, "
                                      f"alibi={'set' if alibi_slopes is not None else None}, "
                                      f"block_table={'set' if block_table is not None else None})")
        out, lse = flash_attn_varlen_fp8_func(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q,
                                              max_seqlen_k, q_descale, k_descale, v_descale,
                                              softmax_scale, causal, window_size, out_dtype,
                                              return_lse=True)
        return out if not return_attn_probs else (out, lse, None)
    out, lse, s_dmask = _FlashAttnVarlenFunc.apply(
        q, k, v, sink, cu_seqlens_q, cu_seqlens_k, int(max_seqlen_q), int(max_seqlen_k), dropout_p,
        softmax_scale, causal, tuple(int(w) for w in window_size), softcap, alibi_slopes,
        deterministic, return_attn_probs, block_table)
    return out if not return_attn_probs else (out, lse, s_dmask)


def flash_attn_varlen_kvpacked_func(q, kv, cu_seqlens_q, cu_seqlens_k, max_seqlen_q,
                                    max_seqlen_k, dropout_p=0.0, softmax_scale=None,
                                    causal=False, window_size=(-1, -1), softcap=0.0,
                                    alibi_slopes=None, deterministic=False,
                                    return_attn_probs=False, *, sink=None):
    """kv [total_k, 2, hk, d] (test.py:151-187)."""
    return flash_attn_varlen_func(q, kv[:, 0], kv[:, 1], cu_seqlens_q, cu_seqlens_k,
                                  max_seqlen_q, max_seqlen_k, dropout_p, softmax_scale, causal,
                                  window_size, softcap, alibi_slopes, deterministic,
                                  return_attn_probs, sink=sink)


def flash_attn_with_kvcache(q, k_cache, v_cache, k=None, v=None, rotary_cos=None,
                            rotary_sin=None,
                            cache_seqlens: Optional[Union[int, torch.Tensor]] = None,
                            cache_batch_idx: Optional[torch.Tensor] = None,
                            cache_leftpad: Optional[torch.Tensor] = None,
                            block_table: Optional[torch.Tensor] = None, softmax_scale=None,
                            causal=False, window_size=(-1, -1), softcap=0.0,
                            rotary_interleaved=True, alibi_slopes=None, num_splits=0,
                            return_softmax_lse=False, k_scale=1.0, v_scale=1.0, *, sink=None):
    """Decode / chunked prefill against a (paged) KV cache (test.py:189-245).  With k/v the new
    rows are first written into the cache in place at cache_seqlens (rotary_cos/sin: rotary
    embedding on k and q, interleaved = GPT-J pairs), then attended over.

    Extension: a `torch.float8_e4m3fn` paged cache is read natively (dequantised in-kernel as
    fp8 * k_scale / v_scale); it requires `block_table` and `cache_seqlens`.  With k/v (bf16 /
    fp16, q's dtype) the new rows are quantised into it first: K after its rotary in fp32, times
    1 / k_scale, clamped to +-448 and rounded once to e4m3; V times 1 / v_scale likewise
    (k_scale, v_scale positive floats); rotary_cos/sin and rotary_interleaved as for a bf16 cache.
    ALiBi and softcap are not supported with an fp8 cache.

    sink: a per-head logit [h] (any float dtype) in each row's softmax denominator, as
    `flash_attn_func` (forward only here); bf16 / fp16 and fp8 caches alike, not with ALiBi."""
    assert k_cache.stride(-1) == 1, "k_cache must have contiguous last dimension"
    assert v_cache.stride(-1) == 1, "v_cache must have contiguous last dimension"
    if cache_leftpad is not None and (block_table is not None or k_cache.dtype == torch.float8_e4m3fn):
        raise NotImplementedError("cache_leftpad needs a non-paged cache (flash-attn: no Paged KV "
                                  "and leftpad_k at the same time)")
    q, k, v = (_maybe_contiguous(x) for x in (q, k, v))
    if softmax_scale is None:
        softmax_scale = q.shape[-1] ** (-0.5)
    if sink is not None:
        _check_sink_args(q, 0.0, alibi_slopes)
        sink = _sink_f32(sink, q)
    if isinstance(cache_seqlens, int):
        cache_seqlens = torch.full((q.shape[0],), cache_seqlens, dtype=torch.int32, device=q.device)
    window = (int(window_size[0]), int(window_size[1]))
    if k_cache.dtype == torch.float8_e4m3fn:
        if block_table is None or cache_seqlens is None or alibi_slopes is not None or softcap > 0:
            raise NotImplementedError("fp8 K/V cache: paged decode with block_table and "
                                      "cache_seqlens only (no ALiBi, no softcap)")
        if (k is None) != (v is None):
            raise ValueError("If key is supplied, value must also be passed in")
        if k is None and (rotary_cos is not None or rotary_sin is not None):
            raise ValueError("If rotary cos/sin are provided, new key / value to be appended to "
                             "KV cache must also be provided")
        if k is not None:
            # append (+ rotary on k and q) into the fp8 cache, then attend over the grown lengths
            per_token = bool(causal) or window[0] >= 0 or window[1] >= 0
            cache_seqlens, q = paged_attn.kvcache_append_fp8(
                q, k_cache.view(torch.uint8), v_cache.view(torch.uint8), k, v,
                _maybe_contiguous(cache_seqlens), block_table, rotary_cos, rotary_sin,
                float(k_scale), float(v_scale), rotary_interleaved, per_token)
        op = "fwd_kvcache_fp8"
        args = (q, k_cache.view(torch.uint8), v_cache.view(torch.uint8), cache_seqlens,
                block_table, float(k_scale), float(v_scale), softmax_scale, causal, *window,
                num_splits)
    else:
        op = "fwd_kvcache"
        args = (q, k_cache, v_cache, k, v, cache_seqlens, rotary_cos, rotary_sin,
                _maybe_contiguous(cache_batch_idx), _maybe_contiguous(block_table), alibi_slopes,
                None, softmax_scale, causal, *window, softcap, rotary_interleaved, num_splits,
                _maybe_contiguous(cache_leftpad))
    if sink is not None:
        op, args = op + "_sink", args + (sink,)
    out, lse = getattr(paged_attn, op)(*args)
    return (out, lse) if return_softmax_lse else out
