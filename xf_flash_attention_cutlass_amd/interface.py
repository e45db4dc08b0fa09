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


def flash_mla_sparse_fwd(q, kv, indices, sm_scale=None, d_v=512, out=None):
    """Sparse attention of multi-head latent attention over s_q new tokens (DeepSeek-V3.2's prefill;
    FlashMLA's function of this name): one HIP launch (`paged_attn.mla_sparse_fwd`), no key split,
    no scratch, no copies, no host sync.  A workgroup serves one token and 64 heads, so a selected
    row is gathered once per 64 heads.

    q: [s_q, heads, 576] bf16 or fp16 (a view is fine: last dimension contiguous, 16-byte aligned
    rows); kv: [s_kv, 1, 576] of q's dtype, any row stride that is a multiple of 8 elements - a
    paged 16-bit latent cache viewed flat, `kv_cache.view(-1, 1, 576)`, is valid input, its
    indices physical slots (what `mla_index_topk_ragged(slots=slot_mapping)` emits); indices: int32
    [s_q, 1, topk] (or [s_q, topk]), last dimension contiguous.  Token i attends over exactly the
    rows of kv at the valid entries of indices[i], in that order; an entry is valid iff
    0 <= entry < s_kv, every other value (-1 is the usual padding; pad rows of differing lengths with
    it) contributes nothing, and the kernel checks every entry.  The value is the first d_v = 512
    features of the row.  sm_scale defaults to 576 ** -0.5 (pass the model's own).

    An fp8 latent cache - kv of dtype uint8 or float8_e4m3fn, [s_kv, 1, 656] bytes
    (`mla_fp8_cache_row_bytes`; rows any multiple of 16 bytes apart), as `mla_cache_append_fp8`
    writes it: `kv_cache8.view(-1, 1, 656)` is valid input - takes `paged_attn.mla_sparse_fwd_fp8`:
    the call dispatches on kv.dtype, as `flash_mla_with_kvcache` does.  A selected row is gathered
    and dequantised to q's dtype (one fp32 product, rounded once) once per 64 heads, inside the
    kernel: no 16-bit copy of the cache or of the selected rows.  Everything else is as above; out
    and lse equal the fp8 cache's decode route at num_splits=1 bit for bit.

    Returns (out [s_q, heads, 512], max_logits fp32 [s_q, heads], lse fp32 [s_q, heads]): lse is the
    NATURAL-log sum of exponentials of the scaled scores, max_logits their maximum.  A token whose
    entries are all invalid gives out = 0, lse = +inf and max_logits = -inf.  out and lse equal
    `flash_mla_with_kvcache(q[None], cache, None, None, indices=indices[None], num_splits=1)` bit
    for bit.  Not differentiable.

    When to prefer the decode route (`flash_mla_with_kvcache(..., indices=...)`, which splits the
    keys and combines): at up to 16 heads.  There only one of a workgroup's four waves
    has products to do and this call took 2.5 to 3.3 times the decode route's time; at 64 and 128
    heads it took 0.95 of it (MI355X, bf16, s_kv 32768, topk 2048, s_q 512 and 4096:
    DESIGN.md §3.10.3, profiles/mla_sparse_fwd_ab.log).  Over the fp8 cache the same holds, more
    sharply: at 16 heads this call took 2.3 to 2.7 times the fp8 decode route's time, at 64 and 128
    heads 0.73 of it (the decode route converts every selected row once per 16 heads), and 1.12 to 1.15
    times the 16-bit call's over a bf16 copy of the cache (same shapes: DESIGN.md §3.10.4,
    profiles/mla_sparse_fwd_fp8_ab.log)."""
    if sm_scale is None:
        sm_scale = q.shape[-1] ** (-0.5)
    fp8 = kv.dtype in (torch.uint8, torch.float8_e4m3fn)
    op = paged_attn.mla_sparse_fwd_fp8 if fp8 else paged_attn.mla_sparse_fwd
    with torch.no_grad():
        o, max_logits, lse = op(q.detach(), kv.detach(), indices, float(sm_scale), int(d_v), out)
    return o, max_logits, lse


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


def mla_index_cache_block_bytes(page_block_size):
    """Bytes of one block of the MLA index-key cache: `page_block_size` rows of 128 e4m3fn features,
    then `page_block_size` fp32 descales (vLLM's and DeepGEMM's layout)."""
    return 132 * int(page_block_size)


_INDEX_SCALE_FMT = {None: 0, "ue8m0": 1}


def mla_index_cache_append_fp8(k, index_cache, slot_mapping, scale_fmt=None):
    """Append index keys to the fp8 paged index-key cache of DeepSeek-V3.2's lightning indexer
    (vLLM's `indexer_k_quant_and_cache`), one HIP launch, no host sync.

    k: [tokens, 128] bf16 or fp16 (a view is fine: last dimension contiguous, 16-byte aligned rows).
    index_cache: uint8 or float8_e4m3fn [num_blocks, mla_index_cache_block_bytes(page)], page a
    multiple of 16, written in place.  slot_mapping: int64 [tokens], slot = block * page + row - the
    latent cache's slot mapping; a negative or out-of-range slot is skipped.  One scale per row:
    descale = amax / 448 (1.0 for an all-zero row), bytes = e4m3fn(clamp(x * (1 / descale)));
    scale_fmt="ue8m0" (what V3.2 ships) first rounds the descale up to a power of two."""
    if scale_fmt not in _INDEX_SCALE_FMT:
        raise ValueError(f"scale_fmt must be None or 'ue8m0' (got {scale_fmt!r})")
    with torch.no_grad():
        paged_attn.mla_index_cache_append_fp8(k.detach(), index_cache, slot_mapping, _INDEX_SCALE_FMT[scale_fmt])


def mla_index_logits(q8, weights, index_cache, block_table, context_lens, max_seqlen_k, out=None):
    """The lightning indexer's logits over the paged fp8 index-key cache (DeepGEMM's
    `fp8_paged_mqa_logits`), one HIP launch (`paged_attn.mla_index_logits`), no scratch, no copies:

        logits[b * seqlen_q + i, s] = descale[b, s] * sum_h weights[., h] * relu(q8[b, i, h] . k8[b, s])

    for the keys s position i may see (bottom-right causal within context_lens[b]) and -inf for the
    others up to max_seqlen_k, so `torch.topk` over a row is valid as it stands.

    q8: [b, seqlen_q, heads, 128] float8_e4m3fn or uint8, heads 32 or 64 (a view is fine: last
    dimension contiguous, 16-byte aligned rows); weights: fp32 [b * seqlen_q, heads] with q's own
    quantisation scale, the softmax scale and heads ** -0.5 folded in (any sign); block_table: int32
    [b, max_blocks_per_seq]; context_lens: int32 [b]; out: fp32 [b * seqlen_q, max_seqlen_k] with
    unit column stride (a column slice of a wider buffer is fine; the rest of it is not touched).
    Returns the logits.  Not differentiable."""
    with torch.no_grad():
        return paged_attn.mla_index_logits(q8.detach(), weights.detach(), index_cache, block_table,
                                           context_lens, int(max_seqlen_k), out)


def mla_index_logits_ragged(q8, weights, k8, k_scale, ks, ke, out=None):
    """The lightning indexer's logits for prefill and chunked prefill (DeepGEMM's `fp8_mqa_logits`),
    one HIP launch (`paged_attn.mla_index_logits_ragged`), no scratch, no [rows, heads, keys] tensor:

        logits[r, s] = k_scale[s] * sum_h weights[r, h] * relu(q8[r, h] . k8[s])    ks[r] <= s < ke[r]

    with ks / ke clamped to [0, N], and -inf for every other s < N (a row with ke <= ks is all -inf),
    so `torch.topk` over a row is valid as it stands.  Rows are new tokens of one causal sequence
    (ks = 0, ke = position + 1), of several packed sequences (each row the range of its own
    sequence's keys) or of a chunk over cached keys; a key outside a row's range never reaches it.

    q8: [M, heads, 128] float8_e4m3fn or uint8, heads 32 or 64 (a view is fine: last dimension
    contiguous, 16-byte aligned rows); weights: fp32 [M, heads] with q's quantisation scale, the
    softmax scale and heads ** -0.5 folded in (any sign); k8: [N, 128] float8_e4m3fn or uint8 (row
    stride a multiple of 16 bytes); k_scale: fp32 [N]; ks, ke: int32 [M]; out: fp32 [M, N] with unit
    column stride (a column slice of a wider buffer is fine; the rest of it is not touched).

    k8 and k_scale need no quantiser of their own: `mla_index_cache_append_fp8(k, cache, arange(N))`
    into a one-block cache `[1, mla_index_cache_block_bytes(page)]` with page = N rounded up to 16
    leaves `page * 128` key bytes followed by `page` fp32 descales, so
    `k8 = cache[0, :N * 128].view(N, 128)` and
    `k_scale = cache[0, page * 128:].view(torch.float32)[:N]` are views of it.
    Returns the logits.  Not differentiable."""
    with torch.no_grad():
        return paged_attn.mla_index_logits_ragged(q8.detach(), weights.detach(), k8, k_scale, ks, ke, out)


def mla_index_topk_slots(logits, block_table, context_lens, topk, seqlen_q=1, page_block_size=64):
    """The indexer's choice as `flash_mla_with_kvcache(indices=...)` takes it: int32 [b, seqlen_q,
    topk] of physical slots, from `mla_index_logits`' result.  A few lines of torch glue, not a
    kernel (the selection kernel is `mla_index_topk`, which returns the same set in ascending key
    position; this one stays as the eager baseline): `torch.topk` over each row (over all of it when
    the row is shorter than topk, the rest padded), an entry whose logit is -inf becomes -1, the
    others go through the block table, slot = block_table[b, s // page] * page + s % page with
    page = page_block_size (the model's is 64).  context_lens is not read - the logits carry the
    visibility - and is taken so that a selection kernel can replace this without a new signature."""
    rows, width = logits.shape
    b = rows // int(seqlen_q)
    page = int(page_block_size)
    val, pos = torch.topk(logits, min(int(topk), width), dim=1)
    table = block_table.long().repeat_interleave(int(seqlen_q), dim=0)
    slots = torch.gather(table, 1, pos // page) * page + pos % page
    slots = torch.where(val == float("-inf"), torch.full_like(slots, -1), slots).int()
    if slots.shape[1] < int(topk):
        slots = torch.nn.functional.pad(slots, (0, int(topk) - slots.shape[1]), value=-1)
    return slots.view(b, int(seqlen_q), int(topk))


MLA_INDEX_TOPK_SPLIT_CHUNK = 16384      # columns of one workgroup the automatic split aims at
MLA_INDEX_TOPK_SPLIT_WORKGROUPS = 256   # ... as long as the launch stays within this many workgroups (the MI355X's CUs)


def mla_index_topk_splits(max_seqlen_k, topk, rows=1):
    """The workgroups a row `mla_index_topk(splits=None)` gives: 1, the one-workgroup kernel, for
    every launch whose rows it keeps in LDS (max_seqlen_k <= 32768) and wherever the split kernels'
    limits cannot be met (splits in [2, 16], splits * topk <= 32768, a chunk of at most 32768
    columns); else one per MLA_INDEX_TOPK_SPLIT_CHUNK columns, fewer where `rows` of them would be
    more than MLA_INDEX_TOPK_SPLIT_WORKGROUPS workgroups, never fewer than the chunk limit asks for."""
    stage = paged_attn._mla_index_topk_stage
    if max_seqlen_k <= stage:
        return 1
    least = -(-max_seqlen_k // stage)
    splits = max(least, min(-(-max_seqlen_k // MLA_INDEX_TOPK_SPLIT_CHUNK), MLA_INDEX_TOPK_SPLIT_WORKGROUPS // max(rows, 1)))
    return splits if splits <= min(16, stage // max(topk, 1)) else 1


def mla_index_topk(logits, block_table, context_lens, topk, seqlen_q=1, page_block_size=64, max_seqlen_k=None,
                   out=None, num_blocks=None, splits=None):
    """The indexer's choice as `flash_mla_with_kvcache(indices=...)` takes it, in HIP
    (`paged_attn.mla_index_topk`: an exact radix select, no host sync, graph-capturable, bitwise
    reproducible): int32 [b, seqlen_q, topk] of physical slots from `mla_index_logits`' result.
    One launch and no scratch with one workgroup a row; `splits` >= 2 cuts every row over that many
    workgroups (`paged_attn.mla_index_topk_split`: two launches and scratch from the library's
    per-stream pool) - the result is the same, bit for bit.  splits=1 forces the one-workgroup
    kernel; None chooses (`mla_index_topk_splits`): rows the kernel keeps in LDS, max_seqlen_k <=
    32768, stay on it, longer ones are split.

    Row b * seqlen_q + i selects among the columns position i may see (bottom-right causal within
    min(context_lens[b], max_seqlen_k); nothing behind them is read, so they need not hold -inf).
    The order is the order on floats with -0.0 == +0.0 and +inf the largest; -inf and NaN are never
    selected.  Of equal values at the threshold the lowest key positions win.  The selected
    positions come in ASCENDING key position (not by descending logit, as `mla_index_topk_slots`
    gives them), each as block_table[b, s // page] * page + s % page, then -1 up to topk; a table
    entry outside [0, num_blocks) gives -1 in place.

    logits: fp32 [b * seqlen_q, keys], last dimension contiguous (a view of a wider buffer is fine);
    block_table: int32 [b, max_blocks_per_seq]; context_lens: int32 [b]; max_seqlen_k defaults to
    logits.shape[1]; num_blocks: blocks of the cache, or None for "unknown" - then only the int32
    range of a slot bounds a table entry (INT32_MAX // page_block_size is passed down); out: int32
    [b, seqlen_q, topk], rows may lie further apart than topk (the rest of them is not touched).
    Returns the indices.  Not differentiable."""
    max_k = int(logits.shape[1] if max_seqlen_k is None else max_seqlen_k)
    splits = mla_index_topk_splits(max_k, int(topk), logits.shape[0]) if splits is None else int(splits)
    args = (logits.detach(), block_table, context_lens, int(topk), int(seqlen_q), int(page_block_size), max_k,
            -1 if num_blocks is None else int(num_blocks), out)
    with torch.no_grad():
        return paged_attn.mla_index_topk(*args) if splits == 1 else paged_attn.mla_index_topk_split(*args, splits)


def mla_index_topk_ragged(logits, ks, ke, topk, slots=None, out=None):
    """The indexer's choice for prefill and chunked prefill, in one HIP launch
    (`paged_attn.mla_index_topk_ragged`: an exact radix select, one workgroup of 4 waves per row, no
    scratch, no host sync, graph-capturable, bitwise reproducible): int32 [M, topk] from
    `mla_index_logits_ragged`'s result.

    Row r selects among the columns clamp(ks[r], 0, N) <= s < clamp(ke[r], 0, N) and reads nothing
    outside them (they need not hold -inf); ke <= ks gives a row of -1.  Order, ties and output order
    are `mla_index_topk`'s: the order on floats with -0.0 == +0.0 and +inf the largest; -inf and NaN
    are never selected; of equal values at the threshold the lowest columns win; the selected columns
    come in ASCENDING column order, then -1 up to topk.  With `slots` (int64 [N]: the physical cache
    slot of key column s - the append's slot_mapping for new tokens, the gather list for cached
    ones) column s is emitted as slots[s], or as -1 in place where that is outside [0, 2^31);
    without it as s itself (an index into k8 or into an un-paged [N, 576] latent tensor).

    logits: fp32 [M, N], last dimension contiguous, any row stride >= N (a view of a wider buffer is
    fine); ks, ke: int32 [M]; out: int32 [M, topk] with unit column stride (a column slice of a wider
    buffer is fine; the rest of it is not touched).

    A chunked-prefill step over a paged latent cache, HIP end to end:

        logits = mla_index_logits_ragged(q8, weights, k8, k_scale, ks, ke)
        idx = mla_index_topk_ragged(logits, ks, ke, topk, slots=slots)
        out, max_logits, lse = flash_mla_sparse_fwd(q, kv_cache.view(-1, 1, 576), idx, sm_scale)

    Returns the indices.  Not differentiable."""
    with torch.no_grad():
        return paged_attn.mla_index_topk_ragged(logits.detach(), ks, ke, int(topk), slots, out)


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
