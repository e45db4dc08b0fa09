"""GPU: one-defect calls for every op of the `paged_attn` module (the PyTorch binding), in the
style of tests/test_validation_table.py for the C ABI.  Each row takes an otherwise valid small
call, breaks one argument and pins RuntimeError plus a substring of the message.  Every row is
refused by the binding's own checks, before any attention kernel is launched; only single-defect
calls are pinned (which of two defects is reported first is not).

The TIGHTENED rows are inputs the binding used to read without a check (a q of too low a rank
through an unchecked sizes()[i]; cu_seqlens / seqlens_k pointers and a dout row width handed to
a kernel unexamined): they must be a clean RuntimeError."""
import pytest
import torch

pytestmark = pytest.mark.gpu

B, S, H, HK, D, PAGE, D8 = 2, 16, 4, 2, 64, 16, 128
BF, F16, F32, U8 = torch.bfloat16, torch.float16, torch.float32, torch.uint8


def _t(*shape, dtype=BF):
    return torch.zeros(*shape, dtype=dtype, device="cuda")


def _i32(*vals):
    return torch.tensor(vals, dtype=torch.int32, device="cuda")


def _strided(t):
    """t's values in a non-contiguous 1-D view (every second element of a longer tensor)"""
    return torch.stack([t, t], dim=-1).flatten()[::2]


def _cols(t):
    """t's values with a non-contiguous last dimension"""
    return torch.stack([t, t], dim=-1)[..., 0]


def _heads(t):
    """t's values in a head-sliced view: last dimension contiguous, the tensor not"""
    return torch.cat([t, t], dim=-2)[..., ::2, :]


# ---- a valid call of each op, as an ordered {argument: value}; the _sink ops take `sink` last
def _fwd(d=D, hk=HK, dtype=BF):
    return dict(q=_t(B, S, H, d, dtype=dtype), k=_t(B, S, hk, d, dtype=dtype), v=_t(B, S, hk, d, dtype=dtype),
                out=None, alibi=None, p=0.0, scale=0.125, causal=False, wl=-1, wr=-1, softcap=0.0,
                ret=False, gen=None)


def _varlen_fwd(d=D, hk=HK, dtype=BF, paged=False):
    kv = (lambda: _t(4, PAGE, hk, d, dtype=dtype)) if paged else (lambda: _t(B * S, hk, d, dtype=dtype))
    return dict(q=_t(B * S, H, d, dtype=dtype), k=kv(), v=kv(), out=None, cu_q=_i32(0, S, 2 * S),
                cu_k=_i32(0, S, 2 * S), seqused_k=None, block_table=_i32([0, 1], [2, 3]) if paged else None,
                alibi=None, max_q=S, max_k=S, p=0.0, scale=0.125, zero=False, causal=False, wl=-1, wr=-1,
                softcap=0.0, ret=False, gen=None)


def _kvcache(d=D, hk=HK, dtype=BF, paged=False, append=False, rotary=False, sq=1):
    cache = (lambda: _t(4, PAGE, hk, d, dtype=dtype)) if paged else (lambda: _t(B, 2 * PAGE, hk, d, dtype=dtype))
    new = (lambda: _t(B, sq, hk, d, dtype=dtype)) if append else (lambda: None)
    rot = (lambda: _t(2 * PAGE, 16, dtype=dtype)) if rotary else (lambda: None)
    return dict(q=_t(B, sq, H, d, dtype=dtype), kcache=cache(), vcache=cache(), k=new(), v=new(),
                seqlens_k=_i32(5, 7), cos=rot(), sin=rot(), cache_batch_idx=None,
                block_table=_i32([0, 1], [2, 3]) if paged else None, alibi=None, out=None, scale=0.125,
                causal=False, wl=-1, wr=-1, softcap=0.0, interleaved=False, num_splits=0, cache_leftpad=None)


def _bwd(d=D, hk=HK, dtype=BF):
    return dict(dout=_t(B, S, H, d, dtype=dtype), q=_t(B, S, H, d, dtype=dtype), k=_t(B, S, hk, d, dtype=dtype),
                v=_t(B, S, hk, d, dtype=dtype), out=_t(B, S, H, d, dtype=dtype), lse=_t(B, H, S, dtype=F32),
                dq=None, dk=None, dv=None, alibi=None, p=0.0, scale=0.125, causal=False, wl=-1, wr=-1,
                softcap=0.0, det=False, gen=None, rng=None)


def _varlen_bwd(d=D, hk=HK, dtype=BF):
    return dict(dout=_t(B * S, H, d, dtype=dtype), q=_t(B * S, H, d, dtype=dtype), k=_t(B * S, hk, d, dtype=dtype),
                v=_t(B * S, hk, d, dtype=dtype), out=_t(B * S, H, d, dtype=dtype), lse=_t(H, B * S, dtype=F32),
                dq=None, dk=None, dv=None, cu_q=_i32(0, S, 2 * S), cu_k=_i32(0, S, 2 * S), alibi=None,
                max_q=S, max_k=S, p=0.0, scale=0.125, zero=False, causal=False, wl=-1, wr=-1, softcap=0.0,
                det=False, gen=None, rng=None)


def _kvcache_fp8(d=D8, hk=HK):
    return dict(q=_t(B, 1, H, D8), kcache=_t(4, PAGE, hk, d, dtype=U8), vcache=_t(4, PAGE, hk, d, dtype=U8),
                seqlens_k=_i32(5, 7), block_table=_i32([0, 1], [2, 3]), k_scale=1.0, v_scale=1.0, scale=0.088,
                causal=False, wl=-1, wr=-1, num_splits=0)


def _descale(ex):
    return torch.ones(1, dtype=F32, device="cuda") if ex else 1.0


def _fwd_fp8(d=D8, hk=HK, ex=False):
    return dict(q=_t(B, S, H, d, dtype=U8), k=_t(B, S, hk, d, dtype=U8), v=_t(B, S, hk, d, dtype=U8), out=None,
                qs=_descale(ex), ks=_descale(ex), vs=_descale(ex), scale=0.088, causal=False, wl=-1, wr=-1,
                out_fp16=False)


def _varlen_fwd_fp8(d=D8, hk=HK, ex=False):
    return dict(q=_t(B * S, H, d, dtype=U8), k=_t(B * S, hk, d, dtype=U8), v=_t(B * S, hk, d, dtype=U8),
                out=None, cu_q=_i32(0, S, 2 * S), cu_k=_i32(0, S, 2 * S), seqused_k=None, max_q=S, max_k=S,
                qs=_descale(ex), ks=_descale(ex), vs=_descale(ex), scale=0.088, causal=False, wl=-1, wr=-1,
                out_fp16=False)


def _quantize(packed=False):
    return dict(x=_t(B * S, H, D) if packed else _t(B, S, H, D), granularity=1, group=2,
                cu_seqlens=_i32(0, S, 2 * S) if packed else None, max_seqlen=0)


def _append_fp8(hk=HK, rotary=False):
    rot = (lambda: _t(2 * PAGE, 16)) if rotary else (lambda: None)
    return dict(q=_t(B, 1, H, D8), kcache=_t(4, PAGE, hk, D8, dtype=U8), vcache=_t(4, PAGE, hk, D8, dtype=U8),
                kn=_t(B, 1, hk, D8), vn=_t(B, 1, hk, D8), seqlens_k=_i32(5, 7),
                block_table=_i32([0, 1], [2, 3]), cos=rot(), sin=rot(), k_scale=1.0, v_scale=1.0,
                interleaved=False, per_token=False)


def _sink_bwd(varlen=False):
    shape = (H, B * S) if varlen else (B, H, S)
    return dict(lse=_t(*shape, dtype=F32), softmax_d=_t(*shape, dtype=F32), sink=_t(H, dtype=F32), varlen=varlen)


def _with_sink(base):
    def make(**kw):
        a = base(**kw)
        a["sink"] = _t(H, dtype=F32)
        return a
    return make


OPS = {
    "fwd": _fwd, "fwd_sink": _with_sink(_fwd),
    "varlen_fwd": _varlen_fwd, "varlen_fwd_sink": _with_sink(_varlen_fwd),
    "fwd_kvcache": _kvcache, "fwd_kvcache_sink": _with_sink(_kvcache),
    "bwd": _bwd, "varlen_bwd": _varlen_bwd, "sink_bwd": _sink_bwd,
    "fwd_kvcache_fp8": _kvcache_fp8, "fwd_kvcache_fp8_sink": _with_sink(_kvcache_fp8),
    "fwd_fp8": _fwd_fp8, "fwd_fp8_ex": lambda **kw: _fwd_fp8(ex=True, **kw),
    "varlen_fwd_fp8": _varlen_fwd_fp8, "varlen_fwd_fp8_ex": lambda **kw: _varlen_fwd_fp8(ex=True, **kw),
    "quantize_fp8": _quantize, "kvcache_append_fp8": _append_fp8,
}


# ---- the defects: (the valid call's arguments) -> {argument: broken value}
def to(name, dtype):
    return lambda a: {name: a[name].to(dtype)}


def cpu(name):
    return lambda a: {name: a[name].cpu()}


def view(name, f):
    return lambda a: {name: f(a[name])}


def put(**kw):
    return lambda a: kw


def new(name, *shape, dtype=BF):
    return lambda a: {name: _t(*shape, dtype=dtype)}


def _qkv_checks(op):
    """the checks every bf16 / fp16 attention op makes on q, k, v (k, v: the caches of fwd_kvcache)"""
    k = "kcache" if op.startswith("fwd_kvcache") else "k"
    return [(op, dict(dtype=F32), put(), "fp16 and bf16"),
            (op, {}, to(k, F16), "query and key must have the same dtype"),
            (op, {}, cpu("q"), "q must be on CUDA"),
            (op, {}, view("q", _cols), "contiguous last dimension"),
            (op, dict(hk=3), put(), "must divide"),
            (op, dict(d=264), put(), "at most 256")]


def _dropout_checks(op, ret=True):
    rows = [(op, {}, put(p=1.0), "p_dropout must be in [0, 1)"),
            (op, {}, put(p=-0.1), "p_dropout must be in [0, 1)"),
            (op, {}, put(p=0.1, softcap=30.0), "Softcapping does not support dropout")]
    if ret:
        rows.append((op, {}, put(ret=True), "return_softmax is only supported when p_dropout > 0.0"))
    return rows


def _out_checks(op, shape, dtype_needle, strict=False):
    rows = [(op, {}, new("out", *shape, dtype=F16), dtype_needle),
            (op, {}, new("out", *shape[:-1], shape[-1] + 8), "out must have shape"),
            (op, {}, new("out", 1, *shape), "out must have shape"),
            (op, {}, lambda a: {"out": _t(*shape).cpu()}, " must be on ")]
    if strict:      # the fp8 ops refuse an `out` they cannot compute into
        rows.append((op, {}, lambda a: {"out": _heads(_t(*shape))}, "out must be contiguous"))
    else:           # the others copy back from a temporary, but want rows they can copy into
        rows.append((op, {}, lambda a: {"out": _cols(_t(*shape))}, "Output tensor must have contiguous last dimension"))
    return rows


def _batch_int32_checks(op, name, kw=None):
    """an optional int32 [batch] index tensor: dtype, device, contiguity, shape"""
    kw = kw or {}
    return [(op, kw, lambda a: {name: _i32(0, 1).long()}, "int32"),
            (op, kw, lambda a: {name: _i32(0, 1).cpu()}, " must be on "),
            (op, kw, lambda a: {name: _strided(_i32(0, 1))}, "must be contiguous"),
            (op, kw, lambda a: {name: _i32(0, 1, 2)}, "must have shape (batch_size)")]


def _block_table_checks(op, kw=None, last_dim=True):
    kw = kw or {}
    rows = [(op, kw, to("block_table", torch.int64), "int32"),
            (op, kw, cpu("block_table"), "block_table must be on CUDA"),
            (op, kw, lambda a: {"block_table": _i32([0, 1], [2, 3], [0, 1])}, "block_table must have shape")]
    if last_dim:    # (the fp8 ops take a contiguous copy instead)
        rows.append((op, kw, view("block_table", _cols), "block_table must have contiguous last dimension"))
    return rows


def _cu_checks(op):
    rows = []
    for name in ("cu_q", "cu_k"):
        full = "cu_seqlens_" + name[-1]
        rows += [(op, {}, to(name, torch.int64), full + " must have dtype int32"),
                 (op, {}, cpu(name), full + " must be on "),
                 (op, {}, view(name, _strided), full + " must be contiguous"),
                 (op, {}, lambda a, name=name: {name: _i32(0, S, 2 * S, 2 * S)}, "must have shape (batch_size + 1)")]
    return rows


def _sink_checks(op):
    return [(op, {}, to("sink", F16), "sink must have dtype fp32"),
            (op, {}, new("sink", H + 1, dtype=F32), "sink must have shape (num_heads)"),
            (op, {}, new("sink", 1, H, dtype=F32), "sink must have shape (num_heads)"),
            (op, {}, cpu("sink"), "sink must be on q's device"),
            (op, {}, view("sink", _strided), "must be contiguous")]


def _rotary_checks(op, d):
    kw = dict(rotary=True) if op == "kvcache_append_fp8" else dict(append=True, rotary=True)
    both = lambda *shape: (lambda a: {"cos": _t(*shape), "sin": _t(*shape)})      # noqa: E731
    return [(op, kw, put(sin=None), "If rotary cos is provided, rotary sin must also be provided"),
            (op, kw, both(2 * PAGE, 12), "Only rotary dimensions divisible by 16"),
            (op, kw, both(2 * PAGE, d // 2 + 8), "rotary_dim must be <= headdim"),
            (op, kw, both(PAGE, 16), "cos/sin seqlen must be at least the seqlen of KV cache"),
            (op, kw, new("sin", 2 * PAGE + 1, 16), "sin must have shape"),
            (op, kw, to("cos", F32), "rotary_cos/sin must have the same dtype as query"),
            (op, kw, to("sin", F16), "rotary_cos/sin must have the same dtype as query"),
            (op, kw, cpu("cos"), " must be on "),
            (op, kw, view("sin", _cols), "must be contiguous")]


ROWS = []
# ---- fwd / fwd_sink
for op in ("fwd", "fwd_sink"):
    ROWS += _qkv_checks(op) + _dropout_checks(op)
    ROWS += _out_checks(op, (B, S, H, D), "Output must have the same dtype as inputs")
    ROWS += [(op, {}, new("k", B + 1, S, HK, D), "k must have shape"),
             (op, {}, new("v", B, S + 1, HK, D), "v must have shape"),
             (op, {}, new("q", 0, S, H, D), "batch size must be pos"),
             (op, {}, new("q", S, H, D), "q must be (batch, seqlen, heads, head_size)"),
             (op, {}, new("alibi", H, dtype=F16), "ALiBi slopes must have dtype fp32"),
             (op, {}, new("alibi", H + 1, dtype=F32), "ALiBi slopes must have shape"),
             (op, {}, lambda a: {"alibi": _t(H, dtype=F32).cpu()}, " must be on ")]
ROWS += _sink_checks("fwd_sink")
# ---- varlen_fwd / varlen_fwd_sink
for op in ("varlen_fwd", "varlen_fwd_sink"):
    ROWS += _qkv_checks(op) + _dropout_checks(op) + _cu_checks(op)
    ROWS += _out_checks(op, (B * S, H, D), "Output must have the same dtype as inputs")
    ROWS += _batch_int32_checks(op, "seqused_k") + _block_table_checks(op, dict(paged=True))
    ROWS += [(op, dict(paged=True), put(p=0.1), "dropout over a paged K/V cache is not supported"),
             (op, {}, new("k", B * S, HK, D + 8), "k must have shape"),
             (op, {}, new("v", B * S + 1, HK, D), "v must have shape"),
             (op, dict(paged=True), new("v", 4, PAGE + 1, HK, D), "v must have shape"),
             (op, {}, new("alibi", B + 1, H, dtype=F32), "ALiBi slopes must have shape")]
ROWS += _sink_checks("varlen_fwd_sink")
# ---- fwd_kvcache / fwd_kvcache_sink
for op in ("fwd_kvcache", "fwd_kvcache_sink"):
    ROWS += _qkv_checks(op) + _out_checks(op, (B, 1, H, D), "Output must have the same dtype as inputs")
    ROWS += _batch_int32_checks(op, "seqlens_k") + _batch_int32_checks(op, "cache_leftpad")
    ROWS += _batch_int32_checks(op, "cache_batch_idx") + _block_table_checks(op, dict(paged=True))
    ROWS += _rotary_checks(op, D)
    ROWS += [(op, dict(paged=True), lambda a: {"cache_leftpad": _i32(0, 1)}, "leftpad"),
             (op, {}, lambda a: {"cache_leftpad": _i32(0, 1), "seqlens_k": None}, "cache_leftpad needs seqlens_k"),
             (op, dict(paged=True), lambda a: {"cache_batch_idx": _i32(0, 1)},
              "cache_batch_idx cannot be combined with a paged KV cache"),
             (op, {}, lambda a: {"kcache": _t(B + 1, 2 * PAGE, HK, D), "vcache": _t(B + 1, 2 * PAGE, HK, D)},
              "k_cache batch must equal q batch without cache_batch_idx"),
             (op, {}, new("vcache", B, 2 * PAGE + 1, HK, D), "vcache must have shape"),
             (op, dict(paged=True), new("vcache", 5, PAGE, HK, D), "vcache must have shape"),
             (op, dict(append=True), put(seqlens_k=None), "If key is supplied, seqlens_k must also be passed in"),
             (op, dict(append=True), put(v=None), "If key is supplied, value must also be passed in"),
             (op, dict(append=True), to("k", F16), "Key must have the same dtype as query"),
             (op, dict(append=True), to("v", F16), "Value must have the same dtype as query"),
             (op, dict(append=True), new("k", B, 2, HK, D), "must have shape"),
             (op, dict(append=True), new("v", B, 1, HK + 1, D), "vn must have shape"),
             (op, dict(append=True), view("k", _cols), "must be contiguous"),
             (op, dict(append=True, sq=2 * PAGE + 1), put(), "it must have seqlen <= the seqlen of the KV cache"),
             (op, dict(append=True, d=36), put(), "appending needs contiguous caches with head_size a multiple of 8"),
             (op, {}, lambda a: {"cos": _t(2 * PAGE, 16), "sin": _t(2 * PAGE, 16)},
              "new key / value to be appended to KV cache must also be provided"),
             (op, {}, new("alibi", H, dtype=F16), "ALiBi slopes must have dtype fp32")]
ROWS += _sink_checks("fwd_kvcache_sink")
# ---- bwd / varlen_bwd / sink_bwd
for op, lead in (("bwd", (B, S)), ("varlen_bwd", (B * S,))):
    ROWS += _qkv_checks(op) + _dropout_checks(op, ret=False)
    ROWS += [(op, {}, view("lse", lambda t: torch.cat([t, t], -1)), "softmax_lse must have shape"),
             (op, {}, new("out", *lead, H + 1, D), "out must have shape"),
             (op, {}, new("dout", lead[0] + 1, *lead[1:], H, D), "dout must have shape"),
             (op, {}, new("v", *lead, HK, D + 8), "v must have shape"),
             (op, dict(d=60), put(), "head_size should be a multiple of 8"),
             (op, {}, put(p=0.1), "backward with dropout needs the forward's rng_state"),
             (op, {}, lambda a: {"p": 0.1, "rng": _i32(1, 2)}, "rng_state must be int64 {seed, offset}"),
             (op, {}, new("alibi", H + 1, dtype=F32), "ALiBi slopes must have shape")]
    for g, like in (("dq", "q"), ("dk", "k"), ("dv", "v")):       # the gradient intake
        ROWS += [(op, {}, lambda a, g=g, like=like: {g: a[like].to(F16)}, "gradient must have the same dtype as its input"),
                 (op, {}, lambda a, g=g, like=like: {g: a[like][..., :-8].contiguous()}, "gradient has the wrong shape"),
                 (op, {}, lambda a, g=g, like=like: {g: a[like].cpu()}, " must be on ")]
ROWS += [("bwd", {}, to("dout", F16), "query and dout must have the same dtype"),
         ("bwd", {}, to("out", F16), "query and out must have the same dtype"),
         ("bwd", {}, new("q", 0, S, H, D), "batch size must be pos"),
         ("bwd", {}, new("dout", B, S, H, D - 16), "head_size must be head_size_og rounded to a multiple of 8"),
         ("varlen_bwd", {}, to("cu_q", torch.int64), "cu_seqlens_q must have dtype int32"),
         ("varlen_bwd", {}, to("cu_k", torch.int64), "cu_seqlens_k must have dtype int32")]
for kw in (dict(varlen=False), dict(varlen=True)):
    ROWS += [("sink_bwd", kw, to("lse", F16), "must be fp32"),
             ("sink_bwd", kw, to("sink", BF), "must be fp32"),
             ("sink_bwd", kw, cpu("softmax_d"), " must be on "),
             ("sink_bwd", kw, new("lse", 1, B, H, S, dtype=F32), "softmax_lse must be (batch, heads, seqlen_q)"),
             ("sink_bwd", kw, new("softmax_d", B, H, dtype=F32), "softmax_d must have softmax_lse's shape"),
             ("sink_bwd", kw, new("sink", H + 1, dtype=F32), "sink must have shape (num_heads)"),
             ("sink_bwd", kw, view("sink", _strided), "must be contiguous")]
# ---- fwd_kvcache_fp8 / _sink (seqlens_k's contiguity: a TIGHTENED row)
for op in ("fwd_kvcache_fp8", "fwd_kvcache_fp8_sink"):
    ROWS += [r for r in _batch_int32_checks(op, "seqlens_k") if r[3] != "must be contiguous"]
    ROWS += _block_table_checks(op, last_dim=False)
    ROWS += [(op, {}, to("q", F32), "q must be fp16 or bf16"),
             (op, {}, to("kcache", BF), "fp8 K/V cache expected"),
             (op, {}, cpu("vcache"), "vcache must be on CUDA"),
             (op, {}, view("kcache", _heads), "kcache must be contiguous"),
             (op, dict(d=64), put(), "head_size must be a multiple of 8 and <= 256"),
             (op, dict(hk=3), put(), "must divide")]
ROWS += _sink_checks("fwd_kvcache_fp8_sink")
# ---- fwd_fp8 / fwd_fp8_ex / varlen_fwd_fp8 / varlen_fwd_fp8_ex
for op, shape, rank_needle in (("fwd_fp8", (B, S, H, D8), "q, k, v must be [b, s, h, d]"),
                               ("fwd_fp8_ex", (B, S, H, D8), "q, k, v must be [b, s, h, d]"),
                               ("varlen_fwd_fp8", (B * S, H, D8), "q, k, v must be [total, h, d]"),
                               ("varlen_fwd_fp8_ex", (B * S, H, D8), "q, k, v must be [total, h, d]")):
    ROWS += _out_checks(op, shape, "out has the wrong dtype", strict=True)
    ROWS += [(op, {}, to("q", BF), "must be float8_e4m3fn (or uint8 bytes)"),
             (op, {}, cpu("k"), "k must be on CUDA"),
             (op, {}, view("v", _heads), "v must be contiguous"),
             (op, {}, view("q", lambda t: t[0]), rank_needle),
             (op, dict(d=64), put(), "fp8 forward supports head_size 128"),
             (op, dict(hk=3), put(), "must divide"),
             (op, {}, view("v", lambda t: torch.cat([t, t[:1]], 0)), "v must have shape")]
    if op.endswith("_ex"):
        ROWS += [(op, {}, to("qs", F16), "descales must have dtype float32"),
                 (op, {}, new("ks", 3, dtype=F32), "a descale must have one element or shape (batch_size, num_heads_k)"),
                 (op, {}, new("vs", B, HK + 1, dtype=F32), "a descale must have one element or shape (batch_size, num_heads_k)"),
                 (op, {}, cpu("vs"), "descales must be CUDA tensors on q's device")]
for op in ("varlen_fwd_fp8", "varlen_fwd_fp8_ex"):
    ROWS += _cu_checks(op) + _batch_int32_checks(op, "seqused_k")
    ROWS += [(op, {}, put(max_q=0), "max_seqlen_q and max_seqlen_k must be positive"),
             (op, {}, put(max_k=0), "max_seqlen_q and max_seqlen_k must be positive")]
# ---- quantize_fp8
packed = dict(packed=True)
ROWS += [("quantize_fp8", {}, to("x", F32), "quantize_fp8: x must be fp16 or bf16"),
         ("quantize_fp8", {}, cpu("x"), "x must be on CUDA"),
         ("quantize_fp8", {}, put(granularity=2), "granularity must be 0 (tensor) or 1 (head)"),
         ("quantize_fp8", {}, put(group=3), "group must divide the number of heads"),
         ("quantize_fp8", {}, put(group=0), "group must divide the number of heads"),
         ("quantize_fp8", {}, view("x", lambda t: t[0]), "x must be [b, s, h, d], or [total, h, d] with cu_seqlens"),
         ("quantize_fp8", packed, view("x", lambda t: t[None]), "x must be [b, s, h, d], or [total, h, d] with cu_seqlens"),
         ("quantize_fp8", packed, put(group=3), "group must divide the number of heads"),
         ("quantize_fp8", packed, to("cu_seqlens", torch.int64), "cu_seqlens must have dtype int32"),
         ("quantize_fp8", packed, cpu("cu_seqlens"), "cu_seqlens must be on "),
         ("quantize_fp8", packed, view("cu_seqlens", _strided), " must be contiguous"),
         ("quantize_fp8", packed, lambda a: {"cu_seqlens": _i32(0)}, "cu_seqlens must "),
         ("quantize_fp8", packed, lambda a: {"cu_seqlens": _i32([0, S], [S, 2 * S])}, "cu_seqlens must ")]
# ---- kvcache_append_fp8
op = "kvcache_append_fp8"
ROWS += _rotary_checks(op, D8) + _block_table_checks(op, last_dim=False) + _batch_int32_checks(op, "seqlens_k")
ROWS += [(op, {}, to("q", F32), "q must be fp16 or bf16"),
         (op, {}, to("kn", F16), "new key / value must have the same dtype as query"),
         (op, {}, to("vcache", BF), "fp8 K/V cache expected"),
         (op, {}, cpu("kn"), "kn must be on CUDA"),
         (op, {}, view("vcache", _heads), "vcache must be contiguous"),
         (op, {}, view("q", lambda t: t[0]), "q, k, v, caches must be 4-D and block_table 2-D"),
         (op, {}, lambda a: {"block_table": _i32(0, 1)}, "q, k, v, caches must be 4-D and block_table 2-D"),
         (op, {}, new("kcache", 4, PAGE, HK, 64, dtype=U8), "head_size must be a multiple of 8 and <= 256"),
         (op, dict(hk=3), put(), "must divide"),
         (op, {}, new("vcache", 5, PAGE, HK, D8, dtype=U8), "k_cache and v_cache must have the same shape"),
         (op, {}, new("kn", B, 2, HK, D8), "must have shape"),
         (op, {}, new("vn", B + 1, 1, HK, D8), "vn must have shape"),
         (op, {}, put(k_scale=0.0), "fp8 cache descales must be positive"),
         (op, {}, put(v_scale=-1.0), "fp8 cache descales must be positive"),
         (op, dict(rotary=True), new("cos", 2 * PAGE * 16), "rotary_cos must be [seqlen_ro, rotary_dim / 2]")]

# ---- inputs the binding used to read unchecked: now a clean RuntimeError
TIGHTENED = [
    ("varlen_fwd", {}, new("q", B * S, H * D), "q must be (total, heads, head_size)"),
    ("varlen_fwd_sink", {}, new("q", B * S, H * D), "q must be (total, heads, head_size)"),
    ("fwd_kvcache", {}, new("q", B, H * D), "q must be (batch, seqlen, heads, head_size)"),
    ("fwd_kvcache", {}, new("q", H * D), "q must be (batch, seqlen, heads, head_size)"),
    ("fwd_kvcache_sink", {}, new("q", B, H, D), "q must be (batch, seqlen, heads, head_size)"),
    ("bwd", {}, new("q", B * S, H, D), "q must be (batch, seqlen, heads, head_size)"),
    ("bwd", {}, new("q", D), "q must be (batch, seqlen, heads, head_size)"),
    ("varlen_bwd", {}, cpu("cu_q"), "cu_seqlens_q must be on CUDA"),
    ("varlen_bwd", {}, cpu("cu_k"), "cu_seqlens_k must be on CUDA"),
    ("varlen_bwd", {}, view("cu_q", _strided), "cu_seqlens_q must be contiguous"),
    ("varlen_bwd", {}, view("cu_k", _strided), "cu_seqlens_k must be contiguous"),
    ("varlen_bwd", {}, lambda a: {"cu_q": _i32(0, S, 2 * S, 2 * S)}, "must have shape (batch_size + 1)"),
    ("varlen_bwd", {}, lambda a: {"cu_k": _i32(0, S, 2 * S, 2 * S)}, "must have shape (batch_size + 1)"),
    ("varlen_bwd", {}, lambda a: {"cu_q": _i32([0, S, 2 * S])}, "must have shape (batch_size + 1)"),
    ("varlen_bwd", {}, new("dout", B * S, H, D - 16), "head_size must be head_size_og rounded to a multiple of 8"),
    ("fwd_kvcache_fp8", {}, view("seqlens_k", _strided), "seqlens_k must be contiguous"),
    ("fwd_kvcache_fp8_sink", {}, view("seqlens_k", _strided), "seqlens_k must be contiguous"),
]


def _refused(op, base_kw, defect):
    from xf_flash_attention_cutlass_amd import paged_attn
    a = OPS[op](**base_kw)
    over = defect(a)
    assert set(over) <= set(a), (op, sorted(over))
    a.update(over)
    with pytest.raises(RuntimeError) as e:
        getattr(paged_attn, op)(*a.values())
    assert type(e.value) is RuntimeError, type(e.value)      # not one of its subclasses
    return str(e.value)


@pytest.mark.parametrize("op,base_kw,defect,needle", ROWS, ids=[f"{r[0]}-{i}" for i, r in enumerate(ROWS)])
def test_one_defect_is_refused(op, base_kw, defect, needle):
    assert needle in _refused(op, base_kw, defect)


@pytest.mark.parametrize("op,base_kw,defect,needle", TIGHTENED,
                         ids=[f"{r[0]}-{i}" for i, r in enumerate(TIGHTENED)])
def test_tightened_unchecked_reads_are_refused(op, base_kw, defect, needle):
    assert needle in _refused(op, base_kw, defect)


@pytest.mark.parametrize("op", ["fwd", "varlen_fwd", "fwd_kvcache", "fwd_kvcache_fp8"])
def test_sink_is_positional_and_required(op):
    """the base op takes no sink (`fwd`: 13 arguments, a 14th is a TypeError); the _sink op
    requires it (`fwd_sink`: 14, not 13, and not None)"""
    from xf_flash_attention_cutlass_amd import paged_attn
    a = list(OPS[op + "_sink"]().values())
    assert op != "fwd" or len(a) == 14
    with pytest.raises(TypeError):
        getattr(paged_attn, op)(*a)
    with pytest.raises(TypeError):
        getattr(paged_attn, op + "_sink")(*a[:-1])
    with pytest.raises(TypeError):
        getattr(paged_attn, op + "_sink")(*a[:-1], None)


def test_every_op_has_rows():
    from xf_flash_attention_cutlass_amd import paged_attn
    ops = {n for n in dir(paged_attn) if not n.startswith("_") and n != "version"}
    assert ops == set(OPS) == {r[0] for r in ROWS}, sorted(ops ^ set(OPS))
