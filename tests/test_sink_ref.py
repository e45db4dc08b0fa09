"""CPU: the attention-sink reference (tests/sink_ref.py) agrees with the post-hoc identity and
the dsink formula of DESIGN.md §3.8 in float64, and the 2.7 entries are exported, bound and
validate on the host (no kernel is launched here: every call fails a check before any launch)."""
import ctypes

import pytest
import torch

from oracle import attention_ref as orc
from tests import sink_ref as sr
from xf_flash_attention_cutlass_amd import capi

NEW = ("fmha_fwd_sink", "fmha_varlen_fwd_sink", "fmha_page_kvcache_fwd_sink", "fmha_bwd_sink")
MASKS = [dict(causal=True), dict(window=(4, 0))]


def _problem(seed=0):
    g = torch.Generator().manual_seed(seed)
    b, s, h, hk, d = 2, 130, 4, 2, 32
    q = torch.randn(b, s, h, d, generator=g, dtype=torch.float64)
    k = torch.randn(b, s, hk, d, generator=g, dtype=torch.float64)
    v = torch.randn(b, s, hk, d, generator=g, dtype=torch.float64)
    return q, k, v, sr.sink_values(h, torch.float64)


@pytest.mark.parametrize("mask", MASKS, ids=["causal", "window4_0"])
def test_explicit_form_equals_posthoc_identity(mask):
    q, k, v, sink = _problem()
    o, lse = sr.sink_attention(q, k, v, sink, **mask)
    # the sink-free result from the oracle itself (float64: upcast=False keeps the dtype)
    o0, _ = orc.attention_ref(q, k, v, upcast=False, **{("window_size" if n == "window" else n): x
                                                        for n, x in mask.items()})
    _, l0 = sr.sink_attention(q, k, v, None, **mask)
    o_id, lse_id = sr.posthoc(o0, l0, sink)
    assert (o - o_id).abs().max().item() <= 1e-12
    assert torch.equal(torch.isinf(lse), torch.isinf(lse_id))
    fin = torch.isfinite(lse)
    assert (lse[fin] - lse_id[fin]).abs().max().item() <= 1e-12
    # the -inf head is the sink-free head, the +20 head is nearly all sink
    assert torch.equal(o[:, :, 2], o0[:, :, 2])
    assert o[:, :, 1].abs().max().item() < 1e-5 * o0[:, :, 1].abs().max().item() + 1e-6


@pytest.mark.parametrize("mask", MASKS, ids=["causal", "window4_0"])
def test_autograd_dsink_equals_formula(mask):
    q, k, v, sink = _problem(1)
    sink = sink.clone().requires_grad_(True)
    o, lse = sr.sink_attention(q, k, v, sink, **mask)
    g = torch.randn(o.shape, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    (dsink,) = torch.autograd.grad(o, sink, g)
    want = sr.dsink_formula(sink.detach(), lse.detach(), g, o.detach())
    assert (dsink - want).abs().max().item() <= 1e-10
    assert dsink[2].item() == 0.0                      # the -inf head


def test_empty_rows_keep_the_convention():
    q, k, v, sink = _problem(3)
    # causal with more queries than keys: the first rows see no key
    o, lse = sr.sink_attention(q, k[:, :100], v[:, :100], sink, causal=True)
    assert torch.equal(o[:, :30], torch.zeros_like(o[:, :30]))
    assert bool((lse[:, :, :30] == float("inf")).all()) and bool(torch.isfinite(lse[:, :, 30:]).all())


# ---------------------------------------------------------------- the C ABI ---------------
def test_entries_are_exported_and_versioned():
    for name in NEW:
        assert name in capi.EXPORTED
        assert hasattr(capi.lib(), name)
    ver = capi.lib().fmha_version().decode().split()[1]
    assert tuple(int(x) for x in ver.split(".")) >= (2, 7)


def test_pybind_and_python_surface():
    import inspect
    import xf_flash_attention_cutlass_amd as xfa
    for op in ("fwd_sink", "varlen_fwd_sink", "fwd_kvcache_sink", "sink_bwd"):
        assert hasattr(xfa.paged_attn, op)
    for fn in (xfa.flash_attn_func, xfa.flash_attn_varlen_func, xfa.flash_attn_with_kvcache,
               xfa.flash_attn_kvpacked_func, xfa.flash_attn_varlen_kvpacked_func):
        par = inspect.signature(fn).parameters["sink"]
        assert par.kind is inspect.Parameter.KEYWORD_ONLY and par.default is None


def _result():
    L = capi.lib()
    return L.fmha_last_status(), L.fmha_last_error().decode(), L.fmha_last_kernel().decode()


def _dense(**over):
    a = dict(q=16, k=16, v=16, o=16, alibi=None, lse=None, sq=16, sk=16, b=1, h=4, hk=2, d=64,
             strides=(ctypes.c_int64 * 12)(*([16 * 4 * 64, 4 * 64, 64, 16 * 2 * 64, 2 * 64, 64] * 2)),
             scale=0.125, wl=-1, wr=-1, softcap=0.0, fp16=False, splits=1, stream=None, p=0.0,
             s_dmask=None, sink=16)
    a.update(over)
    capi.lib().fmha_fwd_sink(*a.values())
    return _result()


def _varlen(**over):
    a = dict(q=16, k=16, v=16, o=16, lse=None, cu_q=16, cu_k=16, seqused=None, bt=None, bts=0,
             page=0, alibi=None, abs=0, max_q=16, max_k=16, total_q=32, b=2, h=4, hk=2, d=64,
             scale=0.125, wl=-1, wr=-1, softcap=0.0, fp16=False, stream=None, p=0.0, s_dmask=None,
             sink=16)
    a.update(over)
    capi.lib().fmha_varlen_fwd_sink(*a.values())
    return _result()


def _paged(**over):
    a = dict(q=16, kc=16, vc=16, o=16, lse=None, bt=16, bts=4, seqlens=16, sq=1, max_k=64, b=2,
             h=4, hk=2, d=64, page=16, scale=0.125, wl=-1, wr=-1, softcap=0.0, alibi=None, abs=0,
             splits=0, kv_dtype=0, ks=1.0, vs=1.0, leftpad=None, fp16=False, stream=None, sink=16)
    a.update(over)
    capi.lib().fmha_page_kvcache_fwd_sink(*a.values())
    return _result()


@pytest.mark.parametrize("call", [_dense, _varlen, _paged])
def test_sink_with_alibi_is_refused(call):
    status, msg, kern = call(alibi=16)
    assert status != 0 and "sink" in msg and "ALiBi" in msg, msg
    assert kern == ""


@pytest.mark.parametrize("call", [_dense, _varlen])
@pytest.mark.parametrize("over", [dict(p=0.1), dict(s_dmask=16), dict(p=0.1, s_dmask=16, lse=16)])
def test_sink_with_dropout_is_refused(call, over):
    status, msg, kern = call(**over)
    assert status != 0 and "sink" in msg and "dropout" in msg, msg
    assert kern == ""


@pytest.mark.parametrize("call,later", [(_dense, dict(sk=0)), (_varlen, dict(max_k=0)),
                                        (_paged, dict(page=0))])
def test_null_sink_is_accepted(call, later):
    """sink = NULL is the base entry: what the sink check refuses passes it (ALiBi here), and the
    call goes on to the entry's later checks (one of which is made to fail, so that nothing is
    launched on the fake pointers)."""
    status, msg, kern = call(sink=None, alibi=16, **later)
    assert status != 0 and "sink" not in msg and kern == "", msg
    # ... and with a sink, the sink check comes first
    status, msg, kern = call(alibi=16, **later)
    assert status != 0 and "sink" in msg and kern == "", msg


def test_misaligned_sink_and_null_bwd_arguments():
    status, msg, _ = _dense(sink=18)
    assert status != 0 and "sink" in msg
    L = capi.lib()
    for args in ((None, 16, 16, 16), (16, None, 16, 16), (16, 16, None, 16), (16, 16, 16, None)):
        L.fmha_bwd_sink(*args, 2, 4, 16, 64, 16, None)
        assert L.fmha_last_status() != 0 and "non-null" in L.fmha_last_error().decode()
    L.fmha_bwd_sink(16, 16, 16, 16, 2, 4, 0, 0, 0, None)
    assert L.fmha_last_status() != 0 and "positive" in L.fmha_last_error().decode()


def test_python_wrappers_refuse_what_a_sink_does_not_support():
    import xf_flash_attention_cutlass_amd as xfa
    q = torch.zeros(1, 4, 4, 128, dtype=torch.bfloat16)
    kv = torch.zeros(1, 4, 2, 128, dtype=torch.bfloat16)
    sink = torch.zeros(4)
    cu = torch.tensor([0, 4], dtype=torch.int32)
    for kw in (dict(alibi_slopes=torch.ones(4)), dict(dropout_p=0.1)):
        with pytest.raises(NotImplementedError):
            xfa.flash_attn_func(q, kv, kv, sink=sink, **kw)
        with pytest.raises(NotImplementedError):
            xfa.flash_attn_varlen_func(q[0], kv[0], kv[0], cu, cu, 4, 4, sink=sink, **kw)
    q8, kv8 = q.to(torch.float8_e4m3fn), kv.to(torch.float8_e4m3fn)
    with pytest.raises(NotImplementedError):                   # as ALiBi there
        xfa.flash_attn_func(q8, kv8, kv8, sink=sink)
    with pytest.raises(NotImplementedError):
        xfa.flash_attn_varlen_func(q8[0], kv8[0], kv8[0], cu, cu, 4, 4, sink=sink)
    with pytest.raises(NotImplementedError):
        xfa.flash_attn_with_kvcache(q[:, :1], kv, kv, cache_seqlens=4, sink=sink,
                                    alibi_slopes=torch.ones(4))
    with pytest.raises(ValueError):                            # one logit per query head
        xfa.flash_attn_func(q, kv, kv, sink=torch.zeros(2))
