"""CPU: the 2.6 entries (fmha_quantize_fp8, fmha_fwd_fp8_ex, fmha_varlen_fwd_fp8_ex,
fmha_kvcache_append_fp8) are exported, bound and versioned, and their host-side validation
reports through fmha_last_error without launching.  No kernel is launched here."""
import ctypes

import pytest
import torch

from xf_flash_attention_cutlass_amd import capi

NEW = ("fmha_quantize_fp8", "fmha_fwd_fp8_ex", "fmha_varlen_fwd_fp8_ex", "fmha_kvcache_append_fp8")


def test_entries_are_exported_and_versioned():
    for name in NEW:
        assert name in capi.EXPORTED
        assert hasattr(capi.lib(), name)
    ver = capi.lib().fmha_version().decode().split()[1]
    assert tuple(int(x) for x in ver.split(".")) >= (2, 6)


def test_pybind_and_package_surface():
    import xf_flash_attention_cutlass_amd as xfa
    for op in ("quantize_fp8", "fwd_fp8_ex", "varlen_fwd_fp8_ex", "kvcache_append_fp8"):
        assert hasattr(xfa.paged_attn, op)
    assert "quantize_fp8" in xfa.__all__ and callable(xfa.quantize_fp8)
    # the functions that were there keep working names
    for op in ("fwd_fp8", "varlen_fwd_fp8", "fwd_kvcache_fp8", "fwd_kvcache"):
        assert hasattr(xfa.paged_attn, op)


def _result():
    L = capi.lib()
    return L.fmha_last_status(), L.fmha_last_error().decode(), L.fmha_last_kernel().decode()


def _strides(*s):
    return (ctypes.c_int64 * 3)(*s)


def _quant(**over):
    a = dict(x=16, x8=16, descale=16, cu=None, b=2, s=16, h=4, group=2, d=128,
             strides=_strides(16 * 4 * 128, 4 * 128, 128), gran=1, fp16=False, stream=None)
    a.update(over)
    capi.lib().fmha_quantize_fp8(*a.values())
    return _result()


@pytest.mark.parametrize("over,needle", [
    (dict(x=None), "non-null"),
    (dict(x8=None), "non-null"),
    (dict(descale=None), "non-null"),
    (dict(strides=None), "non-null"),
    (dict(d=60), "multiple of 8"),
    (dict(d=264), "multiple of 8"),
    (dict(group=3), "must divide"),
    (dict(group=0), "must divide"),
    (dict(gran=2), "granularity"),
    (dict(gran=-1), "granularity"),
    (dict(s=1 << 20, h=4096, group=1, strides=_strides(0, 4096 * 128, 128)), "supports <"),
])
def test_quantize_validation_errors(over, needle):
    status, msg, kern = _quant(**over)
    assert status != 0 and needle in msg, msg
    assert kern == ""                      # nothing was launched


def _fwd_ex(**over):
    a = dict(q=16, k=16, v=16, o=16, lse=None, qd=16, kd=16, vd=16, dbs=2, dhs=1, sq=16, sk=16,
             b=2, h=4, hk=2, d=128, scale=128 ** -0.5, wl=-1, wr=-1, fp16=False, stream=None)
    a.update(over)
    capi.lib().fmha_fwd_fp8_ex(*a.values())
    return _result()


def _varlen_ex(**over):
    a = dict(q=16, k=16, v=16, o=16, lse=None, cu_q=16, cu_k=16, seqused=None, qd=16, kd=16, vd=16,
             dbs=2, dhs=1, max_q=16, max_k=16, total_q=32, b=2, h=4, hk=2, d=128,
             scale=128 ** -0.5, wl=-1, wr=-1, fp16=False, stream=None)
    a.update(over)
    capi.lib().fmha_varlen_fwd_fp8_ex(*a.values())
    return _result()


@pytest.mark.parametrize("call", [_fwd_ex, _varlen_ex])
@pytest.mark.parametrize("over,needle", [
    (dict(q=None), "non-null"),
    (dict(qd=None), "descale"),
    (dict(kd=None), "descale"),
    (dict(vd=None), "descale"),
    (dict(dbs=-1), "strides"),
    (dict(d=64), "128"),
    (dict(h=3, hk=2), "must divide"),
])
def test_fwd_fp8_ex_validation_errors(call, over, needle):
    status, msg, kern = call(**over)
    assert status != 0 and needle in msg, msg
    assert kern == ""


def test_fwd_fp8_ex_slab_rule():
    status, msg, kern = _fwd_ex(sq=1 << 20, h=4096, hk=4096)
    assert status != 0 and "32-bit offsets" in msg and kern == ""
    status, msg, kern = _varlen_ex(max_q=1 << 20, h=4096, hk=4096)
    assert status != 0 and "32-bit offsets" in msg and kern == ""


def _append(**over):
    a = dict(q=16, q_out=16, kc=16, vc=16, kn=16, vn=16, snew=1, bt=16, bts=4, page=16, seq=16,
             seq_out=32, cos=None, sin=None, rdim=0, inter=False, per_tok=False, b=2, sq=1, h=4,
             hk=2, d=128, fp16=False, stream=None, ks=0.5, vs=0.5)
    a.update(over)
    capi.lib().fmha_kvcache_append_fp8(*a.values())
    return _result()


@pytest.mark.parametrize("over,needle", [
    (dict(ks=0.0), "descales must be positive"),
    (dict(vs=-1.0), "descales must be positive"),
    (dict(ks=float("nan")), "descales must be positive"),
    (dict(kc=None), "kcache"),
    (dict(kn=None), "new K and V"),
    (dict(seq_out=16), "alias"),
    (dict(d=60), "multiple of 8"),
    (dict(rdim=24, cos=16, sin=16), "rotary"),
    (dict(h=3), "head counts"),
])
def test_append_fp8_validation_errors(over, needle):
    status, msg, kern = _append(**over)
    assert status != 0 and needle in msg, msg
    assert kern == ""


def test_python_wrappers_refuse_bad_arguments():
    import xf_flash_attention_cutlass_amd as xfa
    x = torch.zeros(1, 4, 2, 128, dtype=torch.bfloat16)
    with pytest.raises(ValueError):
        xfa.quantize_fp8(x, granularity="row")
    with pytest.raises(ValueError):
        xfa.flash_attn_fp8_func(x, x, x, quantize="row")
    with pytest.raises(ValueError):                       # quantize= computes the descales
        xfa.flash_attn_fp8_func(x, x, x, q_descale=1.0, quantize="tensor")
    with pytest.raises(TypeError):                        # quantize= is for bf16 / fp16 inputs
        x8 = x.to(torch.float8_e4m3fn)
        xfa.flash_attn_fp8_func(x8, x8, x8, quantize="tensor")
    kc = torch.zeros(2, 16, 2, 128).to(torch.float8_e4m3fn)
    q = torch.zeros(1, 1, 4, 128, dtype=torch.bfloat16)
    bt = torch.zeros(1, 2, dtype=torch.int32)
    for kw in (dict(alibi_slopes=torch.ones(4)), dict(softcap=30.0)):   # stay refused
        with pytest.raises(NotImplementedError):
            xfa.flash_attn_with_kvcache(q, kc, kc, k=q[:, :, :2], v=q[:, :, :2], cache_seqlens=1,
                                        block_table=bt, **kw)
