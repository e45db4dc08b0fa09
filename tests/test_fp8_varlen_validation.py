"""CPU: host-side validation of the packed fp8 forward (fmha_varlen_fwd_fp8 reports through
fmha_last_error and launches nothing; the Python wrapper refuses what the fp8 forward lacks).
No kernel is launched here."""
import pytest
import torch

from xf_flash_attention_cutlass_amd import capi


def _call(**over):
    a = dict(q=16, k=16, v=16, o=16, lse=None, cu_q=16, cu_k=16, seqused=None, qs=1.0, ks=1.0,
             vs=1.0, max_q=16, max_k=16, total_q=32, b=2, h=4, hk=2, d=128, scale=128 ** -0.5,
             wl=-1, wr=-1, fp16=False, stream=None)
    a.update(over)
    L = capi.lib()
    L.fmha_varlen_fwd_fp8(*a.values())
    return L.fmha_last_status(), L.fmha_last_error().decode(), L.fmha_last_kernel().decode()


@pytest.mark.parametrize("over,needle", [
    (dict(cu_q=None), "cu_seqlens_q"),
    (dict(cu_k=None), "cu_seqlens_k"),
    (dict(q=None), "non-null"),
    (dict(d=64), "128"),
    (dict(ks=0.0), "descales"),
    (dict(vs=-1.0), "descales"),
    (dict(max_k=0), "max_seqlen_k"),
    (dict(max_q=0), "max_seqlen_q"),
    (dict(lse=16, total_q=0), "total_q"),
    (dict(h=3, hk=2), "must divide"),
    (dict(max_q=1 << 20, h=4096), "32-bit offsets"),
])
def test_varlen_fp8_validation_errors(over, needle):
    status, msg, kern = _call(**over)
    assert status != 0 and needle in msg, msg
    assert kern == ""                      # nothing was launched


def test_varlen_fp8_is_exported_and_versioned():
    assert "fmha_varlen_fwd_fp8" in capi.EXPORTED
    ver = capi.lib().fmha_version().decode().split()[1]
    assert tuple(int(x) for x in ver.split(".")) >= (2, 5)


def test_pybind_has_varlen_fwd_fp8():
    import xf_flash_attention_cutlass_amd as xfa
    assert hasattr(xfa.paged_attn, "varlen_fwd_fp8")
    assert "flash_attn_varlen_fp8_func" in xfa.__all__


def _fp8_inputs():
    q = torch.zeros(6, 4, 128).to(torch.float8_e4m3fn)
    k = torch.zeros(6, 2, 128).to(torch.float8_e4m3fn)
    cu = torch.tensor([0, 2, 6], dtype=torch.int32)
    return q, k, k.clone(), cu, cu, 4, 4


@pytest.mark.parametrize("kw", [
    dict(dropout_p=0.1),
    dict(softcap=30.0),
    dict(alibi_slopes=torch.ones(4)),
    dict(block_table=torch.zeros(2, 1, dtype=torch.int32)),
])
def test_varlen_func_refuses_unsupported_fp8_features(kw):
    import xf_flash_attention_cutlass_amd as xfa
    with pytest.raises(NotImplementedError):
        xfa.flash_attn_varlen_func(*_fp8_inputs(), **kw)


def test_varlen_fp8_func_refuses_requires_grad_and_bad_out_dtype():
    import xf_flash_attention_cutlass_amd as xfa

    class _Grad:
        """stands for a tensor that asks for a gradient (float8 tensors cannot)"""
        requires_grad = True
    q, k, v, cu_q, cu_k, mq, mk = _fp8_inputs()
    with pytest.raises(NotImplementedError):
        xfa.flash_attn_varlen_fp8_func(_Grad(), k, v, cu_q, cu_k, mq, mk)
    with pytest.raises(ValueError):
        xfa.flash_attn_varlen_fp8_func(q, k, v, cu_q, cu_k, mq, mk, out_dtype=torch.float32)
