"""CPU: the surface of fmha_mla_sparse_fwd_fp8 (ABI 2.20) and the refusals that
need no device (fake aligned pointers: nothing can be written, nothing is launched)."""
import ctypes as C

from xf_flash_attention_cutlass_amd import capi

FAKE = 0x10000


def test_surface_and_host_refusals():
    import xf_flash_attention_cutlass_amd as xfa
    from tests.test_abi import header_symbols
    sym, L = "fmha_mla_sparse_fwd_fp8", capi.lib()
    assert sym in header_symbols() and sym in capi.EXPORTED and hasattr(L, sym)
    assert tuple(int(x) for x in L.fmha_version().decode().split()[1].split(".")) >= (2, 20)
    assert "mla_sparse_fwd_fp8" not in dir(xfa.paged_attn)
    assert xfa.paged_attn.mla_sparse_fwd_fp8 is xfa.paged_attn._mla_sparse_fwd_fp8
    assert "656" in xfa.flash_mla_sparse_fwd.__doc__
    st = (C.c_int64 * 4)(16 * 576, 576, 16 * 512, 512)
    for over, needle in ((dict(q=None), "q, kv and o must be non-null"),
                         (dict(kv_row=664), "at least 656 and a multiple of 16 bytes"),
                         (dict(kv_row=640), "at least 656 and a multiple of 16 bytes"),
                         (dict(s_kv=0), "s_kv must be at least 1")):
        a = dict(q=FAKE, kv_row=656, s_kv=1024)
        a.update(over)
        L.fmha_mla_sparse_fwd_fp8(a["q"], FAKE + (1 << 30), FAKE + (1 << 29), None, None, FAKE + (1 << 27), 64, 64, 3,
                                  a["s_kv"], 16, 576, 512, a["kv_row"], st, 576 ** -0.5, False, None)
        assert L.fmha_last_status() != 0 and needle in L.fmha_last_error().decode(), L.fmha_last_error()
        assert L.fmha_last_kernel().decode() == ""     # nothing was launched
