"""CPU: the MLA indexer's prefill logits (ABI 2.16) - the 2.16 surface and every
refusal of fmha_mla_index_logits_ragged (fake aligned pointers: each case fails before a launch),
reported through fmha_last_error().
"""
import ctypes as C

import pytest

from xf_flash_attention_cutlass_amd import capi

SYM = "fmha_mla_index_logits_ragged"
FAKE = 0x10000


def test_surface_2_16():
    import xf_flash_attention_cutlass_amd as xfa
    from tests.test_abi import header_symbols
    assert SYM in header_symbols() and SYM in capi.EXPORTED and hasattr(capi.lib(), SYM)
    ver = capi.lib().fmha_version().decode().split()[1]
    assert tuple(int(x) for x in ver.split(".")) >= (2, 16)
    assert len(getattr(capi.lib(), SYM).argtypes) == 15
    assert xfa.paged_attn.mla_index_logits_ragged is xfa.paged_attn._mla_index_logits_ragged
    assert "mla_index_logits_ragged" not in dir(xfa.paged_attn)
    assert "mla_index_logits_ragged" in xfa.__all__ and callable(xfa.mla_index_logits_ragged)
    assert xfa.paged_attn._mla_index_ragged_chunk % 128 == 0 and xfa.paged_attn._mla_index_ragged_rows == 16


def _ragged(q=FAKE, w=FAKE + (1 << 26), k=FAKE + (1 << 30), scale=FAKE + (1 << 28), ks=FAKE + (1 << 27),
            ke=FAKE + (1 << 25), out=FAKE + (1 << 29), m=0, n=1057, heads=64, d=128, strides=(64 * 128, 128),
            k_row=128, row=1101):
    L = capi.lib()
    st = None if strides is None else (C.c_int64 * 2)(*strides)
    L.fmha_mla_index_logits_ragged(q, w, k, scale, ks, ke, out, m, n, heads, d, st, k_row, row, None)
    return L.fmha_last_status(), L.fmha_last_error().decode(), L.fmha_last_kernel().decode()


@pytest.mark.parametrize("over,needle", [
    (dict(q=None), "non-null"), (dict(w=None), "non-null"), (dict(k=None), "non-null"), (dict(scale=None), "non-null"),
    (dict(ks=None), "non-null"), (dict(ke=None), "non-null"), (dict(out=None), "non-null"),
    (dict(strides=None), "q_strides must be a non-null"),
    (dict(heads=16), "32 or 64 heads"), (dict(heads=128), "32 or 64 heads"), (dict(d=64), "head_size 128"),
    (dict(m=-1), "non-negative"), (dict(n=-1), "non-negative"),
    (dict(m=2, strides=(-8192, 128)), "multiples of 16"), (dict(m=2, strides=(8200, 128)), "multiples of 16"),
    (dict(strides=(8192, 72)), "multiples of 16"), (dict(strides=(8192, -128)), "multiples of 16"),
    (dict(k_row=-128), "key row stride"), (dict(k_row=136), "key row stride"), (dict(k_row=112), "key row stride"),
    (dict(row=1056), "logits_row_stride"),
    (dict(q=FAKE + 8), "16-byte aligned"), (dict(k=FAKE + (1 << 30) + 8), "16-byte aligned"),
    (dict(w=FAKE + (1 << 26) + 2), "4-byte aligned"), (dict(scale=FAKE + (1 << 28) + 2), "4-byte aligned"),
    (dict(ks=FAKE + (1 << 27) + 2), "4-byte aligned"), (dict(ke=FAKE + (1 << 25) + 1), "4-byte aligned"),
    (dict(out=FAKE + (1 << 29) + 2), "4-byte aligned"),
    (dict(m=(1 << 31) - 1, n=(1 << 31) - 1, row=1 << 31), "more than one launch covers"),
])
def test_refusals(over, needle):
    st, msg, kern = _ragged(**over)
    assert st != 0 and needle in msg and kern == "", (msg, kern)
    assert _ragged() == (0, "", "")                           # no rows: validated, unlaunched, fine
    assert _ragged(m=5, n=0, row=0) == (0, "", "")            # no keys: likewise
