"""CPU: the MLA indexer's selection for prefill rows (ABI 2.17) - the 2.17 surface
and every refusal of fmha_mla_index_topk_ragged (fake aligned pointers: each case fails before a
launch), reported through fmha_last_error().
"""
import pytest

from xf_flash_attention_cutlass_amd import capi

FAKE = 0x10000
SYM = "fmha_mla_index_topk_ragged"


def test_surface_2_17():
    import xf_flash_attention_cutlass_amd as xfa
    from tests.test_abi import header_symbols
    assert SYM in header_symbols() and SYM in capi.EXPORTED and hasattr(capi.lib(), SYM)
    ver = capi.lib().fmha_version().decode().split()[1]
    assert tuple(int(x) for x in ver.split(".")) >= (2, 17)
    assert xfa.paged_attn.mla_index_topk_ragged is xfa.paged_attn._mla_index_topk_ragged
    assert "mla_index_topk_ragged" not in dir(xfa.paged_attn)
    assert "mla_index_topk_ragged" in xfa.__all__ and callable(xfa.mla_index_topk_ragged)
    assert xfa.paged_attn._mla_index_topk_ragged_stage == 2048


def _topk(logits=FAKE, row=1101, ks=FAKE + (1 << 25), ke=FAKE + (1 << 26), slots=FAKE + (1 << 27),
          out=FAKE + (1 << 29), orow=2048, topk=2048, rows=0, keys=1061):
    L = capi.lib()
    L.fmha_mla_index_topk_ragged(logits, row, ks, ke, slots, out, orow, topk, rows, keys, None)
    return L.fmha_last_status(), L.fmha_last_error().decode(), L.fmha_last_kernel().decode()


@pytest.mark.parametrize("over,needle", [
    (dict(logits=None), "non-null"), (dict(out=None), "non-null"), (dict(ks=None), "non-null"),
    (dict(ke=None), "non-null"),
    (dict(topk=0), "topk must be at least 1"), (dict(rows=-1), "non-negative"), (dict(keys=-1), "non-negative"),
    (dict(orow=2047), "indices_row_stride"),
    (dict(row=-1), "logits_row_stride"), (dict(row=1060, rows=2), "logits_row_stride"),
    (dict(logits=FAKE + 2), "4-byte aligned"), (dict(out=FAKE + (1 << 29) + 1), "4-byte aligned"),
    (dict(ks=FAKE + (1 << 25) + 2), "4-byte aligned"), (dict(ke=FAKE + (1 << 26) + 2), "4-byte aligned"),
    (dict(slots=FAKE + (1 << 27) + 4), "8-byte aligned"),
    (dict(rows=1 << 24), "more than one launch covers"),
])
def test_topk_ragged_refusals(over, needle):
    st, msg, kern = _topk(**over)
    assert st != 0 and needle in msg and kern == "", (msg, kern)
    assert _topk() == (0, "", "")                             # no rows: validated, unlaunched, fine
    assert _topk(slots=None, row=1060, keys=1061) == (0, "", "")   # ... as are no slots, and a short stride of no rows
