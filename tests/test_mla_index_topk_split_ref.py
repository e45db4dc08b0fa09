"""CPU: the MLA indexer's selection with rows split over workgroups (ABI 2.18) -
the 2.18 surface, the scratch size, and every refusal of the C entry that needs no device (fake
aligned pointers: each case fails before a launch), reported through fmha_last_error().
"""
import inspect

import pytest

import xf_flash_attention_cutlass_amd as xfa
from xf_flash_attention_cutlass_amd import capi

FAKE = 0x10000


def test_surface_2_18():
    from tests.test_abi import header_symbols
    for sym in ("fmha_mla_index_topk_split", "fmha_mla_index_topk_split_workspace_size"):
        assert sym in header_symbols() and sym in capi.EXPORTED and hasattr(capi.lib(), sym)
    ver = capi.lib().fmha_version().decode().split()[1]
    assert tuple(int(x) for x in ver.split(".")) >= (2, 18)
    assert xfa.paged_attn.mla_index_topk_split is xfa.paged_attn._mla_index_topk_split
    assert "mla_index_topk_split" not in dir(xfa.paged_attn)
    sig = inspect.signature(xfa.mla_index_topk)
    assert sig.parameters["splits"].default is None
    # the automatic choice: rows the one-workgroup kernel keeps in LDS stay there; the entry's limits hold
    auto = xfa.interface.mla_index_topk_splits
    assert [auto(k, 2048, r) for k in (0, 1061, 32768) for r in (1, 512)] == [1] * 6
    for k, topk in ((32769, 2048), (40003, 64), (131072, 2048), (1 << 20, 1), (1 << 20, 4096), (40000, 32768)):
        for rows in (1, 8, 64, 4096):
            s = auto(k, topk, rows)
            assert s == 1 or (2 <= s <= 16 and s * topk <= 32768 and (-(-k // s) + 3) // 4 * 4 <= 32768), (k, topk, s)
    assert (auto(131072, 2048, 8), auto(131072, 2048, 64), auto(65536, 2048, 8), auto(40003, 64, 30)) == (8, 4, 4, 3)


@pytest.mark.parametrize("rows,topk,splits", [(1, 1, 2), (8, 2048, 8), (3, 7, 5), (1 << 20, 2048, 16)])
def test_workspace_size(rows, topk, splits):
    want = rows * splits * (8 * topk + 4)
    assert capi.lib().fmha_mla_index_topk_split_workspace_size(rows, topk, splits) == (want + 15) // 16 * 16


def _split(logits=FAKE, row=70000, table=FAKE + (1 << 27), bt=1100, lens=FAKE + (1 << 25), out=FAKE + (1 << 29),
           orow=2048, topk=2048, sq=1, max_k=65536, batch=0, blocks=64, page=64, splits=4, ws=FAKE + (1 << 30),
           ws_bytes=1 << 30):
    L = capi.lib()
    L.fmha_mla_index_topk_split(logits, row, table, bt, lens, out, orow, topk, sq, max_k, batch, blocks, page, splits,
                                ws, ws_bytes, None)
    return L.fmha_last_status(), L.fmha_last_error().decode(), L.fmha_last_kernel().decode()


@pytest.mark.parametrize("over,needle", [
    (dict(splits=1), "splits must lie in [2, 16]"), (dict(splits=17), "splits must lie in [2, 16]"),
    (dict(splits=0), "splits must lie in [2, 16]"),
    (dict(splits=16, topk=2049, orow=2049), "splits * topk must be at most 32768"),
    (dict(splits=2, max_k=65537), "more than 32768"),                # L = 32772
    (dict(batch=2, ws_bytes=2 * 4 * (8 * 2048 + 4) - 1), "workspace too small"),
    (dict(ws=FAKE + (1 << 30) + 8), "16-byte aligned"),
    # ... and what fmha_mla_index_topk refuses, in its words
    (dict(logits=None), "non-null"), (dict(out=None), "non-null"), (dict(table=None), "non-null"),
    (dict(lens=None), "non-null"),
    (dict(topk=0), "topk must be at least 1"), (dict(sq=0), "seqlen_q must be at least 1"),
    (dict(batch=-1), "non-negative"),
    (dict(page=24), "positive multiple of 16"), (dict(blocks=0), "num_blocks must be at least 1"),
    (dict(max_k=-1), "max_seqlen_k must lie in"), (dict(max_k=1100 * 64 + 1, row=80000), "max_seqlen_k must lie in"),
    (dict(row=65535), "logits_row_stride"), (dict(orow=2047), "indices_row_stride"),
    (dict(logits=FAKE + 2), "4-byte aligned"), (dict(out=FAKE + (1 << 29) + 1), "4-byte aligned"),
    (dict(batch=1 << 30, sq=4), "more than one launch covers"),
])
def test_split_refusals(over, needle):
    st, msg, kern = _split(**over)
    assert st != 0 and needle in msg and kern == "", (msg, kern)
    assert _split() == (0, "", "")                            # batch 0: validated, unlaunched, fine
    assert _split(ws=None, ws_bytes=0) == (0, "", "")         # ... with the pool's scratch too
