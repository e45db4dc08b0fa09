"""CPU: the MLA indexer's selection (ABI 2.15) - the 2.15 surface, every refusal
of the C entry that needs no device (fake aligned pointers: each case fails before a launch),
reported through fmha_last_error(), and the reference helper against the definition.
"""
import pytest
import torch

from tests import mla_index_topk_util as tu
from xf_flash_attention_cutlass_amd import capi

FAKE = 0x10000


def test_surface_2_15():
    import xf_flash_attention_cutlass_amd as xfa
    from tests.test_abi import header_symbols
    sym = "fmha_mla_index_topk"
    assert sym in header_symbols() and sym in capi.EXPORTED and hasattr(capi.lib(), sym)
    ver = capi.lib().fmha_version().decode().split()[1]
    assert tuple(int(x) for x in ver.split(".")) >= (2, 15)
    assert xfa.paged_attn.mla_index_topk is xfa.paged_attn._mla_index_topk
    assert "mla_index_topk" not in dir(xfa.paged_attn)
    assert "mla_index_topk" in xfa.__all__ and callable(xfa.mla_index_topk)
    assert xfa.paged_attn._mla_index_topk_stage == 32768


def _topk(logits=FAKE, row=1101, table=FAKE + (1 << 27), bt=20, lens=FAKE + (1 << 25), out=FAKE + (1 << 29),
          orow=2048, topk=2048, sq=1, max_k=1061, batch=0, blocks=64, page=64):
    L = capi.lib()
    L.fmha_mla_index_topk(logits, row, table, bt, lens, out, orow, topk, sq, max_k, batch, blocks, page, None)
    return L.fmha_last_status(), L.fmha_last_error().decode(), L.fmha_last_kernel().decode()


@pytest.mark.parametrize("over,needle", [
    (dict(logits=None), "non-null"), (dict(out=None), "non-null"), (dict(table=None), "non-null"),
    (dict(lens=None), "non-null"),
    (dict(topk=0), "topk must be at least 1"), (dict(sq=0), "seqlen_q must be at least 1"),
    (dict(batch=-1), "non-negative"),
    (dict(page=24), "positive multiple of 16"), (dict(page=0), "positive multiple of 16"),
    (dict(blocks=0), "num_blocks must be at least 1"),
    (dict(max_k=-1), "max_seqlen_k must lie in"), (dict(max_k=20 * 64 + 1, row=4096), "max_seqlen_k must lie in"),
    (dict(row=1060), "logits_row_stride"), (dict(orow=2047), "indices_row_stride"),
    (dict(logits=FAKE + 2), "4-byte aligned"), (dict(out=FAKE + (1 << 29) + 1), "4-byte aligned"),
    (dict(table=FAKE + (1 << 27) + 2), "4-byte aligned"), (dict(lens=FAKE + (1 << 25) + 2), "4-byte aligned"),
    (dict(batch=1 << 30, sq=4), "more than one launch covers"),
])
def test_topk_refusals(over, needle):
    st, msg, kern = _topk(**over)
    assert st != 0 and needle in msg and kern == "", (msg, kern)
    assert _topk() == (0, "", "")                             # batch 0: validated, unlaunched, fine


def test_reference_matches_the_definition():
    """topk_ref against brute force on tiny rows with ties, both zeros, NaN and -inf: pick the
    largest remaining value topk times, the lowest position among equals."""
    inf, nan = float("inf"), float("nan")
    logits = torch.tensor([[2.0, -inf, 2.0, nan, 0.0, -0.0, 2.0, inf, -1.0, 9.0],
                           [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0]])
    table, lens, page = torch.tensor([[2, 5, 0]], dtype=torch.int32), [9], 4
    for topk in (1, 3, 4, 6, 9):
        got = tu.topk_ref(logits, table, lens, topk, 2, page, 5)
        for r in range(2):
            left = {s: float(logits[r, s]) + 0.0 for s in range(9 - 2 + r + 1)
                    if logits[r, s] == logits[r, s] and logits[r, s] != -inf}
            want = []
            while left and len(want) < topk:
                best = max(left.values())
                want.append(min(s for s, v in left.items() if v == best))
                del left[want[-1]]
            slots = [int(table[0, s // page]) * page + s % page if table[0, s // page] < 5 else -1 for s in sorted(want)]
            assert got[r].tolist() == slots + [-1] * (topk - len(slots)), (topk, r)
    assert tu.topk_ref(logits, table, lens, 6, 2, page, 5)[0].tolist() == [8, 10, -1, -1, -1, -1]   # block 5 is outside
