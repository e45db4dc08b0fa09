"""CPU: the merge of partial attention states in float64, the 2.8 surface, and the
refusals of fmha_merge_states that need no device.

* attention over the full K/V equals `merge_ref` of the attention over 1, 2 and 3 K/V chunks;
* the gradients of the full problem equal the chunk-wise ones computed from the MERGED out and
  LSE (`bwd_from_lse`, the `bwd` contract): the claim that makes ring attention need no new
  backward kernel;
* fmha_merge_states is declared, exported and bound, the version is >= 2.8, and each refusal of
  the entry is reported through fmha_last_error (fake pointers: nothing is launched).
"""
import ctypes as C

import pytest
import torch

from tests import merge_ref as mr
from tests import sink_ref as sr
from xf_flash_attention_cutlass_amd import capi

TOL = 1e-12
INF = float("inf")


def _problem(b=2, sq=13, sk=29, h=4, hk=2, d=16, seed=0):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(b, sq, h, d, generator=g, dtype=torch.float64)
    k = torch.randn(b, sk, hk, d, generator=g, dtype=torch.float64)
    v = torch.randn(b, sk, hk, d, generator=g, dtype=torch.float64)
    return q, k, v


def _chunks(sk, cuts):
    edges = [0, *cuts, sk]
    return [slice(a, b) for a, b in zip(edges[:-1], edges[1:])]


def _chunk_parts(q, k, v, chunks, causal, softcap=0.0, off=None):
    """(out, lse) of q against each key chunk.  causal: row i sees keys j <= i + off of the FULL key
    range (off = sk - sq, the bottom-right alignment, by default), restricted to the chunk."""
    sq, sk = q.shape[1], k.shape[1]
    off = sk - sq if off is None else off
    scale = mr.default_scale(q)
    outs, lses = [], []
    for ch in chunks:
        s, _, _ = mr._masked_scores(q, k[:, ch], scale, False, softcap)
        if causal:
            i = torch.arange(sq).view(sq, 1)
            j = torch.arange(ch.start, ch.stop).view(1, -1)
            s = s.masked_fill(~(j <= i + off), -INF)
        l = torch.logsumexp(s, dim=-1)
        dead = torch.isneginf(l)
        p = torch.exp(s - torch.where(dead, torch.zeros_like(l), l).unsqueeze(-1))
        p = p.masked_fill(dead.unsqueeze(-1), 0.0)
        outs.append(torch.einsum("bhts,bshd->bthd", p, mr.orc.expand_kv(v[:, ch], q.shape[2])))
        lses.append(torch.where(dead, torch.full_like(l, INF), l))
    return outs, lses


def _assert_same(o, lse, ro, rl):
    assert torch.equal(torch.isinf(lse), torch.isinf(rl))
    fin = torch.isfinite(rl)
    assert (o - ro).abs().max().item() <= TOL
    assert (lse[fin] - rl[fin]).abs().max().item() <= TOL
    assert (o[~fin.permute(0, 2, 1)] == 0).all()


CUTS = {"one": (), "two_uneven": (5,), "three_uneven": (3, 20), "three_thin": (1, 2)}


@pytest.mark.parametrize("with_sink", [False, True])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("cuts", list(CUTS))
def test_merge_of_chunks_is_full_attention(cuts, causal, with_sink):
    # causal with sq = 13 > sk = 9: the first 4 rows see no key (all parts absent there), and
    # every chunk is absent for the rows before its first key's row
    q, k, v = _problem(sq=13, sk=9 if causal else 29)
    sk = k.shape[1]
    chunks = _chunks(sk, [c for c in CUTS[cuts] if c < sk])
    sink = sr.sink_values(q.shape[2], torch.float64) if with_sink else None
    outs, lses = _chunk_parts(q, k, v, chunks, causal)
    o, lse = mr.merge_ref(outs, lses, sink)
    _assert_same(o, lse, *sr.sink_attention(q, k, v, sink, causal=causal))


@pytest.mark.parametrize("with_sink", [False, True])
def test_chunk_no_row_sees(with_sink):
    """The queries are the FIRST 6 positions of a 14-key causal sequence (row i sees keys j <= i,
    the early query half of a zigzag shard): the chunks [6, 10) and [10, 14) are seen by no row,
    their LSE is +inf everywhere, and the merge is the attention over keys [0, 6)."""
    q, k, v = _problem(sq=6, sk=14)
    sink = sr.sink_values(q.shape[2], torch.float64) if with_sink else None
    outs, lses = _chunk_parts(q, k, v, _chunks(14, (2, 6, 10)), True, off=0)
    assert all(torch.isinf(l).all() for l in lses[2:]) and not torch.isinf(lses[0]).any()
    o, lse = mr.merge_ref(outs, lses, sink)
    _assert_same(o, lse, *sr.sink_attention(q, k[:, :6], v[:, :6], sink, causal=True))


def test_absent_parts_are_selected_away():
    """A part with LSE = +inf or -inf contributes nothing even when its O is NaN; no part present:
    O = 0 and LSE = +inf, whatever the sink."""
    q, k, v = _problem(sq=4, sk=12)
    outs, lses = _chunk_parts(q, k, v, _chunks(12, (6,)), False)
    ro, rl = mr.merge_ref(outs, lses)
    nan = torch.full_like(outs[0], float("nan"))
    for absent in (INF, -INF):
        o, lse = mr.merge_ref(outs + [nan], lses + [torch.full_like(lses[0], absent)])
        assert torch.equal(o, ro) and torch.equal(lse, rl)
    o, lse = mr.merge_ref([nan, nan], [torch.full_like(lses[0], INF), torch.full_like(lses[0], -INF)],
                          sr.sink_values(4, torch.float64))
    assert (o == 0).all() and (lse == INF).all()


def test_merge_packed_layout_and_gqa():
    q, k, v = _problem(b=1, sq=11, sk=17, h=6, hk=2)
    outs, lses = _chunk_parts(q, k, v, _chunks(17, (4, 9)), False)
    o, lse = mr.merge_ref([x[0] for x in outs], [x[0] for x in lses])          # [total, h, d], [h, total]
    ro, rl = sr.sink_attention(q, k, v, None)
    assert (o - ro[0]).abs().max().item() <= TOL and (lse - rl[0]).abs().max().item() <= TOL


@pytest.mark.parametrize("with_sink", [False, True])
@pytest.mark.parametrize("softcap", [0.0, 5.0])
@pytest.mark.parametrize("cuts", [(7,), (3, 20)])
def test_chunkwise_backward_from_merged_state(cuts, softcap, with_sink):
    """autograd of the full problem == sum over chunks of `bwd_from_lse` with the merged out / lse:
    dk / dv of a chunk exact, dq the sum of the chunks' shares, dsink from the merged LSE and D."""
    q, k, v = _problem(sk=29, seed=1)
    sink = sr.sink_values(q.shape[2], torch.float64) if with_sink else None
    g = torch.randn(q.shape, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    leaves = [x.clone().requires_grad_(True) for x in (q, k, v)] + \
        ([sink.clone().requires_grad_(True)] if with_sink else [])
    ro, _ = sr.sink_attention(leaves[0], leaves[1], leaves[2], leaves[3] if with_sink else None,
                              softcap=softcap)
    ref = torch.autograd.grad(ro, leaves, g)
    chunks = _chunks(29, cuts)
    scale = mr.default_scale(q)
    outs, lses = _chunk_parts(q, k, v, chunks, False, softcap)
    out, lse = mr.merge_ref(outs, lses, sink)
    dq, dk, dv = torch.zeros_like(q), torch.zeros_like(k), torch.zeros_like(v)
    for ch in chunks:
        a, b_, c, dsum = mr.bwd_from_lse(g, q, k[:, ch], v[:, ch], out, lse, scale, False, softcap)
        dq += a
        dk[:, ch], dv[:, ch] = b_, c
    for name, x, r in zip(("dq", "dk", "dv"), (dq, dk, dv), ref):
        assert (x - r).abs().max().item() <= 1e-11, name
    if with_sink:
        ds = mr.OracleOps.sink_bwd(lse, dsum, sink)
        fin = torch.isfinite(sink)
        assert (ds[fin] - ref[3][fin]).abs().max().item() <= 1e-11
        assert (ds[~fin] == 0).all()


# ------------------------------------------------------------------ surface ---------------
def test_surface_2_8():
    import xf_flash_attention_cutlass_amd as xfa
    from tests.test_abi import header_symbols
    assert "fmha_merge_states" in header_symbols()
    assert "fmha_merge_states" in capi.EXPORTED
    assert hasattr(capi.lib(), "fmha_merge_states")
    ver = capi.lib().fmha_version().decode().split()[1]
    assert tuple(int(x) for x in ver.split(".")) >= (2, 8)
    assert callable(xfa.paged_attn.merge_states)
    for name in ("merge_attn_states", "ring_attention", "zigzag_split", "zigzag_gather"):
        assert name in xfa.__all__ and callable(getattr(xfa, name)), name
    assert "FMHA_MERGE_MAX_PARTS 16" in open(header_symbols.__globals__["HEADER"]).read()


# ------------------------------------------------------------------ refusals --------------
FAKE = 0x10000         # 16-byte aligned, never dereferenced: every case fails before a launch


def _merge(n=2, parts=None, lparts=None, o=FAKE + (1 << 30), lse=FAKE + (3 << 29), batch=2, rows=5,
           heads=3, d=64, strides=None):
    L = capi.lib()
    step = 1 << 20
    parts = [FAKE + i * step for i in range(max(n, 0))] if parts is None else parts
    lparts = [FAKE + (1 << 29) + i * step for i in range(max(n, 0))] if lparts is None else lparts
    if strides is None:
        strides = [rows * heads * d, heads * d, d] * 2 + [heads * rows, rows] * 2
    op = (C.c_void_p * max(len(parts), 1))(*parts)
    lp = (C.c_void_p * max(len(lparts), 1))(*lparts)
    st = (C.c_int64 * 10)(*strides)
    L.fmha_merge_states(op, lp, n, o, lse, None, batch, rows, heads, d, st, False, None)
    return L.fmha_last_status(), L.fmha_last_error().decode()


def _strides(**over):
    rows, heads, d = 5, 3, 64
    s = [rows * heads * d, heads * d, d] * 2 + [heads * rows, rows] * 2
    for i, val in over.items():
        s[int(i[1:])] = val
    return s


@pytest.mark.parametrize("over,needle", [
    (dict(n=0), "num_parts must be in [1, 16]"),
    (dict(n=17), "num_parts must be in [1, 16]"),
    (dict(parts=[FAKE, None]), "part 1: o and lse must be non-null"),
    (dict(lparts=[None, FAKE + (1 << 29)]), "part 0: o and lse must be non-null"),
    (dict(o=None), "must be non-null"),
    (dict(d=60), "head_size must be a multiple of 8 and at most 256"),
    (dict(d=264), "head_size must be a multiple of 8 and at most 256"),
    (dict(heads=0), "num_heads positive"),
    (dict(rows=-1), "non-negative"),
    (dict(strides=_strides(s1=100)), "multiples of 8"),
    (dict(strides=_strides(s2=-64)), "non-negative"),
    (dict(strides=_strides(s4=0)), "the output's positive"),
    (dict(strides=_strides(s7=-1)), "LSE strides must be non-negative"),
    (dict(parts=[FAKE + 8, FAKE + (1 << 20)]), "16-byte aligned"),
    (dict(o=FAKE + (1 << 20)), "o overlaps part 1"),
    (dict(o=FAKE + 128), "o overlaps part 0"),
    (dict(o=FAKE, strides=_strides(s3=2 * 5 * 3 * 64)), "o overlaps part 0"),
    (dict(lse=FAKE + (1 << 29) + (1 << 20)), "lse overlaps part 1"),
    (dict(lse=FAKE + (1 << 29) + 4), "lse overlaps part 0"),
])
def test_merge_refusals(over, needle):
    st, msg = _merge(**over)
    assert st != 0 and needle in msg, msg


def test_merge_accepts_in_place_and_empty():
    """o / lse exactly part 0 pass validation (rows = 0: nothing is launched, so no pointer is
    read), and so does an empty problem."""
    for kw in (dict(o=FAKE, lse=FAKE + (1 << 29), rows=0), dict(rows=0), dict(batch=0), dict(lse=None, rows=0)):
        st, msg = _merge(**kw)
        assert st == 0 and msg == "", (kw, msg)


def test_merge_attn_states_python_refusals():
    import xf_flash_attention_cutlass_amd as xfa
    with pytest.raises(ValueError, match="at least one part"):
        xfa.merge_attn_states([], [])
    o = torch.zeros(1, 2, 2, 8, dtype=torch.bfloat16)
    l = torch.zeros(1, 2, 2)
    with pytest.raises(RuntimeError, match="1 to 16 parts"):
        xfa.merge_attn_states([o] * 17, [l] * 17)
    with pytest.raises(RuntimeError, match="same length"):
        xfa.merge_attn_states([o] * 2, [l] * 3)
    with pytest.raises(RuntimeError, match="fp16 or bf16"):
        xfa.merge_attn_states([o.float()], [l])
    with pytest.raises(RuntimeError, match="share one shape"):
        xfa.merge_attn_states([o, o[:, :1]], [l, l])
    with pytest.raises(ValueError, match="sink must have shape"):
        xfa.merge_attn_states([o], [l], sink=torch.zeros(3))
    assert "Not differentiable" in xfa.merge_attn_states.__doc__
