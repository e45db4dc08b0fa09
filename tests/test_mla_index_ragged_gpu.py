"""GPU: the MLA indexer's prefill logits (ABI 2.16) - fmha_mla_index_logits_ragged
against a float64 reference restated from the header's definition, over every row family of the
contract on poisoned, strided buffers; the cache-view route to k8 / k_scale; a captured graph.
"""
import pytest
import torch

import xf_flash_attention_cutlass_amd as xfa
from tests import mla_index_util as iu
from xf_flash_attention_cutlass_amd import capi

pytestmark = pytest.mark.gpu
DEV = "cuda"
CHUNK = xfa.paged_attn._mla_index_ragged_chunk        # keys of one workgroup's item
ROWS = xfa.paged_attn._mla_index_ragged_rows          # ... and its query rows


def ragged_ref(q8, w, k8, scale, ks, ke):
    """float64 (logits, A) [M, N]: the header's definition; A = k_scale * sum_h |w| sum_d |q k|."""
    n = k8.shape[0]
    q, k = q8.view(iu.F8).double(), k8.view(iu.F8).double()
    s = torch.arange(n)[None, :]
    vis = (s >= ks.clamp(0, n)[:, None]) & (s < ke.clamp(0, n)[:, None])
    dot = torch.einsum("mhd,nd->mhn", q, k)
    val = scale.double()[None, :] * (w.double()[:, :, None] * dot.clamp(min=0)).sum(1)
    mag = scale.double()[None, :] * (w.double().abs()[:, :, None] * torch.einsum("mhd,nd->mhn", q.abs(), k.abs())).sum(1)
    return torch.where(vis, val, torch.full_like(val, iu.NEG_INF)), torch.where(vis, mag, torch.zeros_like(mag))


def check(got, ref, mag, heads, what):
    got = got.cpu().double()
    dead = ref == iu.NEG_INF
    assert torch.equal(got == iu.NEG_INF, dead) and not got.isnan().any()
    err = torch.where(dead, torch.zeros_like(ref), (got - ref).abs())
    bound = (128 + heads + 8) * 2.0 ** -23 * mag
    print(f"{what}: worst err / bound {(err / bound.clamp(min=1e-300)).max():.3f}, max err {err.max():.3e}")
    assert (err <= bound).all()


def ranges(n):
    """37 rows = two row blocks and a partial one over n = chunk + 33 keys.  Block 0: two packed
    sequences meeting inside it (rows 0..8 causal over keys [0, 200), rows 9..15 over keys from 333,
    no multiple of 32): disjoint ranges, a gap no row sees inside the block's union, and a union
    that misses the second chunk.  Block 1: the second sequence on, across the chunk boundary to
    the last, partial tile; ke <= ks; ks < 0; ke > n.  Block 2: causal from 0, short."""
    assert ROWS == 16 and n == CHUNK + 33
    ks, ke = torch.zeros(37, dtype=torch.int32), torch.zeros(37, dtype=torch.int32)
    for r in range(9):
        ks[r], ke[r] = 0, 192 + r
    for r in range(9, 16):
        ks[r], ke[r] = 333, 338 + (r - 9)
    for r in range(16, 32):
        ks[r], ke[r] = 333, n - 47 + 3 * (r - 16)
    ks[20], ke[20] = 500, 400
    ks[21], ke[21] = 700, 700
    ks[22], ke[22] = -7, 40
    ks[23], ke[23] = CHUNK - 24, n + 50
    for r in range(32, 37):
        ks[r], ke[r] = 0, r + 100
    assert int(ke[31]) == n - 2 and int(ke[:16].max()) < CHUNK and int(ke[32:].max()) < 200
    return ks, ke


@pytest.mark.parametrize("heads", [32, 64])
def test_logits_match_the_float64_reference(heads):
    gen = torch.Generator().manual_seed(heads)
    m, n = 37, CHUNK + 33
    ks, ke = ranges(n)
    b8, scale = iu.quantize_ref((torch.randn(n, 128, generator=gen) * (8.0 ** (torch.arange(n) % 3))[:, None]).bfloat16())
    seen = ((torch.arange(n)[None] >= ks[:, None]) & (torch.arange(n)[None] < ke[:, None])).any(0)
    assert not seen[200:333].any() and seen[:200].all() and seen[333:].all()
    b8[~seen], scale[~seen] = 0x7F, float("nan")          # NaN bytes, NaN scales where no row looks
    kwide = torch.full((n, 256), 0x7F, dtype=torch.uint8)
    kwide[:, 64:192] = b8
    qwide = torch.randn(m, heads + 8, 128, generator=gen).to(iu.F8).view(torch.uint8)
    w = torch.randn(m, heads, generator=gen) * heads ** -0.5
    assert (w > 0).any() and (w < 0).any()
    ref, mag = ragged_ref(qwide[:, 4:4 + heads], w, b8, scale, ks, ke)

    buf = torch.full((m + 1, n + 24), float("nan"), device=DEV)
    qd, kd = qwide.to(DEV)[:, 4:4 + heads], kwide.to(DEV)[:, 64:192]
    assert not qd.is_contiguous() and kd.stride(0) == 256
    got = xfa.mla_index_logits_ragged(qd, w.to(DEV), kd, scale.to(DEV), ks.to(DEV), ke.to(DEV), out=buf[:m, :n])
    torch.cuda.synchronize()
    kern = capi.lib().fmha_last_kernel().decode()
    assert kern.startswith("fmha_mla_index_ragged_kernel<%d>" % heads) and "grid=%dx1x1" % (3 * 2) in kern, kern
    assert got.data_ptr() == buf.data_ptr() and buf[:, n:].isnan().all() and buf[m].isnan().all()
    check(got, ref, mag, heads, f"heads {heads}")


def test_operands_are_views_of_a_one_block_index_cache():
    gen = torch.Generator().manual_seed(3)
    page, n, m, heads = 48, 45, 5, 64
    k = (torch.randn(n, 128, generator=gen) * (8.0 ** (torch.arange(n) % 3))[:, None]).bfloat16()
    cache = torch.zeros(1, xfa.mla_index_cache_block_bytes(page), dtype=torch.uint8, device=DEV)
    xfa.mla_index_cache_append_fp8(k.to(DEV), cache, torch.arange(n, device=DEV))
    k8, scale = cache[0, :n * 128].view(n, 128), cache[0, page * 128:].view(torch.float32)[:n]
    q8 = torch.randn(m, heads, 128, generator=gen).to(iu.F8)
    w = torch.randn(m, heads, generator=gen) / 8
    ks, ke = torch.zeros(m, dtype=torch.int32), (torch.arange(m) + n - m + 1).int()
    got = xfa.mla_index_logits_ragged(q8.to(DEV), w.to(DEV), k8, scale, ks.to(DEV), ke.to(DEV))
    b8, ds = iu.quantize_ref(k)
    check(got, *ragged_ref(q8.view(torch.uint8), w, b8, ds, ks, ke), heads, "cache views")


def test_graph_replay_over_changed_ranges():
    gen = torch.Generator().manual_seed(4)
    m, n, heads = 37, CHUNK + 33, 64
    q8 = torch.randn(m, heads, 128, generator=gen).to(iu.F8).to(DEV)
    k8 = torch.randn(n, 128, generator=gen).to(iu.F8).to(DEV)
    w, scale = (torch.randn(m, heads, generator=gen) / 8).to(DEV), (torch.rand(n, generator=gen) + 0.5).to(DEV)
    ks, ke = (x.to(DEV) for x in ranges(n))
    out = torch.full((m, n), float("nan"), device=DEV)
    xfa.mla_index_logits_ragged(q8, w, k8, scale, ks, ke, out=out)           # (warm-up outside the capture)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        xfa.mla_index_logits_ragged(q8, w, k8, scale, ks, ke, out=out)
    assert capi.lib().fmha_last_kernel().decode().startswith("fmha_mla_index_ragged_kernel<64>")
    for shift in (0, 5, -301):
        a, b = ranges(n)
        ks.copy_(a + shift)
        ke.copy_(b + 2 * shift)
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, xfa.mla_index_logits_ragged(q8, w, k8, scale, ks, ke))
