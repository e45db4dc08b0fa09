"""GPU: appending new K/V rows (+ rotary) into an fp8 e4m3fn paged cache
(fmha_kvcache_append_fp8) and the decode loop over it (flash_attn_with_kvcache with k=, v=).

Setup: page 16, b = 3, h = 4, hk = 2, a permuted block table of 3 pages per sequence,
cache_seqlens = [13, 30, 46], 5 new rows: they cross a page boundary in the first two sequences
and fall off the block table's row (positions >= 48, dropped) in the third.  The caches start as
0x55 bytes, so every byte the append must not touch is checked.

  no rotary   the written bytes are exactly e4m3(clamp(float(x) * (1 / scale), +-448)), every other
              byte is unchanged, seqlens_out = cache_seqlens + 5;
  rotary      K is rounded once from the fp32 rotary: |deq - x| <= 2^-4 |x| + 2^-10 k_scale +
              1e-6 |x| (e4m3: 3 mantissa bits -> half an ulp is 2^-4 relative, subnormal step
              2^-9 -> half of it 2^-10, in units of k_scale; the last term covers fp32 contraction
              differences); q_out is the bf16 rounding of its fp32 rotary (half an ulp, 2^-8 |x|).
"""
import math

import pytest
import torch

from oracle import attention_ref as orc

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAGE, B, H, HK, NEW = 16, 3, 4, 2, 5
SEQLENS = [13, 30, 46]
NPAGES = 11                   # 9 in the table, 2 that no sequence owns
KS, VS = 0.037, 0.051


@pytest.fixture(scope="module")
def xfa():
    import xf_flash_attention_cutlass_amd as m
    return m


def _table():
    perm = torch.randperm(NPAGES, generator=torch.Generator().manual_seed(3))[:9]
    return perm.to(torch.int32).view(B, 3)


def _inv(scale):
    return torch.tensor(1.0, dtype=torch.float32) / torch.tensor(scale, dtype=torch.float32)


def _to_bytes(x32, scale):
    """the entry's formula: fp32 value x (1 / scale), clamped, one rounding to e4m3"""
    return (x32 * _inv(scale)).clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)


def _expected(cache, table, rows, seqlens):
    """`cache` (uint8 [pages, PAGE, HK, d]) with rows[b, j] written at position seqlens[b] + j
    where the block table's row has that slot; returns the mask of written rows too"""
    cache = cache.clone()
    written = torch.zeros(cache.shape[:2], dtype=torch.bool)
    for b in range(B):
        for j in range(NEW):
            pos = seqlens[b] + j
            if pos // PAGE < table.shape[1]:
                pg = int(table[b, pos // PAGE])
                cache[pg, pos % PAGE] = rows[b, j]
                written[pg, pos % PAGE] = True
    return cache, written


def _inputs(d, amp, dtype=torch.bfloat16):
    g = torch.Generator().manual_seed(d)
    q = torch.randn(B, 1, H, d, generator=g).to(dtype)
    k = (torch.randn(B, NEW, HK, d, generator=g) * amp).to(dtype)
    v = (torch.randn(B, NEW, HK, d, generator=g) * amp).to(dtype)
    return q, k, v


def _append(xfa, q, k, v, table, cos=None, sin=None, interleaved=False, per_token=False):
    kc = torch.full((NPAGES, PAGE, HK, q.shape[-1]), 0x55, dtype=torch.uint8, device=DEV)
    vc = torch.full_like(kc, 0x55)
    seq = torch.tensor(SEQLENS, dtype=torch.int32, device=DEV)
    seq_out, q_out = xfa.paged_attn.kvcache_append_fp8(
        q.to(DEV), kc, vc, k.to(DEV), v.to(DEV), seq, table.to(DEV),
        None if cos is None else cos.to(DEV), None if sin is None else sin.to(DEV), KS, VS,
        interleaved, per_token)
    torch.cuda.synchronize()
    assert seq.cpu().tolist() == SEQLENS                      # the input lengths are left alone
    assert seq_out.cpu().tolist() == [s + NEW for s in SEQLENS]
    return kc.cpu(), vc.cpu(), q_out.cpu()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("d", [64, 128])
def test_append_bytes_exact(xfa, d, dtype):
    # amplitude 8: some values pass 448 x scale and are clamped
    q, k, v = _inputs(d, 8.0, dtype)
    assert float(k.float().abs().max()) > 448 * KS
    table = _table()
    kc, vc, q_out = _append(xfa, q, k, v, table)
    blank = torch.full((NPAGES, PAGE, HK, d), 0x55, dtype=torch.uint8)
    k_exp, written = _expected(blank, table, _to_bytes(k.float(), KS), SEQLENS)
    v_exp, _ = _expected(blank, table, _to_bytes(v.float(), VS), SEQLENS)
    assert int(written.sum()) == 5 + 5 + 2                    # three rows of the last sequence dropped
    assert torch.equal(kc, k_exp), f"{int((kc != k_exp).sum())} K bytes differ"
    assert torch.equal(vc, v_exp), f"{int((vc != v_exp).sum())} V bytes differ"
    assert torch.equal(q_out, q)                              # no rotary: q as given


@pytest.mark.parametrize("interleaved", [False, True])
@pytest.mark.parametrize("d", [64, 128])
def test_append_rotary(xfa, d, interleaved):
    rdim = 64
    q, k, v = _inputs(d, 1.0)
    table = _table()
    g = torch.Generator().manual_seed(9)
    angle = torch.rand(3 * PAGE + NEW, rdim // 2, generator=g) * 2 * math.pi
    cos, sin = torch.cos(angle).bfloat16(), torch.sin(angle).bfloat16()
    seq = torch.tensor(SEQLENS, dtype=torch.int32)
    kc, vc, q_out = _append(xfa, q, k, v, table, cos, sin, interleaved)
    # the fp32 rotary of the inputs (oracle.apply_rotary computes in fp32 and returns x's dtype)
    k_ro = orc.apply_rotary(k.float(), cos, sin, seq, interleaved)
    q_ro = orc.apply_rotary(q.float(), cos, sin, seq, interleaved)
    blank = torch.full((NPAGES, PAGE, HK, d), 0x55, dtype=torch.uint8)
    _, written = _expected(blank, table, _to_bytes(k_ro, KS), SEQLENS)
    # rows the append must not touch, and V (no rotary): exact
    assert bool((kc[~written] == 0x55).all())
    v_exp, _ = _expected(blank, table, _to_bytes(v.float(), VS), SEQLENS)
    assert torch.equal(vc, v_exp)
    # K: one rounding of the fp32 rotary to e4m3
    x_exp, _ = _expected(torch.zeros(NPAGES, PAGE, HK, d), table, k_ro, SEQLENS)
    deq = kc.view(torch.float8_e4m3fn).float() * KS
    x, got = x_exp[written], deq[written]
    assert float(x.abs().max()) < 448 * KS                    # nothing clamped: the bound applies
    bound = 2.0 ** -4 * x.abs() + 2.0 ** -10 * KS + 1e-6 * x.abs()
    excess = ((got - x).abs() - bound).max().item()
    assert excess <= 0, f"|deq - x| passes the half-ulp bound by {excess:.3g}"
    # q_out: the bf16 rounding of its fp32 rotary (+ 1e-6: fp32 contraction of x1 c - x2 s, whose
    # terms are below 8 here, when the result is small against them)
    qb = 2.0 ** -8 * q_ro.abs() + 1e-6 * q_ro.abs() + 1e-6
    assert bool(((q_out.float() - q_ro).abs() <= qb).all())


@pytest.mark.parametrize("rotary", [False, True])
def test_decode_loop_over_fp8_cache(xfa, rotary):
    """three decode steps: each appends one token per sequence into the fp8 cache and attends; the
    output is held to the oracle over the cache bytes read back and dequantised (the rule of the
    fp8-cache decode test, tests/test_config_shapes_gpu.py: 3 x the estimate + 1e-5, LSE 1e-3)"""
    d, rdim = 128, 64
    g = torch.Generator().manual_seed(21)
    table = _table().to(DEV)
    lens = [13, 30, 44]
    # a filled cache to start from (random bytes of moderate magnitude)
    kc = (torch.randn(NPAGES, PAGE, HK, d, generator=g) / KS).to(torch.float8_e4m3fn).to(DEV)
    vc = (torch.randn(NPAGES, PAGE, HK, d, generator=g) / VS).to(torch.float8_e4m3fn).to(DEV)
    cos = sin = None
    if rotary:
        angle = torch.rand(3 * PAGE, rdim // 2, generator=g) * 2 * math.pi
        cos, sin = torch.cos(angle).bfloat16().to(DEV), torch.sin(angle).bfloat16().to(DEV)
    for step in range(3):
        q = torch.randn(B, 1, H, d, generator=g).bfloat16()
        k = torch.randn(B, 1, HK, d, generator=g).bfloat16()
        v = torch.randn(B, 1, HK, d, generator=g).bfloat16()
        seq = torch.tensor([n + step for n in lens], dtype=torch.int32, device=DEV)
        out, lse = xfa.flash_attn_with_kvcache(
            q.to(DEV), kc, vc, k=k.to(DEV), v=v.to(DEV), rotary_cos=cos, rotary_sin=sin,
            cache_seqlens=seq, block_table=table, rotary_interleaved=False, k_scale=KS, v_scale=VS,
            return_softmax_lse=True)
        torch.cuda.synchronize()
        k8u, v8u = kc.view(torch.uint8).cpu(), vc.view(torch.uint8).cpu()
        q_att = q if not rotary else orc.apply_rotary(q, cos.cpu(), sin.cpu(), seq.cpu(), False)
        for b in range(B):
            n = lens[b] + step + 1
            idx = table[b].long().cpu()
            # exact dequantisation (fp32): the decode kernel multiplies the scores by k_scale and O
            # by v_scale in fp32, so with scales that are no powers of two a bf16 rounding of
            # fp8 x scale would put an error into the reference that the kernel does not have;
            # only the low-precision estimate, the yardstick of the tolerance, rounds to bf16
            kd = (k8u[idx].view(torch.float8_e4m3fn).float() * KS).reshape(1, -1, HK, d)[:, :n]
            vd = (v8u[idx].view(torch.float8_e4m3fn).float() * VS).reshape(1, -1, HK, d)[:, :n]
            # the new row is in the cache: the appended token, quantised
            k_new = k[b:b + 1].float() if not rotary else \
                orc.apply_rotary(k[b:b + 1].float(), cos.cpu(), sin.cpu(), seq[b:b + 1].cpu(), False)
            x = k_new[0, 0]
            row = k8u[idx].view(torch.float8_e4m3fn).float().reshape(-1, HK, d)[n - 1] * KS
            assert bool(((row - x).abs() <= 2.0 ** -4 * x.abs() + 2.0 ** -10 * KS + 1e-6 * x.abs()).all())
            qs = q_att[b:b + 1]
            ref, _ = orc.attention_ref(qs.float(), kd, vd)
            pt, _ = orc.attention_ref(qs, kd.bfloat16(), vd.bfloat16(), upcast=False, reorder_ops=True)
            ok, err, bound = orc.parity_ok(out[b:b + 1].cpu(), ref, pt, 3.0, 1e-5)
            assert ok, f"step {step} b{b}: {err:.3g} > {bound:.3g}"
            lerr = (lse[b:b + 1].cpu() - orc.attention_lse_ref(qs, kd)).abs().max().item()
            assert lerr < 1e-3, f"step {step} b{b}: LSE {lerr:.3g}"
