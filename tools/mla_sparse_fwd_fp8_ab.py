"""A/B of the sparse MLA prefill attention over the fp8 latent cache on the GPU:

  python tools/mla_sparse_fwd_fp8_ab.py [--sq 512 4096] [--heads 16 64 128] [--topk 2048] [--s 32768]

(a) flash_mla_sparse_fwd over the fp8 cache viewed flat: one workgroup per position and 64 heads, a
    selected row gathered and dequantised once for the four waves;
(b) what the cache had before: flash_mla_with_kvcache(q[None], cache8, None, None, indices=idx[None]),
    the sparse fp8 decode kernel at batch 1 and seqlen_q = s_q, automatic splits, combine included;
(c) the 16-bit flash_mla_sparse_fwd over the same rows kept dequantised in bf16 (a second cache);
(d) the up-convert route: torch gathers the referenced rows (unique), dequantises them into a bf16
    workspace, remaps the indices, and the 16-bit flash_mla_sparse_fwd runs over the workspace.

bf16 q, a paged fp8 latent cache of s slots (page 64) written by mla_cache_append_fp8; every position
draws topk random slots below its causal limit s - s_q + i + 1, sorted ascending.  Per cell:
  FLOP  = 2 * s_q * heads * topk * (576 + 512);  the rate against the 2.5 PFLOP/s bf16 MFMA peak;
  L2-side bytes of the gather = s_q * groups * topk * row bytes (656 fp8, 1152 bf16), groups =
          ceil(heads / 64) for (a), (c), (d) and ceil(heads / 16) for (b);
  conversions per token = groups * topk * 512 e4m3 features ((c): none, (d): in torch).
Times are device events around `iters` back-to-back calls (iters sized so that a window is about
0.4 s), the contenders alternating within every round after a prewarm of all; the median and
min-max over the rounds are printed, and the largest difference of every result from (a)'s.
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_PFLOPS = 2.5
D, DV, PAGE, ROW = 576, 512, 64, 656


def timed(fn, iters):
    beg, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    beg.record()
    for _ in range(iters):
        fn()
    end.record()
    torch.cuda.synchronize()
    return beg.elapsed_time(end) / iters


def dequant(rows8, dt):
    """uint8 [n, 656] -> dt [n, 576]: the operand the fp8 kernels attend over."""
    lat = rows8[:, :512].view(torch.float8_e4m3fn).float().view(-1, 4, 128)
    ds = rows8[:, 512:528].contiguous().view(torch.float32)
    return torch.cat([(lat * ds[..., None]).to(dt).view(-1, 512), rows8[:, 528:].contiguous().view(dt)], -1)


def cell(a, sq, heads):
    import xf_flash_attention_cutlass_amd as xfa
    from xf_flash_attention_cutlass_amd import capi
    dt, s, topk = torch.bfloat16, a.s, a.topk
    gen = torch.Generator(device="cuda").manual_seed(sq + heads)
    src = torch.randn(s, D, device="cuda", dtype=dt, generator=gen)
    cache8 = torch.zeros(s // PAGE, PAGE, 1, ROW, device="cuda", dtype=torch.uint8)
    xfa.mla_cache_append_fp8(src[:, :512], src[:, 512:], cache8, torch.arange(s, device="cuda"))
    flat8 = cache8.view(-1, 1, ROW)
    cache16 = dequant(flat8[:, 0], dt).view(-1, 1, D)
    q = torch.randn(sq, heads, D, device="cuda", dtype=dt, generator=gen)
    lim = torch.arange(s - sq + 1, s + 1, device="cuda")                     # causal limit of row i
    idx = (torch.rand(sq, topk, device="cuda", generator=gen) * lim[:, None]).long().clamp_(max=s - 1)
    idx = idx.sort(dim=-1).values.to(torch.int32)
    scale = D ** -0.5
    outs = {n: torch.empty(sq, heads, DV, device="cuda", dtype=dt) for n in "acd"}
    outs["b"] = torch.empty(1, sq, heads, DV, device="cuda", dtype=dt)

    def upconvert():
        uniq, inverse = torch.unique(idx, return_inverse=True)
        work = dequant(flat8[uniq.long(), 0], dt).view(-1, 1, D)
        return xfa.flash_mla_sparse_fwd(q, work, inverse.to(torch.int32), scale, out=outs["d"])

    runs = {"a": ("(a) sparse_fwd, fp8 cache", lambda: xfa.flash_mla_sparse_fwd(q, flat8, idx, scale, out=outs["a"])),
            "b": ("(b) sparse fp8 decode, b=1", lambda: xfa.flash_mla_with_kvcache(
                q[None], cache8, None, None, softmax_scale=scale, out=outs["b"], indices=idx[None])),
            "c": ("(c) sparse_fwd, bf16 cache", lambda: xfa.flash_mla_sparse_fwd(q, cache16, idx, scale, out=outs["c"])),
            "d": ("(d) up-convert + sparse_fwd", upconvert)}
    iters, kern = {}, {}
    for n, (_, fn) in runs.items():                                           # prewarm, and size the window
        fn()
        torch.cuda.synchronize()
        kern[n] = capi.lib().fmha_last_kernel().decode() + f" splits={capi.lib().fmha_last_num_splits()}"
        iters[n] = max(1, min(1000, round(400.0 / timed(fn, 1))))
    diff = {n: (outs["a"].float() - outs[n].view(sq, heads, DV).float()).abs().max().item() for n in "bcd"}
    times = {n: [] for n in runs}
    for _ in range(a.rounds):
        for n, (_, fn) in runs.items():
            times[n].append(timed(fn, iters[n]))
    flop = 2.0 * sq * heads * topk * (D + DV)
    print(f"sparse MLA prefill, fp8 cache, bf16 q, s_q={sq} heads={heads} s_kv={s} topk={topk}: {flop / 1e12:.2f} TFLOP, "
          f"max |o_a - o_x| = " + ", ".join(f"{n} {v:.3e}" for n, v in diff.items()))
    g64, g16 = (heads + 63) // 64, (heads + 15) // 16
    for n, groups, rowb, conv in (("a", g64, ROW, g64), ("b", g16, ROW, g16), ("c", g64, 1152, 0), ("d", g64, 1152, None)):
        t = times[n]
        med = statistics.median(t)
        l2 = sq * groups * topk * rowb
        cv = "in torch" if conv is None else f"{conv * topk * 512}"
        print(f"  {runs[n][0]:<28} {med:9.3f} ms (min {min(t):.3f} max {max(t):.3f}, {iters[n]} calls a window)  "
              f"{flop / med / 1e12 / PEAK_PFLOPS:.3f} of peak  L2-side {l2 / 1e9:6.2f} GB = {l2 / med / 1e9:.2f} TB/s  "
              f"conversions a token {cv}  [{kern[n]}]")
    ta = times["a"]
    for n in "bcd":
        tx = times[n]
        apart = max(ta) < min(tx) or max(tx) < min(ta)
        print(f"  ({n}) / (a) = {statistics.median(tx) / statistics.median(ta):.2f}"
              f" ({'outside' if apart else 'INSIDE'} the spread of both)", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sq", type=int, nargs="+", default=[512, 4096])
    ap.add_argument("--heads", type=int, nargs="+", default=[16, 64, 128])
    ap.add_argument("--topk", type=int, default=2048)
    ap.add_argument("--s", type=int, default=32768)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    print(torch.cuda.get_device_name(0))
    for sq in a.sq:
        for heads in a.heads:
            cell(a, sq, heads)


if __name__ == "__main__":
    main()
