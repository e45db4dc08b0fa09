"""A/B of the sparse MLA prefill attention on the GPU:

  python tools/mla_sparse_fwd_ab.py [--sq 512 4096] [--heads 16 64 128] [--topk 2048] [--s 32768]

(a) flash_mla_sparse_fwd: one workgroup per position and 64 heads, the gather shared by four waves;
(b) the route before it: flash_mla_with_kvcache(q[None], cache, None, None, indices=idx[None]), the
    sparse decode kernel at batch 1 and seqlen_q = s_q, automatic splits, its combine included.

bf16, a paged latent cache of s slots (page 64) viewed flat for (a); every position draws topk
random slots below its causal limit s - s_q + i + 1, sorted ascending.  Per cell:
  FLOP  = 2 * s_q * heads * topk * (576 + 512);  the rate against the 2.5 PFLOP/s bf16 MFMA peak;
  L2-side bytes of the gather = s_q * groups * topk * 1152, groups = ceil(heads / 64) for (a) and
          ceil(heads / 16) for (b): how often a selected row is pulled into a CU.
Times are device events around `iters` back-to-back calls (iters sized so that a window is about
half a second), the contenders alternating within every round after a prewarm of both; the median
and min-max over the rounds are printed, and the largest difference between the two results.
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_PFLOPS = 2.5
D, DV, PAGE = 576, 512, 64


def timed(fn, iters):
    beg, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    beg.record()
    for _ in range(iters):
        fn()
    end.record()
    torch.cuda.synchronize()
    return beg.elapsed_time(end) / iters


def cell(a, sq, heads):
    import xf_flash_attention_cutlass_amd as xfa
    from xf_flash_attention_cutlass_amd import capi
    dt, s, topk = torch.bfloat16, a.s, a.topk
    gen = torch.Generator(device="cuda").manual_seed(sq + heads)
    cache = torch.randn(s // PAGE, PAGE, 1, D, device="cuda", dtype=dt, generator=gen)
    q = torch.randn(sq, heads, D, device="cuda", dtype=dt, generator=gen)
    lim = torch.arange(s - sq + 1, s + 1, device="cuda")                     # causal limit of row i
    idx = (torch.rand(sq, topk, device="cuda", generator=gen) * lim[:, None]).long().clamp_(max=s - 1)
    idx = idx.sort(dim=-1).values.to(torch.int32)
    o_a = torch.empty(sq, heads, DV, device="cuda", dtype=dt)
    o_b = torch.empty(1, sq, heads, DV, device="cuda", dtype=dt)
    scale = D ** -0.5
    runs = {"(a) sparse_fwd": lambda: xfa.flash_mla_sparse_fwd(q, cache.view(-1, 1, D), idx, scale, out=o_a),
            "(b) sparse decode, b=1": lambda: xfa.flash_mla_with_kvcache(q[None], cache, None, None, softmax_scale=scale,
                                                                         out=o_b, indices=idx[None])}
    iters, kern = {}, {}
    for name, fn in runs.items():                                             # prewarm, and size the window
        fn()
        torch.cuda.synchronize()
        kern[name] = capi.lib().fmha_last_kernel().decode() + f" splits={capi.lib().fmha_last_num_splits()}"
        iters[name] = max(1, min(50, round(500.0 / timed(fn, 1))))
    diff = (o_a.float() - o_b[0].float()).abs().max().item()
    times = {name: [] for name in runs}
    for _ in range(a.rounds):
        for name, fn in runs.items():
            times[name].append(timed(fn, iters[name]))
    flop = 2.0 * sq * heads * topk * (D + DV)
    print(f"sparse MLA prefill bf16 s_q={sq} heads={heads} s_kv={s} topk={topk}: {flop / 1e12:.1f} TFLOP, "
          f"max |o_a - o_b| = {diff:.3e}")
    for name, groups in (("(a) sparse_fwd", (heads + 63) // 64), ("(b) sparse decode, b=1", (heads + 15) // 16)):
        t = times[name]
        med = statistics.median(t)
        l2 = sq * groups * topk * 1152
        print(f"  {name:<24} {med:10.3f} ms (min {min(t):.3f} max {max(t):.3f}, {iters[name]} calls a window)  "
              f"{flop / med / 1e12:7.3f} PFLOP/s = {flop / med / 1e12 / PEAK_PFLOPS:.3f} of peak  "
              f"L2-side {l2 / 1e9:6.1f} GB = {l2 / med / 1e9:.2f} TB/s  [{kern[name]}]")
    ta, tb = times["(a) sparse_fwd"], times["(b) sparse decode, b=1"]
    apart = max(ta) < min(tb) or max(tb) < min(ta)
    print(f"  (b) / (a) = {statistics.median(tb) / statistics.median(ta):.2f}"
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
