"""Same-box, interleaved timing of the MLA decode (`flash_mla_with_kvcache`, one
fmha_mla_decode_kernel launch plus the split combine) against the same attention composed from
torch eager ops over the gathered cache, at several split counts.

  python tools/mla_ab.py [--b 8] [--s 32768] [--page 64] [--heads 16 128] [--splits 0 ...]
                         [--rounds 7] [--iters 20]

Per head count (seqlen_q = 1, bf16, uniform lengths):
  bytes = sum n * 1152 (every cache row once) + q + o;  rate in TB/s against the 6.29 TB/s a
          streaming copy reaches on this part;
  FLOP  = 2 * b * heads * s * (576 + 512);              rate against the 2.5 PFLOP/s bf16 MFMA peak.
16 heads is one 16-row tile per sequence (the HBM-bound, tensor-parallel shape); 128 heads sits near
the ridge of the two bounds.  The eager contender reads a cache gathered once outside the timing
(it has no paged form) and materialises the scores.  Times are device events around `iters`
back-to-back calls, the contenders alternating within every round; the median over rounds is
printed.  There is no earlier kernel of this library to compare against: nothing else in it runs
head size 576.
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

STREAM_TBS = 6.29
PEAK_PFLOPS = 2.5
D, DV = 576, 512


def eager(q, kg, scale):
    """q [b, 1, h, 576], kg [b, s, 576] (gathered) -> o [b, 1, h, 512] in q's dtype."""
    s = torch.einsum("bqhd,bsd->bhqs", q, kg).float() * scale
    p = torch.softmax(s, dim=-1).to(q.dtype)
    return torch.einsum("bhqs,bsd->bqhd", p, kg[..., :DV])


def measure(a, heads):
    import xf_flash_attention_cutlass_amd as xfa
    from xf_flash_attention_cutlass_amd import capi
    dt = torch.bfloat16
    b, s, page = a.b, a.s, a.page
    per = s // page
    gen = torch.Generator(device="cuda").manual_seed(heads)
    kv = torch.randn(b * per, page, 1, D, device="cuda", dtype=dt, generator=gen)
    table = torch.randperm(b * per, device="cuda", generator=gen).to(torch.int32).view(b, per)
    lens = torch.full((b,), s, dtype=torch.int32, device="cuda")
    q = torch.randn(b, 1, heads, D, device="cuda", dtype=dt, generator=gen)
    out = torch.empty(b, 1, heads, DV, device="cuda", dtype=dt)
    kg = kv[table.long()].reshape(b, s, D)
    scale = D ** -0.5
    nbytes = b * s * D * 2 + q.numel() * 2 + out.numel() * 2
    flop = 2.0 * b * heads * s * (D + DV)

    def mla(ns):
        return lambda: xfa.flash_mla_with_kvcache(q, kv, table, lens, num_splits=ns, out=out)

    runs, kern = {}, {}
    ref = eager(q, kg, scale)
    for ns in a.splits:
        name = f"mla_decode num_splits={ns}"
        runs[name] = mla(ns)
        out.zero_()
        runs[name]()
        torch.cuda.synchronize()
        kern[name] = "%s splits=%d" % (capi.lib().fmha_last_kernel().decode(), capi.lib().fmha_last_num_splits())
        print(f"check {name}: max|o - eager| {(out.float() - ref.float()).abs().max().item():.3e}  [{kern[name]}]")
    runs["torch eager (gathered cache)"] = lambda: eager(q, kg, scale)
    del ref

    for run in runs.values():
        for _ in range(3):
            run()
    torch.cuda.synchronize()
    first = next(iter(runs.values()))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    k = 0
    while True:                                           # ~1 s clock-ramp prewarm
        first()
        k += 1
        if k % 20 == 0:
            e1.record()
            torch.cuda.synchronize()
            if e0.elapsed_time(e1) > 1000:
                break
    times = {name: [] for name in runs}
    for _ in range(a.rounds):
        for name, run in runs.items():
            s0, s1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s0.record()
            for _ in range(a.iters):
                run()
            s1.record()
            torch.cuda.synchronize()
            times[name].append(s0.elapsed_time(s1) / a.iters)
    print(f"MLA decode b={b} s_kv={s} page={page} heads={heads} seqlen_q=1 bf16: {nbytes / 1e6:.1f} MB, "
          f"{flop / 1e9:.1f} GFLOP per call")
    for name, t in times.items():
        med = statistics.median(t)
        tbs, pf = nbytes / med / 1e9, flop / med / 1e12
        print(f"{name}: median {med * 1e3:.1f} us  min {min(t) * 1e3:.1f}  max {max(t) * 1e3:.1f}  -> "
              f"{tbs:.2f} TB/s = {tbs / STREAM_TBS:.2f} of {STREAM_TBS} TB/s;  {pf:.3f} PFLOP/s = "
              f"{pf / PEAK_PFLOPS:.2f} of {PEAK_PFLOPS} PFLOP/s")
    del kv, kg
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--b", type=int, default=8)
    ap.add_argument("--s", type=int, default=32768)
    ap.add_argument("--page", type=int, default=64)
    ap.add_argument("--heads", type=int, nargs="+", default=[16, 128])
    ap.add_argument("--splits", type=int, nargs="+", default=[0, 16, 32, 64],
                    help="num_splits values to time (0 = the library's choice)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "mla_ab.py measures on the GPU"
    assert a.s % a.page == 0
    for heads in a.heads:
        measure(a, heads)


if __name__ == "__main__":
    main()
