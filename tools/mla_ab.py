"""Same-box, interleaved timing of the MLA decode (`flash_mla_with_kvcache`, one
fmha_mla_decode_kernel launch plus the split combine) against the same attention composed from
torch eager ops over the gathered cache, at several split counts.

  python tools/mla_ab.py [--b 8] [--s 32768] [--page 64] [--heads 16 128] [--splits 0 ...]
                         [--rounds 7] [--iters 20] [--fp8] [--append 8192]

--fp8 adds the fp8-cache call (fmha_mla_decode_fp8_kernel over rows of 656 bytes, the same tokens
appended with mla_cache_append_fp8) as a contender of every split count, next to the 16-bit-cache
call of the same build, and an eager contender over the dequantised gathered cache; its bytes are
n * 656 + q + o.  --append N times the append kernel alone on N tokens (bytes read + written).

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
    qo = q.numel() * 2 + out.numel() * 2
    nbytes = {"": b * s * D * 2 + qo}
    flop = 2.0 * b * heads * s * (D + DV)

    def mla(cache, ns):
        return lambda: xfa.flash_mla_with_kvcache(q, cache, table, lens, num_splits=ns, out=out)

    caches, refs = {"mla_decode": kv}, {"mla_decode": eager(q, kg, scale)}
    if a.fp8:
        # the same tokens in an fp8 cache, written by the append kernel through the same table
        kv8 = torch.zeros(b * per, page, 1, xfa.mla_fp8_cache_row_bytes, device="cuda", dtype=torch.uint8)
        flat = kv.view(-1, D)
        xfa.mla_cache_append_fp8(flat[:, :DV], flat[:, DV:], kv8, torch.arange(flat.shape[0], device="cuda"))
        r8 = kv8.view(-1, xfa.mla_fp8_cache_row_bytes)
        ds = r8[:, 512:528].contiguous().view(torch.float32).repeat_interleave(128, dim=1)
        lat = (r8[:, :DV].contiguous().view(torch.float8_e4m3fn).float() * ds).to(dt)
        kdq = torch.cat([lat, r8[:, 528:].contiguous().view(dt)], 1).view(b * per, page, D)
        kg8 = kdq[table.long()].reshape(b, s, D)
        caches["mla_decode_fp8"], refs["mla_decode_fp8"] = kv8, eager(q, kg8, scale)
        nbytes["fp8"] = b * s * xfa.mla_fp8_cache_row_bytes + qo
        del r8, ds, lat, kdq
    runs, kern = {}, {}
    for ns in a.splits:
        for op, cache in caches.items():
            name = f"{op} num_splits={ns}"
            runs[name] = mla(cache, ns)
            out.zero_()
            runs[name]()
            torch.cuda.synchronize()
            kern[name] = "%s splits=%d" % (capi.lib().fmha_last_kernel().decode(), capi.lib().fmha_last_num_splits())
            print(f"check {name}: max|o - eager| {(out.float() - refs[op].float()).abs().max().item():.3e}  [{kern[name]}]")
    runs["torch eager (gathered cache)"] = lambda: eager(q, kg, scale)
    if a.fp8:
        runs["torch eager (dequantised gathered cache)"] = lambda: eager(q, kg8, scale)
    del refs

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
    print(f"MLA decode b={b} s_kv={s} page={page} heads={heads} seqlen_q=1 bf16: {nbytes[''] / 1e6:.1f} MB "
          + (f"(fp8 cache {nbytes['fp8'] / 1e6:.1f} MB), " if a.fp8 else "") + f"{flop / 1e9:.1f} GFLOP per call")
    for name, t in times.items():
        med = statistics.median(t)
        nb = nbytes["fp8" if name.startswith("mla_decode_fp8") else ""]     # bytes the call actually reads
        tbs, pf = nb / med / 1e9, flop / med / 1e12
        print(f"{name}: median {med * 1e3:.1f} us  min {min(t) * 1e3:.1f}  max {max(t) * 1e3:.1f}  -> "
              f"{tbs:.2f} TB/s = {tbs / STREAM_TBS:.2f} of {STREAM_TBS} TB/s;  {pf:.3f} PFLOP/s = "
              f"{pf / PEAK_PFLOPS:.2f} of {PEAK_PFLOPS} PFLOP/s")
    del kv, kg, caches
    torch.cuda.empty_cache()


def measure_append(a):
    """The append kernel alone: `a.append` tokens (two views of one 576-wide tensor) into an fp8
    cache through a shuffled slot_mapping; bytes = tokens * (1152 read + 8 slot + 656 written)."""
    import xf_flash_attention_cutlass_amd as xfa
    n, page = a.append, a.page
    blocks = (n + page - 1) // page
    gen = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn(n, D, device="cuda", dtype=torch.bfloat16, generator=gen)
    slots = torch.randperm(blocks * page, device="cuda", generator=gen)[:n].contiguous()
    kv8 = torch.zeros(blocks, page, 1, xfa.mla_fp8_cache_row_bytes, device="cuda", dtype=torch.uint8)
    run = lambda: xfa.mla_cache_append_fp8(x[:, :DV], x[:, DV:], kv8, slots)  # noqa: E731
    for _ in range(20):
        run()
    torch.cuda.synchronize()
    times = []
    for _ in range(a.rounds):
        s0, s1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s0.record()
        for _ in range(a.iters):
            run()
        s1.record()
        torch.cuda.synchronize()
        times.append(s0.elapsed_time(s1) / a.iters)
    med = statistics.median(times)
    nb = n * (D * 2 + 8 + xfa.mla_fp8_cache_row_bytes)
    print(f"mla_cache_append_fp8 tokens={n} page={page}: median {med * 1e3:.1f} us  min {min(times) * 1e3:.1f}  "
          f"max {max(times) * 1e3:.1f}  -> {nb / 1e6:.1f} MB read + written, {nb / med / 1e9:.2f} TB/s = "
          f"{nb / med / 1e9 / STREAM_TBS:.2f} of {STREAM_TBS} TB/s (launch-bound at this size: back-to-back calls)")


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
    ap.add_argument("--fp8", action="store_true", help="add the fp8-cache call and its eager contender")
    ap.add_argument("--append", type=int, default=0, help="also time mla_cache_append_fp8 on this many tokens")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "mla_ab.py measures on the GPU"
    assert a.s % a.page == 0
    for heads in a.heads:
        measure(a, heads)
    if a.append:
        measure_append(a)


if __name__ == "__main__":
    main()
