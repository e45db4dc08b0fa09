"""Same-box, interleaved timing of `merge_states` (one fmha_merge_states launch) against the same
merge composed from torch eager ops on the device, and optionally against other BUILDS of the
library through the C ABI (e.g. one compiled with -DXFA_MERGE_NT=0, tools/build_variant.sh).

  python tools/merge_ab.py [--parts 2] [--b 4] [--s 4096] [--h 32] [--d 128] [--rounds 7]
                           [--iters 20] [--lib name=path.so ...]

Bytes per call, from the shapes: (parts + 1) * R * d * 2 for O plus (parts + 1) * R * 4 for the
LSEs, R = b * s * h.  The rate is reported in TB/s and as a fraction of the 6.3 TB/s a streaming
copy reaches on this part.  Times are device events around `iters` back-to-back
calls, the contenders alternating within every round; the median over rounds is printed.
"""
from __future__ import annotations

import argparse
import ctypes as C
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

STREAM_TBS = 6.3


def eager_merge(os_, ls):
    """The merge from eager ops (any part count; no absent-part handling: finite LSEs only)."""
    L = torch.stack(ls)                                   # [n, b, h, rows]
    m = L.max(0).values
    w = torch.exp(L - m)
    den = w.sum(0)
    wn = (w / den).permute(0, 1, 3, 2).unsqueeze(-1)      # [n, b, rows, h, 1]
    out = wn[0] * os_[0].float()
    for i in range(1, len(os_)):
        out += wn[i] * os_[i].float()
    return out.to(os_[0].dtype), m + torch.log(den)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", type=int, default=2)
    ap.add_argument("--b", type=int, default=4)
    ap.add_argument("--s", type=int, default=4096)
    ap.add_argument("--h", type=int, default=32)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--lib", action="append", default=[], help="name=path of another build (C ABI)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "merge_ab.py measures on the GPU"

    import xf_flash_attention_cutlass_amd as xfa
    from xf_flash_attention_cutlass_amd import capi
    dt = torch.bfloat16
    n, rows = a.parts, a.s
    os_ = [torch.randn(a.b, rows, a.h, a.d, device="cuda", dtype=dt) for _ in range(n)]
    ls = [torch.randn(a.b, a.h, rows, device="cuda") * 3 for _ in range(n)]
    out, lse = torch.empty_like(os_[0]), torch.empty_like(ls[0])
    R = a.b * rows * a.h
    nbytes = (n + 1) * R * a.d * 2 + (n + 1) * R * 4
    stream = torch.cuda.current_stream().cuda_stream

    op = (C.c_void_p * n)(*[x.data_ptr() for x in os_])
    lp = (C.c_void_p * n)(*[x.data_ptr() for x in ls])
    st = (C.c_int64 * 10)(*os_[0].stride()[:3], *out.stride()[:3], *ls[0].stride()[:2], *lse.stride()[:2])

    def c_call(lib):
        def run():
            lib.fmha_merge_states(op, lp, n, out.data_ptr(), lse.data_ptr(), None, a.b, rows, a.h, a.d,
                                  st, False, stream)
        return run

    runs = {"merge_states (op)": lambda: xfa.paged_attn.merge_states(os_, ls, None, False, out, lse),
            "C ABI, product build": c_call(capi.lib()),
            "torch eager": lambda: eager_merge(os_, ls)}
    for spec in a.lib:
        name, _, path = spec.partition("=")
        runs[f"C ABI, {name}"] = c_call(capi.load(path, strict=False))

    # every contender against the eager result (a sanity check at the timed size, not the parity test)
    ref_o, ref_l = eager_merge(os_, ls)
    for name, run in runs.items():
        if name == "torch eager":
            continue
        out.zero_()
        lse.zero_()
        run()
        torch.cuda.synchronize()
        assert capi.lib().fmha_last_status() == 0, capi.lib().fmha_last_error()
        print(f"check {name}: max|o - eager| {(out.float() - ref_o.float()).abs().max().item():.3e} "
              f"max|lse - eager| {(lse - ref_l).abs().max().item():.3e}")
    del ref_o, ref_l

    for run in runs.values():
        for _ in range(3):
            run()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    k = 0
    while True:                                           # ~1 s clock-ramp prewarm
        runs["C ABI, product build"]()
        k += 1
        if k % 50 == 0:
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
    print(f"merge parts={n} R={a.b}x{rows}x{a.h}={R} d={a.d} bf16: {nbytes / 1e6:.1f} MB per call")
    for name, t in times.items():
        med = statistics.median(t)
        tbs = nbytes / med / 1e9
        note = "" if name != "torch eager" else "  (rate on the fused call's bytes; eager moves more)"
        print(f"{name}: median {med * 1e3:.1f} us  min {min(t) * 1e3:.1f}  max {max(t) * 1e3:.1f}  -> "
              f"{tbs:.2f} TB/s = {tbs / STREAM_TBS:.2f} of {STREAM_TBS} TB/s{note}")
    eager, fused = statistics.median(times["torch eager"]), statistics.median(times["merge_states (op)"])
    print(f"single launch vs eager composition: {eager / fused:.2f}x "
          f"({'not slower' if fused <= eager else 'SLOWER'})")


if __name__ == "__main__":
    main()
