"""In-process, interleaved timing of the attention-sink forward against the same call without a
sink, one shape per mechanism:

  epilogue   B2 S4096 H64/Hk8 D64 bf16, causal and window (127, 0) (the gpt-oss prefill shapes):
             fmha_fwd_sink with a sink against fmha_fwd_strided;
  post-pass  the C2 shape (B4 S4096 H32 D128 bf16, causal): the generated body plus
             fmha_sink_kernel against the body alone; the pass's own time is the difference of the
             medians, its GB/s the logical bytes (O read and written, LSE read and written, in
             place) over it, next to the float4 copy rate; and its share of the forward;
  combine    decode B8 H64/Hk8 D64 over a 32768-key bf16 cache, page 16: the sink in the split
             combine against the plain combine.

HIP-event times, without-sink and with-sink alternating in one process (five alternations by
default) so clock drift cancels; the spread (min .. max over the alternations) is printed next to
each median, and the gfx clock over the timed windows.  Every GPU step runs under its own time
limit (status 124, nothing more is started).  Run the tool itself under a limit as well:

  timeout -k 10 300 python tools/sink_ab.py [--rounds 5] [--iters 50]
"""
from __future__ import annotations

import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from quant_ab import COPY_GBS, alternate, clock, report, step_limit  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--step-timeout", type=float, default=60.0)
    ap.add_argument("--no-monitor", action="store_true")
    a = ap.parse_args()
    import bench
    monitor = None if a.no_monitor else bench.ClockMonitor()   # before the GPU is touched
    try:
        return run(a, bench, monitor)
    finally:
        if monitor:
            monitor.close()


def measure(a, monitor, title, base, sink, lib, want_tag):
    """Warm up, ramp the clock (~1 s), alternate; returns (median base ms, median sink ms)."""
    import torch
    from xf_flash_attention_cutlass_amd import capi
    with step_limit(title + " warm-up", a.step_timeout):
        for fn in (base, sink):
            for _ in range(3):
                fn()
            capi.check()
        kern = lib.fmha_last_kernel().decode()
        assert kern.endswith(" sink=" + want_tag), kern
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        while True:
            for _ in range(5):
                base()
            e1.record()
            torch.cuda.synchronize()
            if e0.elapsed_time(e1) > 1000:
                break
    times, windows = alternate(a, [("without sink", base), ("with sink", sink)], torch.cuda.synchronize)
    print(f"{title}: {kern}  [{clock(monitor, windows)}]")
    report("without sink", times[0])
    report("with sink   ", times[1])
    tb, ts = statistics.median(times[0]), statistics.median(times[1])
    print(f"  with / without = {ts / tb:.4f}  (spread of the alternations: without "
          f"{(max(times[0]) - min(times[0])) / tb * 100:.2f} %, with {(max(times[1]) - min(times[1])) / ts * 100:.2f} %)")
    return tb, ts


def run(a, bench, monitor):
    import torch
    from xf_flash_attention_cutlass_amd import capi

    if not torch.cuda.is_available():
        print("sink_ab needs a GPU (nothing is measured without one)")
        return 2
    lib = capi.lib()
    dev = torch.device("cuda", 0)
    if monitor:
        monitor.select(bench.device_info(dev)["pci_bus"])
    g = torch.Generator(device=dev).manual_seed(0)
    stream = torch.cuda.current_stream().cuda_stream
    P = lambda t: t.data_ptr()  # noqa: E731
    bf = torch.bfloat16

    def dense(B, S, H, HK, D, wl, wr):
        q = torch.randn(B, S, H, D, device=dev, generator=g).to(bf)
        k = torch.randn(B, S, HK, D, device=dev, generator=g).to(bf)
        v = torch.randn(B, S, HK, D, device=dev, generator=g).to(bf)
        o = torch.empty_like(q)
        lse = torch.empty(B, H, S, device=dev)
        sink = torch.linspace(-3, 3, H, device=dev)
        st = (ctypes.c_int64 * 12)(*[s for t in (q, k, v, o) for s in t.stride()[:3]])
        args = (P(q), P(k), P(v), P(o), None, P(lse), S, S, B, H, HK, D, st, D ** -0.5, wl, wr, 0.0,
                False, 0, stream, 0.0, None)
        keep = (q, k, v, o, lse, sink, st)
        return (lambda: lib.fmha_fwd_strided(*args)), (lambda: lib.fmha_fwd_sink(*args, P(sink))), keep

    # ---- epilogue: the D = 64 prefill
    for title, wl in (("epilogue D64 causal", -1), ("epilogue D64 window (127, 0)", 127)):
        base, sink, keep = dense(2, 4096, 64, 8, 64, wl, 0)
        measure(a, monitor, f"{title}, B2 S4096 H64/Hk8", base, sink, lib, "epilogue")
        del keep

    # ---- post-pass: the C2 shape
    B, S, H, D = 4, 4096, 32, 128
    base, sink, keep = dense(B, S, H, H, D, -1, 0)
    tb, ts = measure(a, monitor, "post-pass C2 causal, B4 S4096 H32 D128", base, sink, lib, "pass")
    nbytes = 2 * (B * S * H * D * 2) + 2 * (B * H * S * 4)
    dt = ts - tb
    print(f"  fmha_sink_kernel = {dt * 1e3:.1f} us over {nbytes / 1e6:.0f} MB (O and LSE, read and written) "
          f"-> {nbytes / dt / 1e6:.0f} GB/s ({nbytes / dt / 1e6 / COPY_GBS * 100:.0f} % of the {COPY_GBS:.0f} GB/s "
          f"copy rate); {dt / tb * 100:.1f} % of the forward")
    del keep

    # ---- combine: decode over a long bf16 cache
    DB, DH, DHK, DD, DS, page = 8, 64, 8, 64, 32768, 16
    nb = DB * DS // page
    table = torch.randperm(nb, device=dev).to(torch.int32).view(DB, DS // page)
    dq = torch.randn(DB, 1, DH, DD, device=dev, generator=g).to(bf)
    do = torch.empty_like(dq)
    dlse = torch.empty(DB, DH, 1, device=dev)
    lens = torch.full((DB,), DS, dtype=torch.int32, device=dev)
    kc = torch.randn(nb, page, DHK, DD, device=dev, generator=g).to(bf)
    vc = torch.randn(nb, page, DHK, DD, device=dev, generator=g).to(bf)
    dsink = torch.linspace(-3, 3, DH, device=dev)
    dargs = (P(dq), P(kc), P(vc), P(do), P(dlse), P(table), DS // page, P(lens), 1, DS, DB, DH, DHK, DD,
             page, DD ** -0.5, -1, -1, 0.0, None, 0, 0, 0, 1.0, 1.0, None, False, stream)
    a.iters *= 4
    measure(a, monitor, "combine decode B8 H64/Hk8 D64 S_kv 32768 page 16 bf16 cache",
            lambda: lib.fmha_page_kvcache_fwd_ex(*dargs),
            lambda: lib.fmha_page_kvcache_fwd_sink(*dargs, P(dsink)), lib, "combine")
    return 0


if __name__ == "__main__":
    sys.exit(main())
