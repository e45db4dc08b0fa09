"""In-process, interleaved timing of the fp8 quantising kernel and of the device-descale forward at
the C2 tensor shape (B4 S4096 H32 D128 bf16):

  quantise   fmha_quantize_fp8 (one call: two passes over x, descale left on the device) against
             the torch sequence it replaces, at both granularities:
               tensor:  amax -> host scalar (a sync) -> divide -> clamp -> cast
               head:    amax over (seq, d) -> divide -> clamp -> cast, all on the device
             with its achieved GB/s: logical bytes (x read twice, x8 written once) over the time;
  forward    the fp8 C2 causal forward through fmha_fwd_fp8_ex with [b, hk] device descales against
             fmha_fwd_fp8 with the same scales by value.

HIP-event times, baseline and candidate alternating in one process (five alternations by default)
so clock drift cancels; the spread (min .. max over the alternations) is printed next to each
median, and the gfx clock over the timed windows (tools/gpu_monitor.py through bench.ClockMonitor).
Every GPU step runs under its own time limit (status 124, nothing more is started).  Run the tool
itself under a limit as well:

  timeout -k 10 300 python tools/quant_ab.py [--rounds 5] [--iters 100]
"""
from __future__ import annotations

import argparse
import ctypes
import os
import statistics
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_GBS = 6290.0      # measured float4 copy rate of the MI355X (HBM3E, 79 % of the 8 TB/s peak)


class step_limit:
    """`with step_limit(name, seconds)`: the process ends (status 124) if the block runs longer"""

    def __init__(self, name, seconds):
        self.name, self.seconds = name, seconds

    def _expire(self):
        print(f"step '{self.name}' passed its {self.seconds:.0f} s limit: giving up", flush=True)
        os._exit(124)

    def __enter__(self):
        self.timer = threading.Timer(self.seconds, self._expire)
        self.timer.daemon = True
        self.timer.start()

    def __exit__(self, *exc):
        self.timer.cancel()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=100)
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


def alternate(a, variants, sync):
    """times[i]: per-call ms of variants[i] over a.rounds alternations; windows for the clock"""
    import torch
    times = [[] for _ in variants]
    windows = []
    for r in range(a.rounds):
        for i, (name, fn) in enumerate(variants):
            with step_limit(f"round {r} {name}", a.step_timeout):
                s0, s1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                w0 = time.time()
                s0.record()
                for _ in range(a.iters):
                    fn()
                s1.record()
                torch.cuda.synchronize()
                windows.append((w0, time.time()))
                times[i].append(s0.elapsed_time(s1) / a.iters)
    return times, windows


def clock(monitor, windows):
    """gfx clock over the whole timed region of one measurement (the sampler ticks every ~0.1 s,
    longer than one timed window)"""
    if not monitor:
        return "gfx clock: not sampled"
    time.sleep(0.3)                                   # let the sampler flush its last samples
    t0, t1 = windows[0][0], windows[-1][1]
    mhz = [sum(s["gfx_mhz"]) / len(s["gfx_mhz"]) for s in monitor.samples()
           if s.get("gfx_mhz") and t0 <= s["t"] <= t1]
    if not mhz:
        return "gfx clock: no sample in the timed region"
    return f"gfx {statistics.median(mhz):.0f} MHz (median of {len(mhz)} samples over the timed region)"


def report(name, t, extra=""):
    print(f"  {name}: median {statistics.median(t) * 1e3:.1f} us  (min {min(t) * 1e3:.1f}, "
          f"max {max(t) * 1e3:.1f} over {len(t)} alternations){extra}")


def run(a, bench, monitor):
    import torch
    import xf_flash_attention_cutlass_amd as xfa
    from xf_flash_attention_cutlass_amd import capi

    if not torch.cuda.is_available():
        print("quant_ab needs a GPU (nothing is measured without one)")
        return 2
    lib = capi.lib()
    dev = torch.device("cuda", 0)
    if monitor:
        monitor.select(bench.device_info(dev)["pci_bus"])
    B, S, H, D = 4, 4096, 32, 128
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(B, S, H, D, device=dev, generator=g).bfloat16()
    n = x.numel()
    stream = torch.cuda.current_stream().cuda_stream
    x8 = torch.empty(B, S, H, D, device=dev, dtype=torch.uint8)
    ds = torch.empty(B, H, device=dev, dtype=torch.float32)
    st = (ctypes.c_int64 * 3)(*x.stride()[:3])

    def kernel(gran):
        return lambda: lib.fmha_quantize_fp8(x.data_ptr(), x8.data_ptr(), ds.data_ptr(), None, B, S, H,
                                             1, D, st, gran, False, stream)

    def torch_tensor():
        scale = float(x.abs().amax()) / 448.0 or 1.0
        return (x.float() / scale).clamp(-448, 448).to(torch.float8_e4m3fn), scale

    def torch_head():
        amax = x.abs().amax(dim=(1, 3)).float()
        d = torch.where(amax == 0, torch.ones_like(amax), amax / 448.0)
        return (x.float() * (1 / d)[:, None, :, None]).clamp(-448, 448).to(torch.float8_e4m3fn), d

    print(f"quantise: x [{B}, {S}, {H}, {D}] bf16, {n * 2 / 1e6:.0f} MB; "
          f"logical traffic of the kernel {n * 5 / 1e6:.0f} MB (x read twice, x8 written once)")
    with step_limit("check", a.step_timeout):
        xc = x[:, :64].cpu().float()                      # a slab, checked on the CPU (IEEE divide)
        for gran in (0, 1):
            kernel(gran)()
            capi.check()
            torch.cuda.synchronize()
            # the entry's formula (include/paged_attn.h): x * (1 / descale), clamp, one rounding
            d = ds.cpu() if gran else ds.flatten()[:1].cpu().expand(B, H)
            r8 = (xc * (1 / d)[:, None, :, None]).clamp(-448, 448).to(torch.float8_e4m3fn)
            same = torch.equal(x8[:, :64].cpu(), r8.view(torch.uint8))
            print(f"  check granularity {gran}: the first 64 rows' bytes equal the formula's: {same}")
    for gran, ref, what in ((0, torch_tensor, "tensor"), (1, torch_head, "head")):
        variants = [(f"torch sequence ({what})", ref), (f"fmha_quantize_fp8 ({what})", kernel(gran))]
        with step_limit("warm-up", a.step_timeout):
            for _, fn in variants:
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
        times, windows = alternate(a, variants, torch.cuda.synchronize)
        print(f"granularity {what}:  [{clock(monitor, windows)}]")
        report(variants[0][0], times[0])
        tk = statistics.median(times[1])
        report(variants[1][0], times[1], f"  -> {n * 5 / tk / 1e6:.0f} GB/s logical "
                                         f"({n * 5 / tk / 1e6 / COPY_GBS * 100:.0f} % of the {COPY_GBS:.0f} GB/s copy rate)")
        gap = min(times[0]) - max(times[1])
        print(f"  torch / kernel = {statistics.median(times[0]) / tk:.2f}x; slowest kernel round is "
              f"{gap * 1e3:.1f} us {'faster' if gap > 0 else 'SLOWER'} than the fastest torch round")
    del x8

    # ---- the fp8 C2 forward: by value against [b, hk] device descales
    q8, qd = xfa.quantize_fp8(x, "head", 1)
    k8, kd = xfa.quantize_fp8(torch.randn(B, S, H, D, device=dev, generator=g).bfloat16(), "head", 1)
    v8, vd = xfa.quantize_fp8(torch.randn(B, S, H, D, device=dev, generator=g).bfloat16(), "head", 1)
    qd.fill_(0.01), kd.fill_(0.011), vd.fill_(0.012)         # equal scales: equal work, equal bits
    out_v = torch.empty(B, S, H, D, device=dev, dtype=torch.bfloat16)
    out_x = torch.empty_like(out_v)
    lse = torch.empty(B, H, S, device=dev)
    fq, fk, fv = (float(t[0, 0]) for t in (qd, kd, vd))
    P = lambda t: t.data_ptr()  # noqa: E731
    tail = (S, S, B, H, H, D, D ** -0.5, -1, 0, False, stream)

    def by_value():
        lib.fmha_fwd_fp8(P(q8), P(k8), P(v8), P(out_v), P(lse), fq, fk, fv, *tail)

    def device():
        lib.fmha_fwd_fp8_ex(P(q8), P(k8), P(v8), P(out_x), P(lse), P(qd), P(kd), P(vd), H, 1, *tail)

    variants = [("fmha_fwd_fp8 (by value)", by_value), ("fmha_fwd_fp8_ex ([b, hk] descales)", device)]
    with step_limit("forward check + warm-up", a.step_timeout):
        for _, fn in variants:
            for _ in range(3):
                fn()
            capi.check()
        torch.cuda.synchronize()
        print(f"forward: fp8 C2 causal, {lib.fmha_last_kernel().decode()}; "
              f"_ex equals by-value bit for bit: {torch.equal(out_v, out_x)}")
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        while True:                                           # ~1 s clock ramp
            for _ in range(5):
                by_value()
            e1.record()
            torch.cuda.synchronize()
            if e0.elapsed_time(e1) > 1000:
                break
    a.iters *= 2
    times, windows = alternate(a, variants, torch.cuda.synchronize)
    fl = 4.0 * B * H * D * S * S * 0.5
    for (name, _), t in zip(variants, times):
        report(name, t, f"  -> {fl / statistics.median(t) / 1e9:.0f} TFLOP/s")
    print(f"  _ex / by-value time = {statistics.median(times[1]) / statistics.median(times[0]):.4f}")
    print(f"  [{clock(monitor, windows)}]")
    return 0


if __name__ == "__main__":
    sys.exit(main())
