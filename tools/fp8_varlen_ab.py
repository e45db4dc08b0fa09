"""In-process, interleaved timing of the packed fp8 forward on the C4 batch (bench.varlen_lengths():
32 sequences, 131072 tokens, H = 32, D = 128, causal) through the C ABI:

  (a) fmha_varlen_fwd_fp8: one launch over the packed batch;
  (b) the same sequences as 32 dense fmha_fwd_fp8 launches (batch 1 each), all a caller could do
      before fmha_varlen_fwd_fp8 existed;
  (c) the bf16 varlen forward (fmha_varlen_fwd_ex) on the same lengths.

HIP-event timing, rounds interleaved on one device so clock drift cancels (as tools/lib_ab.py);
every shape is warmed up and the clock ramped for ~1 s before the timed rounds.  Reports the
median time, TFLOP/s (4 H D sum(s^2) / 2 flop) and the gfx clock over each variant's timed
windows (tools/gpu_monitor.py, started before this process touches the GPU).

Every GPU step (check, warm-up, each timed round) runs under its own time limit: a step that
passes --step-timeout seconds ends the process with status 124 and starts nothing more.  Run the
tool itself under a limit as well:

  timeout -k 10 300 python tools/fp8_varlen_ab.py [--rounds 7] [--iters 40] [--opt name=value]
"""
from __future__ import annotations

import argparse
import itertools
import os
import statistics
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--h", type=int, default=32)
    ap.add_argument("--hk", type=int, default=0)
    ap.add_argument("--opt", action="append", default=[], help="fmha_set_option name=value")
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


def run(a, bench, monitor):
    import torch
    from xf_flash_attention_cutlass_amd import capi

    if not torch.cuda.is_available():
        print("fp8_varlen_ab needs a GPU (nothing is measured without one)")
        return 2
    lib = capi.lib()
    for o in a.opt:
        name, val = o.split("=")
        assert lib.fmha_set_option(name.encode(), int(val)) == 0, lib.fmha_last_error()
    dev = torch.device("cuda", 0)
    if monitor:
        monitor.select(bench.device_info(dev)["pci_bus"])

    lens = bench.varlen_lengths()
    H, HK, D = a.h, a.hk or a.h, 128
    total, n, mx = sum(lens), len(lens), max(lens)
    offs = [0] + list(itertools.accumulate(lens))
    cu = torch.tensor(offs, dtype=torch.int32, device=dev)
    g = torch.Generator(device=dev).manual_seed(0)
    q = torch.randn(total, H, D, device=dev, generator=g)
    k = torch.randn(total, HK, D, device=dev, generator=g)
    v = torch.randn(total, HK, D, device=dev, generator=g)
    q8, k8, v8 = (t.to(torch.float8_e4m3fn) for t in (q, k, v))
    qb, kb, vb = (t.to(torch.bfloat16) for t in (q, k, v))
    del q, k, v
    o_a = torch.empty(total, H, D, device=dev, dtype=torch.bfloat16)
    o_b, o_c = torch.empty_like(o_a), torch.empty_like(o_a)
    lse_a = torch.empty(H, total, device=dev)
    lse_c = torch.empty_like(lse_a)
    lse_b = torch.empty(H * total, device=dev)       # sequence i: [H, s_i] at H * offs[i]
    sc = D ** -0.5
    stream = torch.cuda.current_stream().cuda_stream
    P = lambda t: t.data_ptr()  # noqa: E731

    def run_a():
        lib.fmha_varlen_fwd_fp8(P(q8), P(k8), P(v8), P(o_a), P(lse_a), P(cu), P(cu), None, 1.0, 1.0,
                                1.0, mx, mx, total, n, H, HK, D, sc, -1, 0, False, stream)

    # (pointers taken once: the timed loop of (b) is the 32 C calls alone)
    seq_ptrs = [(P(q8[t0]), P(k8[t0]), P(v8[t0]), P(o_b[t0]), P(lse_b[H * t0:]), s)
                for t0, s in zip(offs, lens)]

    def run_b():
        for pq, pk, pv, po, pl, s in seq_ptrs:
            lib.fmha_fwd_fp8(pq, pk, pv, po, pl, 1.0, 1.0, 1.0, s, s, 1, H, HK, D, sc, -1, 0, False,
                             stream)

    def run_c():
        lib.fmha_varlen_fwd_ex(P(qb), P(kb), P(vb), P(o_c), P(lse_c), P(cu), P(cu), None, None, 0,
                               0, None, 0, mx, mx, total, n, H, HK, D, sc, -1, 0, 0.0, False,
                               stream, 0.0, None)

    variants = [("a: fmha_varlen_fwd_fp8 (1 launch)", run_a),
                (f"b: {n} dense fmha_fwd_fp8 launches", run_b),
                ("c: bf16 fmha_varlen_fwd_ex", run_c)]
    kernels = []
    with step_limit("check", a.step_timeout):
        for _, fn in variants:
            fn()
            capi.check()
            kernels.append(lib.fmha_last_kernel().decode())
        torch.cuda.synchronize()
        same = torch.equal(o_a, o_b)
        dev_c = (o_a.float() - o_c.float()).abs().max().item()
    print(f"lengths: {n} sequences, {total} tokens, max {mx}; H {H}/{HK} D {D} causal")
    for (name, _), kern in zip(variants, kernels):
        print(f"  {name}: {kern}")
    print(f"check: (a) equals (b) bit for bit: {same}; max|a - c| = {dev_c:.3e} (fp8 vs bf16 inputs)")

    fl = sum(4.0 * H * D * s * s * 0.5 for s in lens)
    with step_limit("warm-up", a.step_timeout):
        for _, fn in variants:
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        # ~1 s clock ramp on the variant under test (bench.py does the same)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        while True:
            for _ in range(5):
                run_a()
            e1.record()
            torch.cuda.synchronize()
            if e0.elapsed_time(e1) > 1000:
                break
    times = [[] for _ in variants]
    windows = [[] for _ in variants]
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
                windows[i].append((w0, time.time()))
                times[i].append(s0.elapsed_time(s1) / a.iters)
    capi.check()
    time.sleep(0.3)                                   # let the sampler flush its last samples
    samples = [x for x in monitor.samples() if x.get("gfx_mhz")] if monitor else []

    def clock(wins):
        mhz = [sum(x["gfx_mhz"]) / len(x["gfx_mhz"]) for x in samples
               if any(w0 <= x["t"] <= w1 for w0, w1 in wins)]
        if not mhz:
            return "gfx clock: no sample in the windows"
        return f"gfx {statistics.median(mhz):.0f} MHz (median of {len(mhz)} samples, mean over XCDs)"
    for i, (name, _) in enumerate(variants):
        med = statistics.median(times[i])
        print(f"{name}: median {med:.4f} ms  min {min(times[i]):.4f}  max {max(times[i]):.4f}"
              f"  -> {fl / med / 1e9:.1f} TFLOP/s  [{clock(windows[i])}]")
    print(f"whole timed region: {clock([(windows[0][0][0], windows[-1][-1][1])])}")
    ta, tb = statistics.median(times[0]), statistics.median(times[1])
    print(f"(a) / (b) time = {ta / tb:.3f}  ({'not slower' if ta <= tb else 'SLOWER'} than the dense launches)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
