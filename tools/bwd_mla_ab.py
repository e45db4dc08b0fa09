"""Same-box, interleaved timing of the MLA prefill backward (`paged_attn.varlen_bwd_mla`: q / k at
head size 192, v at 128; three launches, no atomics) against the only route the library had before
it: V, O and dO zero-padded to 192 columns, `paged_attn.varlen_bwd` at D = 192 (the HD = 256
bucket's 4-wave kernel with fp32 dQ atomics), dV sliced back to 128 columns.

  python tools/bwd_mla_ab.py [--shapes all] [--rounds 7] [--iters 5]

Contenders, alternating within every round in one process on one build, bf16, packed, causal:
  (a)  varlen_bwd_mla;
  (b)  pad V, O, dO + varlen_bwd at D = 192 + slice of dV, the copies inside the timing (what a
       caller paid);
  (b') that backward alone on inputs padded once outside the timing.
Shapes (the forward table's three causal ones; DeepSeek-V3 has 128 heads, 16 is its
tensor-parallel-8 share):
  h128_1x8192   128 heads, one sequence of 8192 tokens
  h128_8x2048   128 heads, 8 sequences of 2048 tokens
  h16_4x8192    16 heads, 4 sequences of 8192 tokens
FLOP = 1664 per visible (query, key) pair and head = 2 (3 x 192 + 2 x 128): what the problem
needs; (a) executes 2304 (S and dP are computed by both of its kernels), the padded route 2560.
Rates are against the 2.5 PFLOP/s bf16 MFMA peak of the part.  Times are device events around
`iters` back-to-back calls after a ~1 s clock prewarm; per contender the median over the rounds
with its minimum and maximum, and the clock and power torch reports right after its last window
(where the driver exposes them).
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_PFLOPS = 2.5
DQK, DV = 192, 128
FLOP_PER_PAIR = 2 * (3 * DQK + 2 * DV)
# name: (heads, [q lengths], [k lengths])
SHAPES = {
    "h128_1x8192": (128, [8192], [8192]),
    "h128_8x2048": (128, [2048] * 8, [2048] * 8),
    "h16_4x8192": (16, [8192] * 4, [8192] * 4),
}


def cu(lens):
    out = [0]
    for n in lens:
        out.append(out[-1] + n)
    return torch.tensor(out, dtype=torch.int32, device="cuda")


def gauges():
    """(clock MHz, power W) as torch reports them, or None where the driver does not"""
    res = []
    for fn in (torch.cuda.clock_rate, torch.cuda.power_draw):
        try:
            res.append(fn())
        except Exception:
            res.append(None)
    return res[0], (None if res[1] is None else res[1] / 1e3)


def measure(a, name):
    import xf_flash_attention_cutlass_amd as xfa
    from xf_flash_attention_cutlass_amd import capi
    pa = xfa.paged_attn
    h, lq, lk = SHAPES[name]
    dt = torch.bfloat16
    gen = torch.Generator(device="cuda").manual_seed(len(name))
    q = torch.randn(sum(lq), h, DQK, device="cuda", dtype=dt, generator=gen)
    k = torch.randn(sum(lk), h, DQK, device="cuda", dtype=dt, generator=gen)
    v = torch.randn(sum(lk), h, DV, device="cuda", dtype=dt, generator=gen)
    g = torch.randn(sum(lq), h, DV, device="cuda", dtype=dt, generator=gen)
    cq, ck, mq, mk = cu(lq), cu(lk), max(lq), max(lk)
    scale = DQK ** -0.5
    pairs = sum(nq * (nq + 1) // 2 + nq * (nk - nq) for nq, nk in zip(lq, lk))
    flop = float(h) * pairs * FLOP_PER_PAIR
    pad = lambda x: torch.nn.functional.pad(x, (0, DQK - DV))      # noqa: E731

    out, lse = pa.varlen_fwd_mla(q, k, v, None, cq, ck, None, mq, mk, scale, True, -1, 0)
    fw = pa.varlen_fwd(q, k, pad(v), None, cq, ck, None, None, None, mq, mk, 0.0, scale, False, True, -1, 0,
                       0.0, False, None)
    lse_p, rng = fw[5], fw[7]
    vp, op, gp = pad(v), pad(out), pad(g)

    def padded(vv, oo, gg):
        return pa.varlen_bwd(gg, q, k, vv, oo, lse_p, None, None, None, cq, ck, None, mq, mk, 0.0, scale, False,
                             True, -1, 0, 0.0, False, None, rng)

    def route_b():
        dq, dk, dv, _ = padded(pad(v), pad(out), pad(g))
        return dq, dk, dv[..., :DV].contiguous()

    ka, kb, kc = "(a) varlen_bwd_mla (192, 128)", "(b) pad V, O, dO + D=192 backward + slice", "(b') D=192 backward alone"
    runs = {
        ka: lambda: pa.varlen_bwd_mla(g, q, k, v, out, lse, None, None, None, cq, ck, mq, mk, scale, True, -1, 0)[:3],
        kb: route_b,
        kc: lambda: padded(vp, op, gp)[:3],
    }
    with torch.no_grad():
        ga = runs[ka]()
        kern = capi.lib().fmha_last_kernel().decode()
        gb = runs[kb]()
        torch.cuda.synchronize()
        diff = [(x.float() - y.float()).abs().max().item() for x, y in zip(ga, gb)]
        print(f"check {name}: max|(a) - (b)| dq {diff[0]:.3e} dk {diff[1]:.3e} dv {diff[2]:.3e}  (a) [{kern}]")
        del ga, gb
        for run in runs.values():
            for _ in range(2):
                run()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        n = 0
        while True:                                           # ~1 s clock-ramp prewarm
            runs[ka]()
            n += 1
            if n % 5 == 0:
                e1.record()
                torch.cuda.synchronize()
                if e0.elapsed_time(e1) > 1000:
                    break
        times = {nm: [] for nm in runs}
        gauge = {}
        for _ in range(a.rounds):
            for nm, run in runs.items():
                s0, s1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s0.record()
                for _ in range(a.iters):
                    run()
                s1.record()
                torch.cuda.synchronize()
                times[nm].append(s0.elapsed_time(s1) / a.iters)
                gauge[nm] = gauges()
    print(f"MLA prefill backward {name}: heads={h} q={lq[0]}x{len(lq)} k={lk[0]}x{len(lk)} causal bf16: "
          f"{flop / 1e12:.3f} TFLOP needed per call")
    med = {}
    for nm, t in times.items():
        med[nm] = statistics.median(t)
        pf = flop / med[nm] / 1e12
        mhz, watt = gauge[nm]
        print(f"  {nm}: median {med[nm]:.3f} ms  min {min(t):.3f}  max {max(t):.3f}  spread "
              f"{(max(t) - min(t)) / med[nm] * 100:.1f} %  -> {pf * 1e3:.0f} TFLOP/s needed-work rate = "
              f"{pf / PEAK_PFLOPS:.2f} of {PEAK_PFLOPS} PFLOP/s"
              + (f"  clock {mhz} MHz" if mhz is not None else "  clock n/a")
              + (f"  power {watt:.0f} W" if watt is not None else "  power n/a"))
    print(f"  (b)/(a) {med[kb] / med[ka]:.2f}x  (b')/(a) {med[kc] / med[ka]:.2f}x  "
          f"(a) beats (b') outside both spreads: {max(times[ka]) < min(times[kc])}")
    del q, k, v, g, vp, op, gp, out, fw
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["all"], help="names of SHAPES, or all")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bwd_mla_ab.py measures on the GPU"
    prop = torch.cuda.get_device_properties(0)
    print(f"device: {prop.name}, {prop.multi_processor_count} CUs, clock_rate {getattr(prop, 'clock_rate', 0) / 1e3:.0f} MHz "
          f"(the driver's maximum; the run's own clocks are ramped by a prewarm before every timed window)")
    for name in (list(SHAPES) if a.shapes == ["all"] else a.shapes):
        measure(a, name)


if __name__ == "__main__":
    main()
