"""Same-box, interleaved timing of the MLA prefill forward (`flash_attn_varlen_func` with q / k at
head size 192 and v at 128: one fmha_fwd_mla_kernel launch) against the only route the library
had before it: V zero-padded to 192 columns, `flash_attn_varlen_func` at D = 192 (the HD = 256
bucket's 4-wave register-staged kernel), the output sliced back to 128 columns.

  python tools/fwd_mla_ab.py [--shapes all] [--rounds 7] [--iters 5] [--ab-lib PATH]

Contenders, alternating within every round, bf16, packed:
  (a)  the new call;
  (b)  pad + D = 192 forward + slice, the copies inside the timing (what a caller paid);
  (b') the D = 192 forward alone over a V padded once outside the timing, its [.., 192] output kept.
--ab-lib PATH adds the fmha_varlen_fwd_mla entry of another build of the library (e.g. one compiled
with -DXFA_MLA_WAVES=4), both builds called through the C ABI so that the two differ in nothing but
the library; its O and LSE are compared with this build's (max |a - b| / max |b|).  The option may
be repeated: a build and a byte copy of it under another name make a control pair.  The C ABI
contenders rotate their order from round to round.

Shapes (DeepSeek-V3 has 128 heads; 16 is its tensor-parallel-8 share), causal unless said:
  h128_1x8192   128 heads, one sequence of 8192 tokens
  h128_8x2048   128 heads, 8 sequences of 2048 tokens
  h16_4x8192    16 heads, 4 sequences of 8192 tokens
  chunk         128 heads, 2048 new tokens over 30720 cached tokens, non-causal (chunked prefill's
                first pass; merge_attn_states joins it with the causal pass over the new keys)
FLOP = 2 * heads * visible (query, key) pairs * (192 + 128): what the problem needs; the padded
route executes 2 * pairs * (256 + 256) on the MFMAs.  Rates are against the 2.5 PFLOP/s bf16 MFMA
peak of the part.  Times are device events around `iters` back-to-back calls after a ~1 s clock
prewarm; the median over the rounds is printed with the minimum and maximum.
"""
from __future__ import annotations

import argparse
import ctypes as C
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_PFLOPS = 2.5
DQK, DV = 192, 128
# name: (heads, [q lengths], [k lengths], causal)
SHAPES = {
    "h128_1x8192": (128, [8192], [8192], True),
    "h128_8x2048": (128, [2048] * 8, [2048] * 8, True),
    "h16_4x8192": (16, [8192] * 4, [8192] * 4, True),
    "chunk": (128, [2048], [30720], False),
}


def cu(lens):
    out = [0]
    for n in lens:
        out.append(out[-1] + n)
    return torch.tensor(out, dtype=torch.int32, device="cuda")


def measure(a, name):
    import xf_flash_attention_cutlass_amd as xfa
    from xf_flash_attention_cutlass_amd import capi
    h, lq, lk, causal = SHAPES[name]
    dt = torch.bfloat16
    gen = torch.Generator(device="cuda").manual_seed(len(name))
    q = torch.randn(sum(lq), h, DQK, device="cuda", dtype=dt, generator=gen)
    k = torch.randn(sum(lk), h, DQK, device="cuda", dtype=dt, generator=gen)
    v = torch.randn(sum(lk), h, DV, device="cuda", dtype=dt, generator=gen)
    cq, ck, mq, mk = cu(lq), cu(lk), max(lq), max(lk)
    pairs = sum((nq * (nq + 1) // 2 + nq * (nk - nq)) if causal else nq * nk for nq, nk in zip(lq, lk))
    flop = 2.0 * h * pairs * (DQK + DV)
    vp = torch.nn.functional.pad(v, (0, DQK - DV))

    ka, kb, kc = "(a) fwd_mla (192, 128)", "(b) pad V + D=192 forward + slice", "(b') D=192 forward alone"
    runs = {
        ka: lambda: xfa.flash_attn_varlen_func(q, k, v, cq, ck, mq, mk, causal=causal),
        kb: lambda: xfa.flash_attn_varlen_func(q, k, torch.nn.functional.pad(v, (0, DQK - DV)), cq, ck, mq, mk,
                                               causal=causal)[..., :DV].contiguous(),
        kc: lambda: xfa.flash_attn_varlen_func(q, k, vp, cq, ck, mq, mk, causal=causal),
    }
    if a.ab_lib:
        o_c = torch.empty(sum(lq), h, DV, device="cuda", dtype=dt)
        st = (C.c_int64 * 8)(q.stride(0), q.stride(1), k.stride(0), k.stride(1), v.stride(0), v.stride(1),
                             o_c.stride(0), o_c.stride(1))
        stream = capi.stream_handle()

        def c_abi(L, lse=None):
            args = (q.data_ptr(), k.data_ptr(), v.data_ptr(), o_c.data_ptr(), lse, cq.data_ptr(), ck.data_ptr(),
                    None, mq, mk, sum(lq), len(lq), h, h, DQK, DV, st, DQK ** -0.5, -1, 0 if causal else -1, False,
                    stream)
            return lambda: L.fmha_varlen_fwd_mla(*args)

        builds = {"this build": capi.lib(), **{path: capi.load(path, strict=False) for path in a.ab_lib}}
        # O and LSE of the other builds against this one's (lib_ab.py's check line)
        lse_c = torch.empty(h, sum(lq), device="cuda", dtype=torch.float32)
        ref = None
        for path, L in builds.items():
            runs[f"(a) C ABI, {path}"] = c_abi(L)
            o_c.zero_()
            lse_c.zero_()
            c_abi(L, lse_c.data_ptr())()
            torch.cuda.synchronize()
            outs = (o_c.float().clone(), lse_c.clone())
            if ref is None:
                ref = outs
                continue
            print(f"check {os.path.basename(path)} vs this build: " + " ".join(
                f"{n}:{(x - r).abs().max().item():.3e}/{r.abs().max().item():.2e}"
                for n, x, r in zip(("o", "lse"), outs, ref)))
        del ref, outs, lse_c
    kern = {}
    with torch.no_grad():
        o_a = runs[ka]()
        kern[ka] = capi.lib().fmha_last_kernel().decode()
        o_b = runs[kb]()
        kern[kb] = capi.lib().fmha_last_kernel().decode()
        torch.cuda.synchronize()
        print(f"check {name}: max|(a) - (b)| {(o_a.float() - o_b.float()).abs().max().item():.3e}  "
              f"(a) [{kern[ka]}]  (b) [{kern[kb]}]")
        del o_a, o_b
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
        cabi = [nm for nm in runs if nm.startswith("(a) C ABI")]
        for r in range(a.rounds):
            # the C ABI builds take turns at the place behind (b'): the call that follows the slower
            # D = 192 kernel measures 1 - 2 % longer whichever build it is
            turn = cabi[r % len(cabi):] + cabi[:r % len(cabi)] if cabi else []
            for nm in [nm for nm in runs if nm not in cabi] + turn:
                run = runs[nm]
                s0, s1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s0.record()
                for _ in range(a.iters):
                    run()
                s1.record()
                torch.cuda.synchronize()
                times[nm].append(s0.elapsed_time(s1) / a.iters)
    print(f"MLA prefill {name}: heads={h} q={lq[0]}x{len(lq)} k={lk[0]}x{len(lk)} causal={causal} bf16: "
          f"{flop / 1e12:.3f} TFLOP needed per call")
    med = {}
    for nm, t in times.items():
        med[nm] = statistics.median(t)
        pf = flop / med[nm] / 1e12
        print(f"  {nm}: median {med[nm]:.3f} ms  min {min(t):.3f}  max {max(t):.3f}  -> {pf * 1e3:.0f} TFLOP/s needed-work "
              f"rate = {pf / PEAK_PFLOPS:.2f} of {PEAK_PFLOPS} PFLOP/s")
    print(f"  (b)/(a) {med[kb] / med[ka]:.2f}x  (b')/(a) {med[kc] / med[ka]:.2f}x  "
          f"(a) beats (b') outside both spreads: {max(times[ka]) < min(times[kc])}")
    del q, k, v, vp
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["all"], help="names of SHAPES, or all")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--ab-lib", action="append", default=[],
                    help="another build of the library to time fmha_varlen_fwd_mla of (may be repeated, e.g. the "
                         "parent's build and a byte copy of it as the control pair)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "fwd_mla_ab.py measures on the GPU"
    prop = torch.cuda.get_device_properties(0)
    print(f"device: {prop.name}, {prop.multi_processor_count} CUs, clock_rate {getattr(prop, 'clock_rate', 0) / 1e3:.0f} MHz "
          f"(the driver's maximum; the run's own clocks are ramped by a prewarm before every timed window)")
    for name in (list(SHAPES) if a.shapes == ["all"] else a.shapes):
        measure(a, name)


if __name__ == "__main__":
    main()
