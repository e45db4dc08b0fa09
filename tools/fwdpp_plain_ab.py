"""In-process alternating A/B of library builds (tools/lib_ab.py's method: one device, one process,
the arms interleaved round by round, cdna_hip_programming.md §5.4 rule 24) over the workloads the
plain ping-pong body (fwd_plain) is judged by:

  c2        mha_fwd B 4, H 32, S 4096, D 128 bf16 causal (bench.py's default)
  c4        mha_varlen_fwd, bench.py's 32 ragged sequences (131072 tokens), causal
  c2_2048   the C2 shape causal with sq 2048, sk 4096
  alibi     C2 causal with ALiBi          } controls: these launches run the full / paged body
  window    C2 with window (1023, 0)      } in every arm
  paged     C2 causal over 16-key pages   }

  python tools/fwdpp_plain_ab.py libA.so libB.so[@name=val,...] [--rounds 7] [--iters 10] [--only c2,c4]

Per workload and arm: the kernel id, TFLOP/s as median and min - max over the rounds, and the
median ms.  Each path is loaded as its own library (copied to a distinct name, so two arms of one
build keep separate option states).
"""
from __future__ import annotations

import argparse
import os
import shutil
import statistics
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV, DT = "cuda", torch.bfloat16
B, H, S, D = 4, 32, 4096, 128
SC = D ** -0.5


def load(spec, i):
    from xf_flash_attention_cutlass_amd import capi
    path, _, opts = spec.partition("@")
    tmp = os.path.join(tempfile.mkdtemp(), f"arm{i}_" + os.path.basename(path))
    shutil.copy(path, tmp)
    lib = capi.load(tmp, strict=False)
    for o in (x for x in opts.split(",") if x):
        name, val = o.split("=")
        assert lib.fmha_set_option(name.encode(), int(val)) == 0, lib.fmha_last_error()
    return lib


def causal_flops(sq, sk, h):
    """4 D per visible (query, key) pair of a bottom-right aligned causal mask, per head"""
    vis = sum(min(sk, p + sk - sq + 1) for p in range(sq))
    return 4.0 * D * h * vis


def workloads(only):
    from bench import varlen_lengths
    st = torch.cuda.current_stream().cuda_stream
    P = lambda t: t.data_ptr()  # noqa: E731
    g = torch.Generator(device=DEV).manual_seed(0)
    rn = lambda *s: torch.randn(*s, device=DEV, dtype=DT, generator=g)  # noqa: E731
    q, k, v = rn(B, S, H, D), rn(B, S, H, D), rn(B, S, H, D)
    o = torch.empty_like(q)
    lse = torch.empty(B, H, S, device=DEV, dtype=torch.float32)
    slopes = torch.linspace(0.01, 0.5, B * H, device=DEV).view(B, H).contiguous()
    W = {}

    def dense(sq, wl, wr, alibi=None):
        return lambda L: L.fmha_fwd(P(q), P(k), P(v), P(o), alibi, sq, S, B, H, H, D, 0.0, st, None, SC, None,
                                    P(lse), wl, wr, 0.0, False, False, 1)
    W["c2"] = (dense(S, -1, 0), B * causal_flops(S, S, H))
    W["c2_2048"] = (dense(2048, -1, 0), B * causal_flops(2048, S, H))
    W["alibi"] = (dense(S, -1, 0, P(slopes)), B * causal_flops(S, S, H))
    W["window"] = (dense(S, 1023, 0), 4.0 * D * H * B * sum(min(p + 1, 1024) for p in range(S)))
    if not only or "c4" in only:
        lens = varlen_lengths()
        cu = torch.tensor([0] + list(torch.tensor(lens).cumsum(0)), dtype=torch.int32, device=DEV)
        tot = sum(lens)
        qv, kv, vv = rn(tot, H, D), rn(tot, H, D), rn(tot, H, D)
        ov = torch.empty_like(qv)
        lv = torch.empty(H, tot, device=DEV, dtype=torch.float32)
        W["c4"] = (lambda L: L.fmha_varlen_fwd_ex(P(qv), P(kv), P(vv), P(ov), P(lv), P(cu), P(cu), None, None, 0, 0,
                                                  None, 0, max(lens), max(lens), tot, len(lens), H, H, D, SC, -1, 0,
                                                  0.0, False, st, 0.0, None),
                   sum(causal_flops(n, n, H) for n in lens))
    if not only or "paged" in only:
        page = 16
        nbp = S // page
        table = torch.randperm(B * nbp, device=DEV, generator=g).to(torch.int32).view(B, nbp).contiguous()
        kc, vc = rn(B * nbp, page, H, D), rn(B * nbp, page, H, D)
        sl = torch.full((B,), S, dtype=torch.int32, device=DEV)
        W["paged"] = (lambda L: L.fmha_page_kvcache_fwd_ex(P(q), P(kc), P(vc), P(o), P(lse), P(table), nbp, P(sl), S,
                                                           S, B, H, H, D, page, SC, -1, 0, 0.0, None, 0, 1, 0, 1.0,
                                                           1.0, None, False, st), B * causal_flops(S, S, H))
    order = ["c2", "c4", "c2_2048", "alibi", "window", "paged"]
    return {n: W[n] for n in order if n in W and (not only or n in only)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("libs", nargs="+")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    libs = [load(s, i) for i, s in enumerate(a.libs)]
    names = [f"{'ABCDEFGH'[i]}={s}" for i, s in enumerate(a.libs)]
    only = [x for x in a.only.split(",") if x]
    for wname, (run, fl) in workloads(only).items():
        kern = []
        for L in libs:
            for _ in range(3):
                run(L)
            assert L.fmha_last_status() == 0, L.fmha_last_error()
            kern.append(L.fmha_last_kernel().decode())
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()                              # ~1 s of the same work first: the clock settles
        while True:
            for _ in range(20):
                run(libs[0])
            e1.record()
            torch.cuda.synchronize()
            if e0.elapsed_time(e1) > 1000:
                break
        ms = [[] for _ in libs]
        for _ in range(a.rounds):
            for i, L in enumerate(libs):
                s0, s1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s0.record()
                for _ in range(a.iters):
                    run(L)
                s1.record()
                torch.cuda.synchronize()
                ms[i].append(s0.elapsed_time(s1) / a.iters)
        print(f"{wname}: {a.rounds} alternations x {a.iters} launches")
        for i, n in enumerate(names):
            tf = sorted(fl / t / 1e9 for t in ms[i])
            print(f"  {n}: {statistics.median(tf):7.1f} TFLOP/s  ({tf[0]:.1f} - {tf[-1]:.1f})  "
                  f"median {statistics.median(ms[i]):.4f} ms   [{kern[i]}]")
        base = statistics.median(ms[0])
        for i in range(1, len(libs)):
            print(f"  {names[i].split('=')[0]} / A: {100 * (base / statistics.median(ms[i]) - 1):+.2f} % (medians)")
        sys.stdout.flush()


if __name__ == "__main__":
    main()
