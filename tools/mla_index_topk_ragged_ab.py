"""MLA indexer, the selection for prefill rows: fmha_mla_index_topk_ragged (a) against what there was
before it for the same call - (b) torch.topk over the -inf-cleaned rows plus the slot gather, and,
where the launch is one causal sequence from column 0, (c) mla_index_topk at batch 1, seqlen_q M -
on logits that come from the real ragged logits kernel on random inputs.  One GPU; device events
around back-to-back calls, the contenders alternating in the same rounds after a warm-up; median and
min-max of the rounds.  topk 2048.

  python tools/mla_index_topk_ragged_ab.py [--rounds 7] [--variant NAME=PATH ...]
  python tools/mla_index_topk_ragged_ab.py --make-variants DIR        (no GPU: builds the A/B libraries)

--variant: another build of the library (same C ABI) timed in the same rounds.  --make-variants
builds the design's alternatives into DIR/<name>.so from the product's objects and one recompiled
unit: waves8 / waves16 (workgroup size), bits12 / bits8 (first digit), nocompact (every pass from
global memory), forward (blockIdx r is row r).
"""
import argparse
import importlib.util
import os
import statistics
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
VARIANTS = {"waves8": ["-DXFA_RAGTOPK_WAVES=8"], "waves16": ["-DXFA_RAGTOPK_WAVES=16"],
            "bits12": ["-DXFA_RAGTOPK_BITS0=12"], "bits8": ["-DXFA_RAGTOPK_BITS0=8"],
            "nocompact": ["-DXFA_RAGTOPK_COMPACT=0"], "forward": ["-DXFA_RAGTOPK_REVERSE=0"]}
HEADS, PAGE, TOPK = 64, 64, 2048
DEV = "cuda"


def make_variants(out_dir):
    spec = importlib.util.spec_from_file_location("b", os.path.join(ROOT, "xf_flash_attention_cutlass_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    b.build_lib()
    os.makedirs(out_dir, exist_ok=True)
    unit = "fmha_mla_index_topk_ragged"
    rest = [os.path.join(b.OBJ, n) for n in sorted(os.listdir(b.OBJ)) if n.endswith(".o") and n != unit + ".o"]
    for name, defs in VARIANTS.items():
        obj = os.path.join(out_dir, name + ".o")
        subprocess.run([b.HIPCC, *b.HIP_FLAGS, "-Xclang", "-target-feature", "-Xclang", "-packed-fp32-ops", *defs, "-c",
                        os.path.join(b.CSRC, unit + ".hip"), "-o", obj], check=True)
        subprocess.run([b.HIPCC, f"--offload-arch={b.ARCH}", "-shared", "-fPIC", "-o", os.path.join(out_dir, name + ".so"),
                        obj, *rest], check=True)
        os.remove(obj)
        print("built", os.path.join(out_dir, name + ".so"), flush=True)


def timed(fn, reps):
    import torch
    a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    z.record()
    z.synchronize()
    return a.elapsed_time(z) * 1e-3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--variant", action="append", default=[], help="NAME=PATH of another build of the library")
    ap.add_argument("--make-variants", default="", help="build the A/B libraries into this directory and exit")
    a = ap.parse_args()
    if a.make_variants:
        return make_variants(a.make_variants)
    import torch
    sys.path.insert(0, ROOT)
    import xf_flash_attention_cutlass_amd as xfa
    from xf_flash_attention_cutlass_amd import capi
    if not torch.cuda.is_available():
        sys.exit("mla_index_topk_ragged_ab.py measures on a GPU: none found")
    libs = [("ragged kernel", capi.lib())] + [(n, capi.load(p, strict=False)) for n, p in (v.split("=", 1) for v in a.variant)]
    print(f"{torch.cuda.get_device_name(0)}; {capi.lib().fmha_version().decode()}; heads {HEADS}, topk {TOPK}; "
          f"{a.rounds} rounds", flush=True)
    packed = [512 + (8192 - 512) * i // 7 for i in range(8)]
    shapes = [("M 4096 over N 4096, one causal sequence", [4096], 4096),
              ("M 4096 over N 32768, a chunk over cached keys", [4096], 32768),
              (f"8 packed sequences of {packed[0]}..{packed[-1]} rows", packed, sum(packed))]
    for name, lens, n in shapes:
        g = torch.Generator(device=DEV).manual_seed(0)
        m = sum(lens)
        q8 = torch.randn(m, HEADS, 128, generator=g, device=DEV).to(torch.float8_e4m3fn)
        w = torch.randn(m, HEADS, generator=g, device=DEV) / 8
        k8 = torch.randn(n, 128, generator=g, device=DEV).to(torch.float8_e4m3fn)
        scale = torch.rand(n, generator=g, device=DEV) + 0.5
        if len(lens) == 1:                                    # bottom-right causal from column 0
            ks, ke = torch.zeros(m, dtype=torch.int32, device=DEV), (torch.arange(m, device=DEV) + n - m + 1).int()
        else:
            start = torch.repeat_interleave(torch.tensor([sum(lens[:i]) for i in range(len(lens))]), torch.tensor(lens))
            ks, ke = start.int().to(DEV), (torch.arange(m, device=DEV) + 1).int()
        logits = xfa.mla_index_logits_ragged(q8, w, k8, scale, ks, ke)
        del q8, w, k8, scale
        table = torch.randperm(-(-n // PAGE), generator=g, device=DEV).int()[None]
        pos = torch.arange(n, device=DEV)
        slots = table[0, pos // PAGE].long() * PAGE + pos % PAGE
        out = torch.empty(m, TOPK, dtype=torch.int32, device=DEV)

        def lib_call(lib):
            args = (logits.data_ptr(), logits.stride(0), ks.data_ptr(), ke.data_ptr(), slots.data_ptr(), out.data_ptr(),
                    out.stride(0), TOPK, m, n, capi.stream_handle())
            return lambda: lib.fmha_mla_index_topk_ragged(*args)

        def glue():
            val, col = torch.topk(logits, min(TOPK, n), dim=1)
            return torch.where(val == float("-inf"), torch.full_like(col, -1), slots[col]).int()

        runs = [(nm, lib_call(L), 5) for nm, L in libs] + [("torch glue", glue, 1)]
        if len(lens) == 1:
            lens_d, out3 = torch.tensor([n], dtype=torch.int32, device=DEV), out.view(1, m, TOPK).clone()
            runs.append(("decode kernel", lambda: xfa.mla_index_topk(logits, table, lens_d, TOPK, seqlen_q=m,
                                                                     page_block_size=PAGE, out=out3), 5))
        runs[0][1]()
        same = torch.equal(out.sort(-1).values, glue().sort(-1).values)
        note = "" if len(lens) > 1 else f" and {'equals' if torch.equal(runs[-1][1]()[0], out) else 'DIFFERS FROM'} the decode kernel's result"
        print(f"{name}: the kernel's set {'equals' if same else 'DIFFERS FROM'} torch.topk's (ties aside){note}", flush=True)
        for _, fn, reps in runs:
            timed(fn, reps)                                    # warm-up
        ts = {nm: [] for nm, _, _ in runs}
        for _ in range(a.rounds):
            for nm, fn, reps in runs:
                ts[nm].append(timed(fn, reps))
        cand = int((ke.clamp(0, n) - ks.clamp(0, n)).clamp(min=0).sum())
        for nm, _, _ in runs:
            med = statistics.median(ts[nm])
            rate = f"  {4 * cand / med / 1e12:.3f} TB/s of candidates" if nm not in ("torch glue",) else ""
            print(f"  {nm:<14} median {med * 1e6:10.1f} us  (min {min(ts[nm]) * 1e6:.1f}, max {max(ts[nm]) * 1e6:.1f}){rate}", flush=True)
        a_max, b_min = max(ts["ragged kernel"]), min(ts["torch glue"])
        print(f"  max(ragged kernel) {'<' if a_max < b_min else '>= (BAR MISSED)'} min(torch glue): "
              f"{a_max * 1e6:.1f} us vs {b_min * 1e6:.1f} us", flush=True)
        del logits, out, slots, runs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
