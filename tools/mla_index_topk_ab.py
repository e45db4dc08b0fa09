"""MLA indexer, the selection: mla_index_topk (one HIP launch, fmha_mla_index_topk_kernel) against
mla_index_topk_slots (torch.topk and the glue around it) on the same logits, which come from the
real logits kernel on random inputs (the indexer's value distribution, not a uniform one).  One
GPU; device events around back-to-back calls, the contenders alternating in the same rounds after
a warm-up, the round's first contender rotating; median and min-max of the rounds.  mla_index_logits is timed beside them: the two
together are the indexer's cost per decode step.

  python tools/mla_index_topk_ab.py [--rounds 7] [--variant NAME=PATH ...] [--splits CHUNK,CHUNK,...]

--variant: another build of the library (same C ABI) timed in the same rounds.  Bytes of a call:
the visible logits, 4 bytes each, against the project's measured copy rate (6.29 TB/s).
--splits: fmha_mla_index_topk_split (this build, pooled scratch) as further contenders, one for
each target chunk length: ceil(keys / CHUNK) workgroups a row, where the entry's limits allow that
(2 .. 16 workgroups, at most 32768 candidates a row); its result is compared with the kernel's.
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import xf_flash_attention_cutlass_amd as xfa  # noqa: E402
from xf_flash_attention_cutlass_amd import capi  # noqa: E402

HEADS, PAGE, TOPK, COPY_RATE = 64, 64, 2048, 6.29e12
DEV = "cuda"


def problem(lens, sq, seed=0):
    """The index cache of `lens` keys a sequence, q and weights; returns what mla_index_logits takes."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    batch, keys = len(lens), -(-max(lens) // PAGE) * PAGE
    nblk = batch * keys // PAGE
    cache = torch.empty(nblk, PAGE * 132, dtype=torch.uint8, device=DEV)
    cache[:, :PAGE * 128] = torch.randn(nblk, PAGE * 128, generator=g, device=DEV).to(torch.float8_e4m3fn).view(torch.uint8)
    cache[:, PAGE * 128:] = (torch.rand(nblk, PAGE, generator=g, device=DEV) + 0.5).view(torch.uint8)
    table = torch.randperm(nblk, generator=g, device=DEV).int().view(batch, keys // PAGE)
    q8 = torch.randn(batch, sq, HEADS, 128, generator=g, device=DEV).to(torch.float8_e4m3fn)
    w = torch.randn(batch * sq, HEADS, generator=g, device=DEV) / 8
    return q8, w, cache, table, torch.tensor(lens, dtype=torch.int32, device=DEV), keys


def lib_call(lib, logits, table, lens, out, sq, keys, nblk):
    args = (logits.data_ptr(), logits.stride(0), table.data_ptr(), table.stride(0), lens.data_ptr(), out.data_ptr(),
            out.stride(1), TOPK, sq, keys, len(lens), nblk, PAGE, capi.stream_handle())
    return lambda: lib.fmha_mla_index_topk(*args)


def split_call(lib, splits, logits, table, lens, out, sq, keys, nblk):
    args = (logits.data_ptr(), logits.stride(0), table.data_ptr(), table.stride(0), lens.data_ptr(), out.data_ptr(),
            out.stride(1), TOPK, sq, keys, len(lens), nblk, PAGE, splits, None, 0, capi.stream_handle())
    return lambda: lib.fmha_mla_index_topk_split(*args)


def timed(fn, reps):
    a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    z.record()
    z.synchronize()
    return a.elapsed_time(z) * 1e-3 / reps


def report(name, ts, nbytes=None):
    med = statistics.median(ts)
    rate = "" if nbytes is None else f"  {nbytes / med / 1e12:.3f} TB/s = {100 * nbytes / med / COPY_RATE:.1f} % of the copy rate"
    print(f"  {name:<14} median {med * 1e6:9.1f} us  (min {min(ts) * 1e6:.1f}, max {max(ts) * 1e6:.1f}){rate}", flush=True)
    return med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--variant", action="append", default=[], help="NAME=PATH of another build of the library")
    ap.add_argument("--splits", default="", help="target chunk lengths of the split contenders, e.g. 8192,16384,32768")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("mla_index_topk_ab.py measures on a GPU: none found")
    libs = [("topk kernel", capi.lib())] + [(n, capi.load(p, strict=False)) for n, p in (v.split("=", 1) for v in a.variant)]
    print(f"{torch.cuda.get_device_name(0)}; {capi.lib().fmha_version().decode()}; heads {HEADS}, page {PAGE}, "
          f"topk {TOPK}; {a.rounds} rounds", flush=True)
    ragged = [1024 + (32768 - 1024) * i // 63 for i in range(64)]
    shapes = [(f"batch {b} seqlen_q {sq}, {k} keys", [k] * b, sq)
              for k, bs, sqs in ((32768, (8, 64), (1, 2)), (40960, (8,), (1,)), (65536, (8,), (1,)), (131072, (8,), (1, 2)), (131072, (64,), (1,)),
                                (65536, (256,), (1,)))
              for b in bs for sq in sqs]
    shapes.append(("batch 64 seqlen_q 1, ragged 1024..32768 keys", ragged, 1))
    for name, lens, sq in shapes:
        q8, w, cache, table, lens_d, keys = problem(lens, sq)
        logits = xfa.mla_index_logits(q8, w, cache, table, lens_d, keys)
        out = torch.empty(len(lens), sq, TOPK, dtype=torch.int32, device=DEV)
        runs = [(n, lib_call(L, logits, table, lens_d, out, sq, keys, cache.shape[0]), 20) for n, L in libs]
        for chunk in (int(c) for c in a.splits.split(",") if c):
            splits = -(-keys // chunk)
            if not (2 <= splits <= 16 and splits * TOPK <= 32768 and (-(-keys // splits) + 3) // 4 * 4 <= 32768):
                continue
            split_out = torch.empty_like(out)
            runs.append((f"split x{splits}", split_call(capi.lib(), splits, logits, table, lens_d, split_out, sq, keys,
                                                        cache.shape[0]), 20))
            runs[0][1](), runs[-1][1]()
            if not torch.equal(out, split_out):
                print(f"{name}: split x{splits} DIFFERS FROM the kernel's result", flush=True)
        runs.append(("torch glue", lambda: xfa.mla_index_topk_slots(logits, table, lens_d, TOPK, sq, PAGE), 5))
        runs.append(("index logits", lambda: xfa.mla_index_logits(q8, w, cache, table, lens_d, keys, out=logits), 20))
        runs[0][1]()
        same = torch.equal(out.sort(-1).values, runs[-2][1]().sort(-1).values)
        print(f"{name}: the kernel's set {'equals' if same else 'DIFFERS FROM'} torch.topk's (ties aside)", flush=True)
        print(f"  (splits=None: x{xfa.interface.mla_index_topk_splits(keys, TOPK, len(lens) * sq)})", flush=True)
        for _, fn, reps in runs:
            timed(fn, reps)                                # warm-up
        ts = {n: [] for n, _, _ in runs}
        for i in range(a.rounds):                          # (who follows whom changes with the round: a contender
            for n, fn, reps in runs[i % len(runs):] + runs[:i % len(runs)]:   # behind the logits kernel finds the logits evicted)
                ts[n].append(timed(fn, reps))
        vis = sum(max(0, n - sq + i + 1) for n in lens for i in range(sq))
        med = {n: report(n, ts[n], 4 * vis if n not in ("torch glue", "index logits") else None) for n, _, _ in runs}
        print(f"  topk kernel / torch glue = {med['topk kernel'] / med['torch glue']:.4f}; "
              f"logits + topk kernel = {(med['index logits'] + med['topk kernel']) * 1e6:.1f} us a step", flush=True)
        del q8, w, cache, table, lens_d, logits, out, runs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
