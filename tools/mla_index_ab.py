"""MLA indexer: fmha_mla_index_logits against the only route there was before it (gather the
sequence's blocks, dequantise, einsum, relu, weighted head sum in torch), and the index-key cache
append's rate.  One GPU; device events around back-to-back calls, the contenders alternating in the
same rounds after a warm-up; median and min-max of the rounds.

  python tools/mla_index_ab.py [--rounds 7] [--variant NAME=PATH ...] [--no-torch]

--variant: another build of the library (same C ABI, e.g. compiled with -DXFA_MLA_INDEX_AHEAD=3 or
-DXFA_MLA_INDEX_CHUNK=2048) timed in the same rounds.  Bytes of a call: keys * 132 + q + weights +
logits, against the project's measured copy rate (6.29 TB/s).
"""
import argparse
import ctypes as C
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from xf_flash_attention_cutlass_amd import capi  # noqa: E402

HEADS, PAGE, KEYS, COPY_RATE = 64, 64, 32768, 6.29e12
DEV = "cuda"


def problem(batch, sq, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    nblk = batch * KEYS // PAGE
    cache = torch.empty(nblk, PAGE * 132, dtype=torch.uint8, device=DEV)
    keys = (torch.randn(nblk, PAGE, 128, generator=g, device=DEV)).to(torch.float8_e4m3fn).view(torch.uint8)
    cache[:, :PAGE * 128] = keys.flatten(1)
    cache[:, PAGE * 128:] = (torch.rand(nblk, PAGE, generator=g, device=DEV) + 0.5).view(torch.uint8).flatten(1)
    table = torch.randperm(nblk, generator=g, device=DEV).int().view(batch, KEYS // PAGE)
    q8 = torch.randn(batch, sq, HEADS, 128, generator=g, device=DEV).to(torch.float8_e4m3fn)
    w = torch.randn(batch * sq, HEADS, generator=g, device=DEV) / 8
    lens = torch.full((batch,), KEYS, dtype=torch.int32, device=DEV)
    return cache, table, q8, w, lens


def lib_call(lib, cache, table, q8, w, lens, out):
    b, sq = q8.shape[:2]
    st = (C.c_int64 * 3)(q8.stride(0), q8.stride(1), q8.stride(2))
    args = (q8.data_ptr(), w.data_ptr(), cache.data_ptr(), out.data_ptr(), table.data_ptr(), table.stride(0),
            lens.data_ptr(), sq, KEYS, b, HEADS, 128, cache.shape[0], PAGE, st, out.stride(0), capi.stream_handle())

    def run():
        lib.fmha_mla_index_logits(*args)
    return run


def torch_call(cache, table, q8, w, lens):
    b, sq = q8.shape[:2]
    idx = table.long()                                     # (index preparation is outside the timing)
    row = torch.arange(KEYS, device=DEV)
    mask = (row[None, None, :] > (KEYS - sq + torch.arange(sq, device=DEV))[None, :, None]).expand(b, sq, KEYS)

    def run():
        blocks = cache[idx]                                # [b, blocks, page * 132]
        k = blocks[..., :PAGE * 128].reshape(b, KEYS, 128).view(torch.float8_e4m3fn).float()
        ds = blocks[..., PAGE * 128:].reshape(b, KEYS * 4).view(torch.float32)
        s = torch.einsum("bqhd,bsd->bqhs", q8.float(), k).relu_()
        out = (s * w.view(b, sq, HEADS, 1)).sum(2) * ds[:, None, :]
        return out.masked_fill_(mask, float("-inf")).view(b * sq, KEYS)
    return run


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
    rate = "" if nbytes is None else f"  {nbytes / med / 1e12:.2f} TB/s = {100 * nbytes / med / COPY_RATE:.0f} % of the copy rate"
    print(f"  {name:<14} median {med * 1e6:9.1f} us  (min {min(ts) * 1e6:.1f}, max {max(ts) * 1e6:.1f}){rate}", flush=True)
    return med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--variant", action="append", default=[], help="NAME=PATH of another build of the library")
    ap.add_argument("--no-torch", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("mla_index_ab.py measures on a GPU: none found")
    libs = [("library", capi.lib())] + [(n, capi.load(p, strict=False)) for n, p in (v.split("=", 1) for v in a.variant)]
    print(f"{torch.cuda.get_device_name(0)}; {capi.lib().fmha_version().decode()}; heads {HEADS}, page {PAGE}, "
          f"{KEYS} keys a sequence; {a.rounds} rounds", flush=True)
    for batch in (8, 64):
        for sq in (1, 2):
            cache, table, q8, w, lens = prob = problem(batch, sq)
            out = torch.empty(batch * sq, KEYS, device=DEV)
            runs = [(n, lib_call(L, *prob, out), 20) for n, L in libs]
            if not a.no_torch:
                runs.append(("torch", torch_call(*prob), 2))
                err = (runs[0][1]() or out) - runs[-1][1]()
                print(f"batch {batch} seqlen_q {sq}: max |library - torch| {err.nan_to_num(0, 0, 0).abs().max().item():.3e}")
            else:
                print(f"batch {batch} seqlen_q {sq}:")
            for _, fn, reps in runs:
                timed(fn, reps)                            # warm-up
            ts = {n: [] for n, _, _ in runs}
            for _ in range(a.rounds):
                for n, fn, reps in runs:
                    ts[n].append(timed(fn, reps))
            nbytes = batch * KEYS * 132 + q8.numel() + 4 * w.numel() + 4 * out.numel()
            med = {n: report(n, ts[n], None if n == "torch" else nbytes) for n, _, _ in runs}
            if "torch" in med:
                print(f"  library / torch = {med['library'] / med['torch']:.4f}", flush=True)
            del prob, cache, table, q8, w, lens, out, runs
            torch.cuda.empty_cache()
    import xf_flash_attention_cutlass_amd as xfa
    n = 8192
    k = torch.randn(n, 128, device=DEV).bfloat16()
    icache = torch.zeros(n // PAGE, PAGE * 132, dtype=torch.uint8, device=DEV)
    slots = torch.randperm(n, device=DEV)
    for fmt in (None, "ue8m0"):
        fn = lambda: xfa.mla_index_cache_append_fp8(k, icache, slots, fmt)  # noqa: E731
        timed(fn, 50)
        ts = [timed(fn, 200) for _ in range(a.rounds)]
        print(f"append, {n} tokens, scale_fmt {fmt}:")
        report("append", ts, n * (256 + 132 + 8))


if __name__ == "__main__":
    main()
