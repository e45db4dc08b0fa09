"""MLA indexer, prefill: fmha_mla_index_logits_ragged (a) against the two routes there were before it:
(b) fmha_mla_index_logits at batch 1, seqlen_q = M over a paged cache holding the same keys (single
causal sequences only) and (c) torch (dequantise, einsum in row chunks, relu, weighted head sum,
scale, mask; index preparation outside the timing).  One GPU; device events around back-to-back
calls, the contenders alternating in the same rounds after a warm-up; median and min-max of the
rounds.  The method of tools/mla_index_ab.py.

  python tools/mla_index_ragged_ab.py [--rounds 7] [--variant NAME=PATH ...] [--no-torch]

--variant: another build of the library (same C ABI, e.g. compiled with -DXFA_MLA_RAGGED_ROWS=4 or
-DXFA_MLA_RAGGED_CHUNK=2048) timed in the same rounds.  FLOP of a call: the visible (row, key)
pairs x heads x 128 x 2, the work the problem needs, against the 5 PFLOP/s fp8 MFMA peak.
"""
import argparse
import ctypes as C
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from xf_flash_attention_cutlass_amd import capi  # noqa: E402

HEADS, PAGE, PEAK = 64, 64, 5e15
DEV = "cuda"
F8 = torch.float8_e4m3fn


def causal(seqs, cached=0):
    """ks / ke of packed causal sequences of the given lengths, the first behind `cached` keys."""
    ks, ke, at = [], [], 0
    for i, n in enumerate(seqs):
        first = cached if i == 0 else 0
        ks.append(torch.full((n,), at, dtype=torch.int32))
        ke.append(at + first + 1 + torch.arange(n, dtype=torch.int32))
        at += first + n
    return torch.cat(ks).to(DEV), torch.cat(ke).to(DEV), at


SHAPES = [("one causal sequence of 4096", [4096], 0), ("one causal sequence of 8192", [8192], 0),
          ("4 x 2048 packed", [2048] * 4, 0), ("2048 new rows over 32768 keys", [2048], 32768 - 2048)]


def ragged_call(lib, q8, w, k8, scale, ks, ke, out):
    st = (C.c_int64 * 2)(q8.stride(0), q8.stride(1))
    args = (q8.data_ptr(), w.data_ptr(), k8.data_ptr(), scale.data_ptr(), ks.data_ptr(), ke.data_ptr(), out.data_ptr(),
            q8.shape[0], k8.shape[0], HEADS, 128, st, k8.stride(0), out.stride(0), capi.stream_handle())
    return lambda: lib.fmha_mla_index_logits_ragged(*args)


def paged_call(lib, q8, w, k8, scale, out):
    """(b): the same keys in a paged cache behind a shuffled table, one sequence of N keys, M positions"""
    m, n = q8.shape[0], k8.shape[0]
    nblk = n // PAGE
    perm = torch.randperm(nblk, device=DEV)
    cache = torch.empty(nblk, PAGE * 132, dtype=torch.uint8, device=DEV)
    cache[perm, :PAGE * 128] = k8.view(torch.uint8).view(nblk, PAGE * 128)
    cache[perm, PAGE * 128:] = scale.view(nblk, PAGE).view(torch.uint8)
    table, lens = perm.int().view(1, nblk), torch.tensor([n], dtype=torch.int32, device=DEV)
    st = (C.c_int64 * 3)(0, q8.stride(0), q8.stride(1))
    keep = (cache, table, lens)
    args = (q8.data_ptr(), w.data_ptr(), cache.data_ptr(), out.data_ptr(), table.data_ptr(), nblk, lens.data_ptr(),
            m, n, 1, HEADS, 128, nblk, PAGE, st, out.stride(0), capi.stream_handle())
    return lambda: (lib.fmha_mla_index_logits(*args), keep)[0]


def torch_call(q8, w, k8, scale, ks, ke, rows=256):
    n = k8.shape[0]
    col = torch.arange(n, device=DEV)[None, :]
    dead = (col < ks[:, None]) | (col >= ke[:, None])          # (index preparation is outside the timing)

    def run():
        k = k8.float()
        out = torch.empty(q8.shape[0], n, device=DEV)
        for r in range(0, q8.shape[0], rows):
            s = torch.einsum("qhd,sd->qhs", q8[r:r + rows].float(), k).relu_()
            out[r:r + rows] = (s * w[r:r + rows, :, None]).sum(1) * scale[None, :]
        return out.masked_fill_(dead, float("-inf"))
    return run


def timed(fn, reps):
    a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    z.record()
    z.synchronize()
    return a.elapsed_time(z) * 1e-3 / reps


def report(name, ts, flop):
    med = statistics.median(ts)
    print(f"  {name:<22} median {med * 1e6:10.1f} us  (min {min(ts) * 1e6:.1f}, max {max(ts) * 1e6:.1f})  "
          f"{flop / med / 1e12:8.1f} TFLOP/s = {100 * flop / med / PEAK:.1f} % of the fp8 peak", flush=True)
    return med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--variant", action="append", default=[], help="NAME=PATH of another build of the library")
    ap.add_argument("--no-torch", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("mla_index_ragged_ab.py measures on a GPU: none found")
    libs = [("ragged", capi.lib())] + [(n, capi.load(p, strict=False)) for n, p in (v.split("=", 1) for v in a.variant)]
    print(f"{torch.cuda.get_device_name(0)}; {capi.lib().fmha_version().decode()}; heads {HEADS}; {a.rounds} rounds", flush=True)
    for name, seqs, cached in SHAPES:
        g = torch.Generator(device=DEV).manual_seed(0)
        ks, ke, n = causal(seqs, cached)
        m = ks.numel()
        q8 = torch.randn(m, HEADS, 128, generator=g, device=DEV).to(F8)
        k8 = torch.randn(n, 128, generator=g, device=DEV).to(F8)
        w, scale = torch.randn(m, HEADS, generator=g, device=DEV) / 8, torch.rand(n, generator=g, device=DEV) + 0.5
        out, out_b = torch.empty(m, n, device=DEV), torch.empty(m, n, device=DEV)
        flop = float((ke.long() - ks.long()).sum()) * HEADS * 128 * 2
        runs = [(nm, ragged_call(L, q8, w, k8, scale, ks, ke, out), 5) for nm, L in libs]
        if len(seqs) == 1:
            runs.append(("paged, seqlen_q = M", paged_call(capi.lib(), q8, w, k8, scale, out_b), 2))
        if not a.no_torch:
            runs.append(("torch", torch_call(q8, w, k8, scale, ks, ke), 1))
        print(f"{name}: M {m}, N {n}, {flop:.3e} FLOP needed")
        runs[0][1]()
        for nm, fn, _ in runs[len(libs):]:                     # the other routes compute the same thing
            other = fn()
            other = other if torch.is_tensor(other) else out_b
            live = ~out.isinf()
            same = torch.equal(out.isinf(), other.isinf())
            print(f"  ragged vs {nm}: -inf pattern equal {same}, max |diff| {(out - other)[live].abs().max().item():.3e}")
        for _, fn, reps in runs:
            timed(fn, reps)                                    # warm-up
        ts = {nm: [] for nm, _, _ in runs}
        for _ in range(a.rounds):
            for nm, fn, reps in runs:
                ts[nm].append(timed(fn, reps))
        med = {nm: report(nm, ts[nm], flop) for nm, _, _ in runs}
        for nm in list(med)[1:]:
            print(f"  ragged / {nm} = {med['ragged'] / med[nm]:.4f}", flush=True)
        del runs, q8, k8, w, scale, out, out_b
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
