"""Same-box, interleaved timing of the MLA decode (`flash_mla_with_kvcache`, one
fmha_mla_decode_kernel launch plus the split combine) against the same attention composed from
torch eager ops over the gathered cache, at several split counts.

  python tools/mla_ab.py [--b 8] [--s 32768] [--page 64] [--heads 16 128] [--splits 0 ...]
                         [--rounds 7] [--iters 20] [--fp8] [--append 8192]
  python tools/mla_ab.py --sparse [--topk 2048] [--b 8 64] [--heads 16 128] [--fp8]

--sparse times the decode over index-selected tokens (`indices=`, fmha_mla_decode_sparse[_fp8]_kernel)
at topk entries per query over sequences of --s cached tokens, the indices a random subset of each
sequence, sorted ascending and unsorted, against (b) what the library offered before - index_select
of the rows into a temporary cache, an identity block table, the dense decode - with and without the
gather in the timing, and (c) the dense decode over topk contiguous keys of the same cache; all at the
sparse call's split count.  bytes = b * topk * row bytes + the indices + q + o.
--ab-lib PATH adds the sparse entry of another build of the library (e.g. one compiled with
-DXFA_MLA_SPARSE_NT=0: plain instead of non-temporal cache-row loads), both builds called through
the C ABI so that the two differ in nothing but the library.

--fp8 adds the fp8-cache call (fmha_mla_decode_fp8_kernel over rows of 656 bytes, the same tokens
appended with mla_cache_append_fp8) as a contender of every split count, next to the 16-bit-cache
call of the same build, and an eager contender over the dequantised gathered cache; its bytes are
n * 656 + q + o.  --append N times the append kernel alone on N tokens (bytes read + written).

Per head count (seqlen_q = 1, bf16, uniform lengths):
  bytes = sum n * 1152 (every cache row once) + q + o;  rate in TB/s against the 6.29 TB/s a
          streaming copy reaches on this part;
  FLOP  = 2 * b * heads * s * (576 + 512);              rate against the 2.5 PFLOP/s bf16 MFMA peak.
16 heads is one 16-row tile per sequence (the HBM-bound, tensor-parallel shape); 128 heads sits near
the ridge of the two bounds.  The eager contender reads a cache gathered once outside the timing
(it has no paged form) and materialises the scores.  Times are device events around `iters`
back-to-back calls, the contenders alternating within every round; the median over rounds is
printed.  There is no earlier kernel of this library to compare against: nothing else in it runs
head size 576.
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

STREAM_TBS = 6.29
PEAK_PFLOPS = 2.5
D, DV = 576, 512


def eager(q, kg, scale):
    """q [b, 1, h, 576], kg [b, s, 576] (gathered) -> o [b, 1, h, 512] in q's dtype."""
    s = torch.einsum("bqhd,bsd->bhqs", q, kg).float() * scale
    p = torch.softmax(s, dim=-1).to(q.dtype)
    return torch.einsum("bhqs,bsd->bqhd", p, kg[..., :DV])


def measure(a, heads):
    import xf_flash_attention_cutlass_amd as xfa
    from xf_flash_attention_cutlass_amd import capi
    dt = torch.bfloat16
    b, s, page = a.b, a.s, a.page
    per = s // page
    gen = torch.Generator(device="cuda").manual_seed(heads)
    kv = torch.randn(b * per, page, 1, D, device="cuda", dtype=dt, generator=gen)
    table = torch.randperm(b * per, device="cuda", generator=gen).to(torch.int32).view(b, per)
    lens = torch.full((b,), s, dtype=torch.int32, device="cuda")
    q = torch.randn(b, 1, heads, D, device="cuda", dtype=dt, generator=gen)
    out = torch.empty(b, 1, heads, DV, device="cuda", dtype=dt)
    kg = kv[table.long()].reshape(b, s, D)
    scale = D ** -0.5
    qo = q.numel() * 2 + out.numel() * 2
    nbytes = {"": b * s * D * 2 + qo}
    flop = 2.0 * b * heads * s * (D + DV)

    def mla(cache, ns):
        return lambda: xfa.flash_mla_with_kvcache(q, cache, table, lens, num_splits=ns, out=out)

    caches, refs = {"mla_decode": kv}, {"mla_decode": eager(q, kg, scale)}
    if a.fp8:
        # the same tokens in an fp8 cache, written by the append kernel through the same table
        kv8 = torch.zeros(b * per, page, 1, xfa.mla_fp8_cache_row_bytes, device="cuda", dtype=torch.uint8)
        flat = kv.view(-1, D)
        xfa.mla_cache_append_fp8(flat[:, :DV], flat[:, DV:], kv8, torch.arange(flat.shape[0], device="cuda"))
        r8 = kv8.view(-1, xfa.mla_fp8_cache_row_bytes)
        ds = r8[:, 512:528].contiguous().view(torch.float32).repeat_interleave(128, dim=1)
        lat = (r8[:, :DV].contiguous().view(torch.float8_e4m3fn).float() * ds).to(dt)
        kdq = torch.cat([lat, r8[:, 528:].contiguous().view(dt)], 1).view(b * per, page, D)
        kg8 = kdq[table.long()].reshape(b, s, D)
        caches["mla_decode_fp8"], refs["mla_decode_fp8"] = kv8, eager(q, kg8, scale)
        nbytes["fp8"] = b * s * xfa.mla_fp8_cache_row_bytes + qo
        del r8, ds, lat, kdq
    runs, kern = {}, {}
    for ns in a.splits:
        for op, cache in caches.items():
            name = f"{op} num_splits={ns}"
            runs[name] = mla(cache, ns)
            out.zero_()
            runs[name]()
            torch.cuda.synchronize()
            kern[name] = "%s splits=%d" % (capi.lib().fmha_last_kernel().decode(), capi.lib().fmha_last_num_splits())
            print(f"check {name}: max|o - eager| {(out.float() - refs[op].float()).abs().max().item():.3e}  [{kern[name]}]")
    runs["torch eager (gathered cache)"] = lambda: eager(q, kg, scale)
    if a.fp8:
        runs["torch eager (dequantised gathered cache)"] = lambda: eager(q, kg8, scale)
    del refs

    for run in runs.values():
        for _ in range(3):
            run()
    torch.cuda.synchronize()
    first = next(iter(runs.values()))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    k = 0
    while True:                                           # ~1 s clock-ramp prewarm
        first()
        k += 1
        if k % 20 == 0:
            e1.record()
            torch.cuda.synchronize()
            if e0.elapsed_time(e1) > 1000:
                break
    times = {name: [] for name in runs}
    for _ in range(a.rounds):
        for name, run in runs.items():
            s0, s1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s0.record()
            for _ in range(a.iters):
                run()
            s1.record()
            torch.cuda.synchronize()
            times[name].append(s0.elapsed_time(s1) / a.iters)
    print(f"MLA decode b={b} s_kv={s} page={page} heads={heads} seqlen_q=1 bf16: {nbytes[''] / 1e6:.1f} MB "
          + (f"(fp8 cache {nbytes['fp8'] / 1e6:.1f} MB), " if a.fp8 else "") + f"{flop / 1e9:.1f} GFLOP per call")
    for name, t in times.items():
        med = statistics.median(t)
        nb = nbytes["fp8" if name.startswith("mla_decode_fp8") else ""]     # bytes the call actually reads
        tbs, pf = nb / med / 1e9, flop / med / 1e12
        print(f"{name}: median {med * 1e3:.1f} us  min {min(t) * 1e3:.1f}  max {max(t) * 1e3:.1f}  -> "
              f"{tbs:.2f} TB/s = {tbs / STREAM_TBS:.2f} of {STREAM_TBS} TB/s;  {pf:.3f} PFLOP/s = "
              f"{pf / PEAK_PFLOPS:.2f} of {PEAK_PFLOPS} PFLOP/s")
    del kv, kg, caches
    torch.cuda.empty_cache()


def measure_sparse(a, b, fp8):
    """The sparse decode against the composition and the dense ceiling, for one batch size and cache."""
    import xf_flash_attention_cutlass_amd as xfa
    from xf_flash_attention_cutlass_amd import capi
    dt = torch.bfloat16
    s, page, topk = a.s, a.page, a.topk
    assert topk % page == 0 and topk <= s
    per = s // page
    gen = torch.Generator(device="cuda").manual_seed(b)
    kv = torch.randn(b * per, page, 1, D, device="cuda", dtype=dt, generator=gen)
    table = torch.randperm(b * per, device="cuda", generator=gen).to(torch.int32).view(b, per)
    row = D * 2
    cache = kv
    if fp8:
        row = xfa.mla_fp8_cache_row_bytes
        cache = torch.zeros(b * per, page, 1, row, device="cuda", dtype=torch.uint8)
        flat = kv.view(-1, D)
        xfa.mla_cache_append_fp8(flat[:, :DV], flat[:, DV:], cache, torch.arange(flat.shape[0], device="cuda"))
        del kv, flat
    rows = cache.view(b * s, -1)
    ident = torch.arange(b * topk // page, device="cuda", dtype=torch.int32).view(b, topk // page)
    lens_k = torch.full((b,), topk, dtype=torch.int32, device="cuda")
    name_c = "fp8" if fp8 else "16-bit"
    for order in ("sorted", "unsorted"):
        tok = torch.stack([torch.randperm(s, device="cuda", generator=gen)[:topk] for _ in range(b)])
        if order == "sorted":
            tok = tok.sort(dim=1).values
        slot = table.long().gather(1, tok // page) * page + tok % page
        ind, ind64 = slot.to(torch.int32).view(b, 1, topk), slot.view(-1)
        for heads in a.heads:
            q = torch.randn(b, 1, heads, D, device="cuda", dtype=dt, generator=gen)
            o_a, o_b, o_c = (torch.empty(b, 1, heads, DV, device="cuda", dtype=dt) for _ in range(3))
            xfa.flash_mla_with_kvcache(q, cache, None, None, out=o_a, indices=ind)
            torch.cuda.synchronize()
            ns = capi.lib().fmha_last_num_splits()
            kern = capi.lib().fmha_last_kernel().decode()
            tmp = rows.index_select(0, ind64).view(b * topk // page, page, 1, -1)
            ka, kb, kg, kc = ("(a) sparse", "(b) index_select + dense", "(b') dense over the gathered cache",
                              "(c) dense over contiguous keys")
            runs = {
                ka: lambda: xfa.flash_mla_with_kvcache(q, cache, None, None, out=o_a, indices=ind),
                kb: lambda: xfa.flash_mla_with_kvcache(
                    q, rows.index_select(0, ind64).view(b * topk // page, page, 1, -1), ident, lens_k,
                    num_splits=ns, out=o_b),
                kg: lambda: xfa.flash_mla_with_kvcache(
                    q, tmp, ident, lens_k, num_splits=ns, out=o_b),
                kc: lambda: xfa.flash_mla_with_kvcache(
                    q, cache, table, lens_k, num_splits=ns, out=o_c),
            }
            if a.ab_lib:
                import ctypes as C
                st = (C.c_int64 * 6)(q.stride(0), q.stride(1), q.stride(2), o_a.stride(0), o_a.stride(1), o_a.stride(2))
                stream = capi.stream_handle()

                def c_abi(L, o):
                    fn = L.fmha_mla_decode_sparse_fp8 if fp8 else L.fmha_mla_decode_sparse
                    args = (q.data_ptr(), cache.data_ptr(), o.data_ptr(), None, ind.data_ptr(), ind.stride(0),
                            ind.stride(1), topk, 1, b, heads, D, DV, cache.shape[0], page, st, D ** -0.5, 0, False,
                            stream)
                    return lambda: fn(*args)

                runs["(a) sparse, C ABI, this build"] = c_abi(capi.lib(), o_a)
                runs[f"(a) sparse, C ABI, {os.path.basename(a.ab_lib)}"] = c_abi(capi.load(a.ab_lib, strict=False), o_c)
            for run in runs.values():
                for _ in range(3):
                    run()
            torch.cuda.synchronize()
            same = torch.equal(o_a, o_b)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            k = 0
            while True:                                       # ~0.5 s clock-ramp prewarm
                runs[ka]()
                k += 1
                if k % 20 == 0:
                    e1.record()
                    torch.cuda.synchronize()
                    if e0.elapsed_time(e1) > 500:
                        break
            times = {name: [] for name in runs}
            for _ in range(a.rounds):
                for name, run in runs.items():
                    s0, s1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    s0.record()
                    for _ in range(a.iters):
                        run()
                    s1.record()
                    torch.cuda.synchronize()
                    times[name].append(s0.elapsed_time(s1) / a.iters)
            nb = b * topk * row + ind.numel() * 4 + q.numel() * 2 + o_a.numel() * 2
            print(f"sparse MLA decode {name_c} cache b={b} s_kv={s} topk={topk} {order} page={page} heads={heads}: "
                  f"{nb / 1e6:.2f} MB per call, splits={ns} [{kern}], (a) == (b) bit for bit: {same}")
            med = {}
            for name, t in times.items():
                med[name] = statistics.median(t)
                tbs = nb / med[name] / 1e9
                print(f"  {name}: median {med[name] * 1e3:.1f} us  min {min(t) * 1e3:.1f}  max {max(t) * 1e3:.1f}  -> "
                      f"{tbs:.2f} TB/s = {tbs / STREAM_TBS:.2f} of {STREAM_TBS} TB/s")
            print(f"  (a)/(b) {med[ka] / med[kb]:.2f}  (a)/(b') {med[ka] / med[kg]:.2f}  (a)/(c) {med[ka] / med[kc]:.2f}  "
                  f"(a) beats (b) outside both spreads: {max(times[ka]) < min(times[kb])}")
            del tmp
    del cache, rows
    torch.cuda.empty_cache()


def measure_append(a):
    """The append kernel alone: `a.append` tokens (two views of one 576-wide tensor) into an fp8
    cache through a shuffled slot_mapping; bytes = tokens * (1152 read + 8 slot + 656 written)."""
    import xf_flash_attention_cutlass_amd as xfa
    n, page = a.append, a.page
    blocks = (n + page - 1) // page
    gen = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn(n, D, device="cuda", dtype=torch.bfloat16, generator=gen)
    slots = torch.randperm(blocks * page, device="cuda", generator=gen)[:n].contiguous()
    kv8 = torch.zeros(blocks, page, 1, xfa.mla_fp8_cache_row_bytes, device="cuda", dtype=torch.uint8)
    run = lambda: xfa.mla_cache_append_fp8(x[:, :DV], x[:, DV:], kv8, slots)  # noqa: E731
    for _ in range(20):
        run()
    torch.cuda.synchronize()
    times = []
    for _ in range(a.rounds):
        s0, s1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s0.record()
        for _ in range(a.iters):
            run()
        s1.record()
        torch.cuda.synchronize()
        times.append(s0.elapsed_time(s1) / a.iters)
    med = statistics.median(times)
    nb = n * (D * 2 + 8 + xfa.mla_fp8_cache_row_bytes)
    print(f"mla_cache_append_fp8 tokens={n} page={page}: median {med * 1e3:.1f} us  min {min(times) * 1e3:.1f}  "
          f"max {max(times) * 1e3:.1f}  -> {nb / 1e6:.1f} MB read + written, {nb / med / 1e9:.2f} TB/s = "
          f"{nb / med / 1e9 / STREAM_TBS:.2f} of {STREAM_TBS} TB/s (launch-bound at this size: back-to-back calls)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--b", type=int, nargs="+", default=[8])
    ap.add_argument("--s", type=int, default=32768)
    ap.add_argument("--page", type=int, default=64)
    ap.add_argument("--heads", type=int, nargs="+", default=[16, 128])
    ap.add_argument("--splits", type=int, nargs="+", default=[0, 16, 32, 64],
                    help="num_splits values to time (0 = the library's choice)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--fp8", action="store_true", help="add the fp8-cache call and its eager contender")
    ap.add_argument("--append", type=int, default=0, help="also time mla_cache_append_fp8 on this many tokens")
    ap.add_argument("--sparse", action="store_true", help="time the sparse decode (indices=) against the "
                    "index_select + dense composition and the dense decode over topk contiguous keys")
    ap.add_argument("--topk", type=int, default=2048, help="entries per query of --sparse")
    ap.add_argument("--ab-lib", default="", help="--sparse: another build of the library to time the sparse "
                    "entry of, next to this build's, both through the C ABI")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "mla_ab.py measures on the GPU"
    assert a.s % a.page == 0
    prop = torch.cuda.get_device_properties(0)
    print(f"device: {prop.name}, {prop.multi_processor_count} CUs, clock_rate {getattr(prop, 'clock_rate', 0) / 1e3:.0f} MHz "
          f"(the driver's maximum; the run's own clocks are ramped by a prewarm before every timed window)")
    if a.sparse:
        for b in a.b:
            for fp8 in ((False, True) if a.fp8 else (False,)):
                measure_sparse(a, b, fp8)
        return
    batches, a.b = a.b, a.b[0]
    for a.b in batches:
        for heads in a.heads:
            measure(a, heads)
    if a.append:
        measure_append(a)


if __name__ == "__main__":
    main()
