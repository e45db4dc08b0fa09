"""Launch decisions of one build of libpaged-attention.so: a fixed list of small calls through the
C ABI, one line per call with the entry, the case, fmha_last_status(), fmha_last_num_splits(),
fmha_last_kernel() and the sha256 of O and of the LSE (backward: of dQ / dK / dV, deterministic
mode only; the atomic sums differ in the last bits from run to run).  Two builds that decide and
compute the same print the same text:

  python tools/launch_trace.py libA.so > a.txt; python tools/launch_trace.py libB.so > b.txt

The cases are sized so that b x kv heads x row blocks crosses the CU count with the smallest
tensors; they ask for one pass (num_splits = 1) except the split-KV and decode cases (0: the
library's choice).  Stops at the first failing call (exit status 1).
"""
from __future__ import annotations

import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from xf_flash_attention_cutlass_amd import capi  # noqa: E402

DEV = "cuda"
BF, F8 = torch.bfloat16, torch.float8_e4m3fn
P = lambda t: None if t is None else t.data_ptr()  # noqa: E731
_cache = {}


def rand(key, *shape, dtype=BF, scale=1.0):
    """the same tensor for the same key in every run (CPU generator)"""
    if key not in _cache:
        g = torch.Generator().manual_seed(int(hashlib.sha256(repr(key).encode()).hexdigest()[:8], 16))
        _cache[key] = (torch.randn(*shape, generator=g) * scale).to(dtype).to(DEV)
    return _cache[key]


def sha(*ts):
    torch.cuda.synchronize()
    return " ".join(hashlib.sha256(t.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()[:16]
                    for t in ts)


def ragged(n, hi, seed):
    lens = torch.randint(1, hi + 1, (n,), generator=torch.Generator().manual_seed(seed))
    cu = torch.zeros(n + 1, dtype=torch.int32)
    cu[1:] = lens.cumsum(0)
    return lens.to(torch.int32).to(DEV), cu.to(DEV), int(lens.sum()), int(lens.max())


class Trace:
    def __init__(self, path):
        self.L = capi.load(path, strict=False)
        self.st = torch.cuda.current_stream().cuda_stream
        self.knobs = ""

    def line(self, entry, case, *outs, fwd=True):
        L = self.L
        status = L.fmha_last_status()
        kern = f"splits={L.fmha_last_num_splits()} kernel=[{L.fmha_last_kernel().decode()}] " if fwd else ""
        print(f"{entry} {case}{self.knobs}: status={status} {kern}sha={sha(*outs) if outs and status == 0 else '-'}", flush=True)
        if status != 0:
            print("FAILED:", L.fmha_last_error().decode(), flush=True)
            sys.exit(1)

    # ---- entries
    def fwd(self, case, b=4, s=2304, sk=None, h=8, hk=8, d=128, wl=-1, wr=0, alibi=False, softcap=0.0,
            p=0.0, splits=1, strided=False):
        sk = sk or s
        if strided:            # every second head of a tensor with 2 h heads
            q, k, v = (rand(("s" + n, b, sl, hh, d), b, sl, 2 * hh, d)[:, :, ::2] for n, sl, hh in
                       (("q", s, h), ("k", sk, hk), ("v", sk, hk)))
        else:
            q, k, v = (rand((n, b, sl, hh, d), b, sl, hh, d) for n, sl, hh in (("q", s, h), ("k", sk, hk), ("v", sk, hk)))
        o = torch.zeros(b, s, h, d, dtype=BF, device=DEV)
        lse = torch.zeros(b, h, s, dtype=torch.float32, device=DEV)
        al = rand(("alibi", b, h), b, h, dtype=torch.float32, scale=0.05).abs() if alibi else None
        self.L.fmha_set_rng_state(1234, 16)
        if strided:
            import ctypes
            st = (ctypes.c_int64 * 12)(*[t.stride(i) for t in (q, k, v, o) for i in (0, 1, 2)])
            self.L.fmha_fwd_strided(P(q), P(k), P(v), P(o), P(al), P(lse), s, sk, b, h, hk, d, st, d ** -0.5,
                                    wl, wr, softcap, False, splits, self.st, p, None)
        else:
            self.L.fmha_fwd(P(q), P(k), P(v), P(o), P(al), s, sk, b, h, hk, d, p, self.st, None, d ** -0.5,
                            None, P(lse), wl, wr, softcap, False, False, splits)
        self.line("fmha_fwd_strided" if strided else "fmha_fwd", case, o, lse)
        return q, k, v, o, lse

    def paged(self, case, b=8, sq=1, s=4096, h=32, hk=8, d=128, page=16, fp8=False, rag=False, wl=-1, wr=0,
              splits=0):
        nb = b * s // page
        table = torch.randperm(nb, generator=torch.Generator().manual_seed(3)).to(torch.int32).view(b, s // page).to(DEV)
        q = rand(("pq", b, sq, h, d), b, sq, h, d)
        kc, vc = (rand((n, nb, page, hk, d, fp8), nb, page, hk, d, dtype=F8 if fp8 else BF) for n in ("kc", "vc"))
        lens = ragged(b, s, 5)[0] if rag else torch.full((b,), s, dtype=torch.int32, device=DEV)
        o = torch.zeros_like(q)
        lse = torch.zeros(b, h, sq, dtype=torch.float32, device=DEV)
        self.L.fmha_page_kvcache_fwd_ex(P(q), P(kc), P(vc), P(o), P(lse), P(table), s // page, P(lens), sq, s,
                                        b, h, hk, d, page, d ** -0.5, wl, wr, 0.0, None, 0, splits, int(fp8),
                                        0.5, 0.5, None, False, self.st)
        self.line("fmha_page_kvcache_fwd_ex", case, o, lse)

    def varlen(self, case, n=40, hi=1024, h=8, hk=8, d=128, seqused=False, fp8=False):
        lens, cu, total, mx = ragged(n, hi, 7)
        dt = F8 if fp8 else BF
        q, k, v = (rand((nm, total, hh, d, fp8), total, hh, d, dtype=dt) for nm, hh in (("vq", h), ("vk", hk), ("vv", hk)))
        o = torch.zeros(total, h, d, dtype=BF, device=DEV)
        lse = torch.zeros(h, total, dtype=torch.float32, device=DEV)
        used = (lens - lens // 3).to(torch.int32) if seqused else None
        if fp8:
            self.L.fmha_varlen_fwd_fp8(P(q), P(k), P(v), P(o), P(lse), P(cu), P(cu), P(used), 1.0, 1.0, 1.0, mx,
                                       mx, total, n, h, hk, d, d ** -0.5, -1, 0, False, self.st)
        else:
            self.L.fmha_varlen_fwd_ex(P(q), P(k), P(v), P(o), P(lse), P(cu), P(cu), P(used), None, 0, 0, None, 0,
                                      mx, mx, total, n, h, hk, d, d ** -0.5, -1, 0, 0.0, False, self.st, 0.0, None)
        self.line("fmha_varlen_fwd_fp8" if fp8 else "fmha_varlen_fwd_ex", case, o, lse)
        return q, k, v, o, lse, cu, total, mx

    def fp8(self, case, b=4, s=2304, h=8, hk=8, d=128, wl=-1, wr=0):
        q, k, v = (rand((n, b, s, hh, d), b, s, hh, d, dtype=F8) for n, hh in (("8q", h), ("8k", hk), ("8v", hk)))
        o = torch.zeros(b, s, h, d, dtype=BF, device=DEV)
        lse = torch.zeros(b, h, s, dtype=torch.float32, device=DEV)
        self.L.fmha_fwd_fp8(P(q), P(k), P(v), P(o), P(lse), 1.0, 1.0, 1.0, s, s, b, h, hk, d, d ** -0.5, wl, wr,
                            False, self.st)
        self.line("fmha_fwd_fp8", case, o, lse)

    def bwd(self, d, det, packed):
        h = 8
        case = f"d{d} {'deterministic' if det else 'atomic'}"
        if packed:
            q, k, v, o, lse, cu, total, mx = self.varlen(f"for the backward d{d}", n=6, hi=512, d=d)
        else:
            q, k, v, o, lse = self.fwd(f"for the backward d{d}", b=2, s=512, d=d)
        do = rand(("do", tuple(o.shape)), *o.shape)
        dq, dk, dv = torch.zeros_like(q), torch.zeros_like(k), torch.zeros_like(v)
        if packed:
            self.L.fmha_varlen_bwd(P(do), P(q), P(k), P(v), P(o), P(lse), P(dq), P(dk), P(dv), P(cu), P(cu), None,
                                   0, mx, mx, total, total, 6, h, h, d, d ** -0.5, -1, 0, 0.0, det, False,
                                   self.st, None, 0, None, 0.0)
        else:
            self.L.fmha_bwd(P(do), P(q), P(k), P(v), P(o), P(lse), P(dq), P(dk), P(dv), None, None, 512, 512, 2,
                            h, h, d, 0.0, d ** -0.5, -1, 0, 0.0, det, False, self.st, None, 0)
        torch.cuda.synchronize()
        self.line("fmha_varlen_bwd" if packed else "fmha_bwd", case, *((dq, dk, dv) if det else ()), fwd=False)

    def swept(self):
        """the cases every knob sweep repeats"""
        self.fwd("causal")
        self.fwd("non-causal", wr=-1)
        self.varlen("40 ragged")
        self.fp8("causal")
        self.varlen("40 ragged", fp8=True)

    def run(self):
        self.swept()
        self.fwd("window (255, 0)", wl=255)
        self.fwd("non-causal alibi", wr=-1, alibi=True)
        self.fwd("non-causal softcap", wr=-1, softcap=30.0)
        self.fwd("dropout 0.1", p=0.1)
        self.fwd("causal b1 s256 (one workgroup per item)", b=1, s=256)
        for d in (64, 96, 256):
            self.fwd(f"causal d{d}", d=d)
        self.fwd("causal gqa 32/8", h=32, hk=8)
        self.fwd("causal head-strided view", strided=True)
        for splits in (0, 4):
            self.fwd(f"split-kv sq64 sk8192 num_splits={splits}", b=1, s=64, sk=8192, splits=splits)
        self.paged("decode page 16")
        self.paged("decode page 256", page=256)
        self.paged("decode fp8 cache", fp8=True)
        self.paged("decode ragged b8", rag=True)
        self.paged("prefill page 16 (ping-pong)", b=4, sq=2304, s=2304, h=8, hk=8, page=16, splits=1)
        self.paged("prefill page 48 (compiler-scheduled)", b=4, sq=2304, s=2304, h=8, hk=8, page=48, splits=1)
        self.varlen("40 ragged seqused_k", seqused=True)
        self.varlen("few items", n=2, hi=256)
        self.fp8("left window (255, 0)", wl=255)
        for packed in (False, True):
            for d in (64, 128, 256):
                for det in (False, True):
                    self.bwd(d, det, packed)
        for name, vals in (("fwd_dyn", (0, 2)), ("fwd_order", (0,)), ("fwd_persistent", (0, 2)), ("fwd_xcdq", (0,)),
                           ("fwd_waves", (4,)), ("fwd_w4", (0, 2, 3)), ("fp8_w4", (0,))):
            default = self.L.fmha_get_option(name.encode())
            for val in vals:
                assert self.L.fmha_set_option(name.encode(), val) == 0, self.L.fmha_last_error()
                self.knobs = f" [{name}={val}]"
                self.swept()
            assert self.L.fmha_set_option(name.encode(), default) == 0
            self.knobs = ""


if __name__ == "__main__":
    Trace(sys.argv[1]).run()
    print("trace complete")
