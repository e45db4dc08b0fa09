"""What the PyTorch layer decides and computes: a fixed, seeded list of small calls through the
`paged_attn` ops and the Python wrappers, one line per call with the case, fmha_last_kernel(),
fmha_last_num_splits() and the sha256 of every tensor the call returns (the padded q / k / v / out,
rng_state and s_dmask included; a cache an op appends to as well).  The sibling of
tools/launch_trace.py, which traces the C ABI.  Two trees that decide and compute the same print
the same text:

  python tools/op_trace.py --root treeA > a.txt; python tools/op_trace.py --root treeB > b.txt

Backward results are hashed in deterministic mode only (the atomic sums differ in the last bits
from run to run; that mode is run, not hashed).  The kernel string of a call that launches no
forward (a backward, seqlen_k == 0, quantize_fp8) is the one the last forward left.

--time: host microseconds per call of `fwd`, `varlen_fwd`, `fwd_kvcache` (decode) and
`fwd_kvcache_fp8` at the small decode shape: N calls enqueued back to back, one synchronise at the end.
"""
from __future__ import annotations

import argparse
import hashlib
import os
import sys
import time

import torch

DEV = "cuda"
BF, F16, F32, F8 = torch.bfloat16, torch.float16, torch.float32, torch.float8_e4m3fn
B, H, HK = 2, 4, 2
_cache = {}


def rand(key, *shape, dtype=BF, scale=1.0):
    """the same tensor for the same key in every run (CPU generator)"""
    k = (key, shape, dtype, scale)
    if k not in _cache:
        g = torch.Generator().manual_seed(int(hashlib.sha256(repr(k).encode()).hexdigest()[:8], 16))
        _cache[k] = (torch.randn(*shape, generator=g) * scale).to(dtype).to(DEV)
    return _cache[k].clone()


def i32(*vals):
    return torch.tensor(vals, dtype=torch.int32, device=DEV)


def cu(*lens):
    return i32(0, *torch.tensor(lens).cumsum(0).tolist())


def sha(t):
    if t is None:
        return "-"
    if not isinstance(t, torch.Tensor):
        return repr(t)
    raw = t.detach().contiguous().view(torch.uint8).cpu().numpy().tobytes()
    return f"{tuple(t.shape)}:{hashlib.sha256(raw).hexdigest()[:16]}"


def head_view(t):
    """t's values as every second head of a tensor with twice the heads (aligned, not contiguous)"""
    big = torch.empty(*t.shape[:-2], 2 * t.shape[-2], t.shape[-1], dtype=t.dtype, device=t.device)
    big[..., ::2, :] = t
    return big[..., ::2, :]


def misaligned(t):
    """t's values at a storage offset of 8 bytes"""
    flat = torch.empty(t.numel() + 8 // t.element_size(), dtype=t.dtype, device=t.device)
    out = flat[8 // t.element_size():].view(t.shape)
    out.copy_(t)
    return out


class Trace:
    def __init__(self, xfa, capi):
        self.xfa, self.pa, self.L = xfa, xfa.paged_attn, capi.lib()

    def line(self, case, *outs):
        torch.cuda.synchronize()
        L = self.L
        print(f"{case}: kernel=[{L.fmha_last_kernel().decode()}] splits={L.fmha_last_num_splits()} "
              f"sha={' '.join(sha(t) for t in outs)}", flush=True)

    # ------------------------------------------------------------------ the ops, positionally
    def qkv(self, d, sq=33, sk=130, tag=""):
        return (rand("q" + tag, B, sq, H, d), rand("k" + tag, B, sk, HK, d), rand("v" + tag, B, sk, HK, d))

    def fwd(self, case, q, k, v, out=None, alibi=None, p=0.0, causal=True, wl=-1, wr=-1, softcap=0.0,
            ret=False, sink=None):
        if p > 0:
            torch.manual_seed(1234)
        a = (q, k, v, out, alibi, p, q.shape[-1] ** -0.5, causal, wl, wr, softcap, ret, None)
        r = self.pa.fwd(*a) if sink is None else self.pa.fwd_sink(*a, sink)
        self.line(case, *r, out)
        return r

    def dense_fwd(self):
        sink = rand("sink", H, dtype=F32)
        al_h = rand("alibi", H, dtype=F32, scale=0.05).abs()
        al_bh = rand("alibi", B, H, dtype=F32, scale=0.05).abs()
        for d in (64, 40, 36):        # 36: padded to 40, the copying path
            q, k, v = self.qkv(d)
            self.fwd(f"fwd d{d} causal", q, k, v)
            self.fwd(f"fwd d{d} non-causal", q, k, v, causal=False)
            self.fwd(f"fwd d{d} window (8, 0)", q, k, v, causal=False, wl=8, wr=0)
            self.fwd(f"fwd d{d} window past seqlen_k", q, k, v, causal=False, wl=200, wr=130)
            self.fwd(f"fwd d{d} softcap", q, k, v, softcap=30.0)
            self.fwd(f"fwd d{d} alibi [h]", q, k, v, alibi=al_h)
            self.fwd(f"fwd d{d} alibi [b, h]", q, k, v, alibi=al_bh, causal=False)
            self.fwd(f"fwd d{d} dropout return_softmax", q, k, v, p=0.1, ret=True)
            self.fwd(f"fwd d{d} dropout", q, k, v, p=0.2, causal=False)
            self.fwd(f"fwd d{d} head-sliced views", head_view(q), head_view(k), head_view(v))
            kv = torch.stack([k, v], dim=2)
            self.fwd(f"fwd d{d} kvpacked", q, kv[:, :, 0], kv[:, :, 1])
            self.fwd(f"fwd d{d} misaligned storage offset", misaligned(q), k, misaligned(v))
            self.fwd(f"fwd d{d} out aligned", q, k, v, out=torch.zeros_like(q))
            self.fwd(f"fwd d{d} out non-contiguous", q, k, v, out=head_view(torch.zeros_like(q)))
            self.fwd(f"fwd d{d} out non-contiguous, views", head_view(q), k, v, out=head_view(torch.zeros_like(q)))
            self.fwd(f"fwd d{d} out misaligned", q, k, v, out=misaligned(torch.zeros_like(q)))
            self.fwd(f"fwd d{d} seqlen_k 0 causal", q, k[:, :0], v[:, :0], out=torch.ones_like(q))
            self.fwd(f"fwd d{d} seqlen_k 0 window", q, k[:, :0], v[:, :0], causal=False, wl=0, wr=0)
            q1 = q[:, :1].contiguous()
            self.fwd(f"fwd d{d} seqlen_q 1 causal", q1, k, v)
            self.fwd(f"fwd d{d} seqlen_q 1 causal alibi", q1, k, v, alibi=al_h)
            self.fwd(f"fwd_sink d{d} causal", q, k, v, sink=sink)
            self.fwd(f"fwd_sink d{d} window, views, out", head_view(q), head_view(k), v, causal=False, wl=16, wr=4,
                     sink=sink, out=torch.zeros_like(q))
        q, k, v = (x.to(F16) for x in self.qkv(64))
        self.fwd("fwd d64 fp16", q, k, v)
        q, k, v = self.qkv(128, tag="128")
        self.fwd("fwd d128 causal", q, k, v)

    def varlen_fwd(self, case, q, k, v, cu_q, cu_k, max_q, max_k, out=None, seqused=None, table=None, alibi=None,
                   p=0.0, zero=False, causal=True, wl=-1, wr=-1, softcap=0.0, ret=False, sink=None):
        if p > 0:
            torch.manual_seed(4321)
        a = (q, k, v, out, cu_q, cu_k, seqused, table, alibi, max_q, max_k, p, q.shape[-1] ** -0.5, zero, causal,
             wl, wr, softcap, ret, None)
        r = self.pa.varlen_fwd(*a) if sink is None else self.pa.varlen_fwd_sink(*a, sink)
        self.line(case, *r, out)
        return r

    def varlen(self):
        sink = rand("sink", H, dtype=F32)
        lq, lk = (17, 33), (50, 80)
        cq, ck = cu(*lq), cu(*lk)
        for d in (64, 40, 36):        # 36: padded to 40, the copying path
            q, k, v = rand("vq", 50, H, d), rand("vk", 130, HK, d), rand("vv", 130, HK, d)
            f = lambda case, **kw: self.varlen_fwd(f"varlen_fwd d{d} {case}", q, k, v, cq, ck, 33, 80, **kw)   # noqa: E731
            f("plain")
            f("non-causal", causal=False)
            f("seqused_k", seqused=i32(40, 70))
            f("zero_tensors", zero=True)
            f("window", causal=False, wl=8, wr=3)
            f("alibi [h]", alibi=rand("alibi", H, dtype=F32, scale=0.05).abs())
            f("alibi [b, h]", alibi=rand("alibi", B, H, dtype=F32, scale=0.05).abs())
            f("dropout return_softmax", p=0.1, ret=True)
            f("out given", out=torch.zeros_like(q))
            f("out non-contiguous", out=head_view(torch.zeros_like(q)))
            f("out misaligned", out=misaligned(torch.zeros_like(q)))
            f("sink", sink=sink)
            self.varlen_fwd(f"varlen_fwd d{d} head-sliced views", head_view(q), head_view(k), v, cq, ck, 33, 80)
            self.varlen_fwd(f"varlen_fwd d{d} max_seqlen_k 0", q, k[:0], v[:0], cq, cu(0, 0), 33, 0,
                            out=torch.ones_like(q))
            self.varlen_fwd(f"varlen_fwd d{d} max_seqlen_q 1", q[:2].contiguous(), k, v, cu(1, 1), ck, 1, 80)
            pages = torch.randperm(10, generator=torch.Generator().manual_seed(3)).to(torch.int32).view(2, 5).to(DEV)
            kp, vp = rand("vkp", 10, 16, HK, d), rand("vvp", 10, 16, HK, d)
            self.varlen_fwd(f"varlen_fwd d{d} paged block_table", q, kp, vp, cq, ck, 33, 80, table=pages)
            self.varlen_fwd(f"varlen_fwd d{d} paged block_table seqused_k sink", q, kp, vp, cq, ck, 33, 80,
                            table=pages, seqused=i32(40, 70), sink=sink)

    def kvcache(self, case, q, kc, vc, k=None, v=None, seqlens=None, cos=None, sin=None, idx=None, table=None,
                alibi=None, out=None, causal=False, wl=-1, wr=-1, softcap=0.0, interleaved=False, splits=0,
                leftpad=None, sink=None):
        kc, vc = kc.clone(), vc.clone()
        a = (q, kc, vc, k, v, seqlens, cos, sin, idx, table, alibi, out, q.shape[-1] ** -0.5, causal, wl, wr,
             softcap, interleaved, splits, leftpad)
        r = self.pa.fwd_kvcache(*a) if sink is None else self.pa.fwd_kvcache_sink(*a, sink)
        self.line(case, *r, out, *((kc, vc) if k is not None else ()))

    def decode(self):
        sink = rand("sink", H, dtype=F32)
        lens = i32(50, 100)
        cos, sin = rand("cos", 128, 16), rand("sin", 128, 16)
        pages = torch.randperm(16, generator=torch.Generator().manual_seed(5)).to(torch.int32).view(2, 8).to(DEV)
        for sq in (1, 3):
            q = rand("dq", B, sq, H, 64)
            kc, vc = rand("dkc", B, 128, HK, 64), rand("dvc", B, 128, HK, 64)
            kn, vn = rand("dkn", B, sq, HK, 64), rand("dvn", B, sq, HK, 64)
            f = lambda case, **kw: self.kvcache(f"fwd_kvcache sq{sq} {case}", q, kc, vc, seqlens=lens, **kw)   # noqa: E731
            f("dense cache")
            f("dense cache causal", causal=True)
            f("dense cache window", wl=16, wr=0)
            f("dense cache num_splits 2", splits=2)
            f("dense cache alibi", alibi=rand("alibi", H, dtype=F32, scale=0.05).abs(), causal=True)
            f("dense cache softcap", softcap=20.0)
            f("dense cache out given", out=torch.zeros_like(q))
            f("dense cache out non-contiguous", out=head_view(torch.zeros_like(q)))
            f("leftpad", leftpad=i32(3, 5))
            f("sink", sink=sink)
            f("append", k=kn, v=vn)
            f("append causal", k=kn, v=vn, causal=True)
            f("append rotary", k=kn, v=vn, cos=cos, sin=sin, causal=True)
            f("append rotary interleaved", k=kn, v=vn, cos=cos, sin=sin, interleaved=True)
            f("append rotary sink", k=kn, v=vn, cos=cos, sin=sin, sink=sink)
            self.kvcache(f"fwd_kvcache sq{sq} no seqlens_k", q, kc, vc)
            self.kvcache(f"fwd_kvcache sq{sq} cache_batch_idx", q, rand("dkc4", 4, 128, HK, 64),
                         rand("dvc4", 4, 128, HK, 64), seqlens=lens, idx=i32(2, 0))
            kp, vp = rand("dkp", 16, 16, HK, 64), rand("dvp", 16, 16, HK, 64)
            self.kvcache(f"fwd_kvcache sq{sq} paged", q, kp, vp, seqlens=lens, table=pages)
            self.kvcache(f"fwd_kvcache sq{sq} paged causal sink", q, kp, vp, seqlens=lens, table=pages, causal=True,
                         sink=sink)
            self.kvcache(f"fwd_kvcache sq{sq} paged append rotary", q, kp, vp, k=kn, v=vn, seqlens=lens, table=pages,
                         cos=cos, sin=sin, causal=True)
            for d in (40, 36):
                qd = rand("dq", B, sq, H, d)
                self.kvcache(f"fwd_kvcache sq{sq} d{d}", qd, rand("dkc", B, 128, HK, d), rand("dvc", B, 128, HK, d),
                             seqlens=lens, out=torch.zeros_like(qd))
            # ---- the fp8 cache
            q8 = rand("dq", B, sq, H, 128)
            k8, v8 = (rand(n, 16, 16, HK, 128).to(F8).view(torch.uint8) for n in ("dk8", "dv8"))
            a = (q8, k8, v8, lens, pages, 0.5, 0.25, 128 ** -0.5, False, -1, -1, 0)
            self.line(f"fwd_kvcache_fp8 sq{sq}", *self.pa.fwd_kvcache_fp8(*a))
            self.line(f"fwd_kvcache_fp8_sink sq{sq}", *self.pa.fwd_kvcache_fp8_sink(*a, sink))
            a = (q8, k8, v8, lens, pages, 0.5, 0.25, 128 ** -0.5, True, 16, -1, 2)
            self.line(f"fwd_kvcache_fp8 sq{sq} causal window num_splits 2", *self.pa.fwd_kvcache_fp8(*a))
            kn8, vn8 = rand("dkn8", B, sq, HK, 128), rand("dvn8", B, sq, HK, 128)
            for name, rot, inter, per_token in (("", (None, None), False, False), (" rotary", (cos, sin), False, True),
                                                (" rotary interleaved", (cos, sin), True, False)):
                kc8, vc8 = k8.clone(), v8.clone()
                r = self.pa.kvcache_append_fp8(q8, kc8, vc8, kn8, vn8, lens, pages, *rot, 0.5, 0.25, inter, per_token)
                self.line(f"kvcache_append_fp8 sq{sq}{name}", *r, kc8, vc8)

    def fp8(self):
        q, k, v = (rand(n, B, 64, hh, 128).to(F8) for n, hh in (("8q", H), ("8k", HK), ("8v", HK)))
        one = lambda x: torch.full((1,), x, dtype=F32, device=DEV)             # noqa: E731
        per = lambda n: rand(n, B, HK, dtype=F32, scale=0.2).abs() + 0.5         # noqa: E731
        tail = (128 ** -0.5, True, -1, -1, False)
        self.line("fwd_fp8 by value", *self.pa.fwd_fp8(q, k, v, None, 0.5, 0.75, 1.25, *tail))
        out = torch.zeros(B, 64, H, 128, dtype=F16, device=DEV)
        self.line("fwd_fp8 by value fp16 out given window", *self.pa.fwd_fp8(q, k, v, out, 0.5, 0.75, 1.25,
                                                                             128 ** -0.5, False, 16, 8, True), out)
        self.line("fwd_fp8 seqlen_q 1", *self.pa.fwd_fp8(q[:, :1].contiguous(), k, v, None, 1.0, 1.0, 1.0, *tail))
        self.line("fwd_fp8_ex [1]", *self.pa.fwd_fp8_ex(q, k, v, None, one(0.5), one(0.75), one(1.25), *tail))
        self.line("fwd_fp8_ex [b, hk]", *self.pa.fwd_fp8_ex(q, k, v, None, per("a"), per("b"), per("c"), *tail))
        self.line("fwd_fp8_ex mixed", *self.pa.fwd_fp8_ex(q, k, v, None, one(0.5), per("b"), one(1.25)[0], *tail))
        cq, ck = cu(17, 33), cu(50, 80)
        q, k, v = (rand(n, t, hh, 128).to(F8) for n, t, hh in (("8vq", 50, H), ("8vk", 130, HK), ("8vv", 130, HK)))
        head = (q, k, v, None, cq, ck, None, 33, 80)
        self.line("varlen_fwd_fp8 by value", *self.pa.varlen_fwd_fp8(*head, 0.5, 0.75, 1.25, *tail))
        head_u = (q, k, v, None, cq, ck, i32(40, 70), 33, 80)
        self.line("varlen_fwd_fp8 seqused_k", *self.pa.varlen_fwd_fp8(*head_u, 0.5, 0.75, 1.25, *tail))
        self.line("varlen_fwd_fp8_ex [1]", *self.pa.varlen_fwd_fp8_ex(*head, one(0.5), one(0.75), one(1.25), *tail))
        self.line("varlen_fwd_fp8_ex [b, hk]", *self.pa.varlen_fwd_fp8_ex(*head, per("a"), per("b"), per("c"), *tail))
        self.line("varlen_fwd_fp8_ex mixed", *self.pa.varlen_fwd_fp8_ex(*head_u, per("a"), one(0.75), one(1.25), *tail))
        # ---- quantize_fp8
        x = rand("x", B, 33, H, 64)
        xp = rand("xp", 50, H, 64)
        for g in (0, 1):
            self.line(f"quantize_fp8 dense granularity {g}", *self.pa.quantize_fp8(x, g, 2, None, 0))
            self.line(f"quantize_fp8 strided granularity {g}", *self.pa.quantize_fp8(head_view(x), g, 1, None, 0))
            self.line(f"quantize_fp8 misaligned granularity {g}", *self.pa.quantize_fp8(misaligned(x), g, 1))
            self.line(f"quantize_fp8 packed granularity {g}", *self.pa.quantize_fp8(xp, g, 2, cq, 0))
            self.line(f"quantize_fp8 packed max_seqlen granularity {g}", *self.pa.quantize_fp8(xp.to(F16), g, 1, cq, 33))

    def backward(self):
        sink = rand("sink", H, dtype=F32)
        for d in (64, 40, 36):        # 36: padded to 40, the copying path
            q, k, v = self.qkv(d)
            for name, kw in (("causal", {}), ("dropout", dict(p=0.1)), ("sink", dict(sink=sink))):
                o, qp, kp, vp, op, lse, _, rng = self.fwd(f"fwd d{d} for the backward {name}", q, k, v, **kw)
                do = rand("do", *o.shape)
                p = kw.get("p", 0.0)
                for det in (False, True):
                    r = self.pa.bwd(do, qp, kp, vp, op, lse, None, None, None, None, p, d ** -0.5, True, -1, -1, 0.0,
                                    det, None, rng)
                    self.line(f"bwd d{d} {name} {'deterministic' if det else 'atomic'}", *(r if det else ()))
                if "sink" in kw:
                    self.line(f"sink_bwd d{d}", self.pa.sink_bwd(lse, r[3], sink, False))
            dq_ = head_view(torch.zeros_like(qp))
            r = self.pa.bwd(do, qp, kp, vp, op, lse, dq_, torch.zeros_like(kp), None, None, 0.0, d ** -0.5, True, -1, -1,
                            0.0, True, None, None)
            self.line(f"bwd d{d} dq_ non-contiguous, dk_ given", *r, dq_)
            # ---- varlen
            cq, ck = cu(17, 33), cu(50, 80)
            q, k, v = rand("vq", 50, H, d), rand("vk", 130, HK, d), rand("vv", 130, HK, d)
            for name, kw in (("causal", {}), ("dropout", dict(p=0.1)), ("sink", dict(sink=sink))):
                o, qp, kp, vp, op, lse, _, rng = self.varlen_fwd(f"varlen_fwd d{d} for the backward {name}", q, k, v,
                                                                 cq, ck, 33, 80, **kw)
                do = rand("vdo", *o.shape)
                p = kw.get("p", 0.0)
                for det in (False, True):
                    r = self.pa.varlen_bwd(do, qp, kp, vp, op, lse, None, None, None, cq, ck, None, 33, 80, p,
                                           d ** -0.5, False, True, -1, -1, 0.0, det, None, rng)
                    self.line(f"varlen_bwd d{d} {name} {'deterministic' if det else 'atomic'}", *(r if det else ()))
                if "sink" in kw:
                    self.line(f"sink_bwd varlen d{d}", self.pa.sink_bwd(lse, r[3], sink, True))
            dq_ = head_view(torch.zeros_like(qp))
            r = self.pa.varlen_bwd(do, qp, kp, vp, op, lse, dq_, None, torch.zeros_like(vp), cq, ck, None, 33, 80, 0.0,
                                   d ** -0.5, False, True, 8, -1, 0.0, True, None, None)
            self.line(f"varlen_bwd d{d} window dq_ non-contiguous, dv_ given", *r, dq_)

    # ------------------------------------------------------------------ the Python wrappers
    def grads(self, case, fn, *leaves):
        """forward and backward through autograd (deterministic), every result and gradient hashed"""
        leaves = [x.clone().requires_grad_(True) for x in leaves]
        out = fn(*leaves)
        outs = out if isinstance(out, tuple) else (out,)
        g = torch.autograd.grad(outs[0], leaves, rand("g" + case, *outs[0].shape, dtype=outs[0].dtype))
        self.line(case, *outs, *g)

    def wrappers(self):
        x = self.xfa
        sink = rand("sink", H, dtype=BF)
        cq, ck = cu(17, 33), cu(50, 80)
        for d in (64, 40, 36):        # 36: padded to 40, the copying path
            q, k, v = self.qkv(d)
            kv = torch.stack([k, v], dim=2)
            vq, vk, vv = rand("vq", 50, H, d), rand("vk", 130, HK, d), rand("vv", 130, HK, d)
            vkv = torch.stack([vk, vv], dim=1)
            det = dict(causal=True, deterministic=True)
            self.grads(f"flash_attn_func d{d}", lambda q, k, v: x.flash_attn_func(q, k, v, **det), q, k, v)
            self.grads(f"flash_attn_func d{d} sink", lambda q, k, v, s: x.flash_attn_func(q, k, v, sink=s, **det),
                       q, k, v, sink)
            self.grads(f"flash_attn_func d{d} sink return_attn_probs",
                       lambda q, k, v: x.flash_attn_func(q, k, v, sink=sink, return_attn_probs=True, **det)[:2], q, k, v)
            torch.manual_seed(99)
            self.grads(f"flash_attn_func d{d} dropout alibi return_attn_probs",
                       lambda q, k, v: x.flash_attn_func(q, k, v, 0.1, alibi_slopes=rand("alibi", H, dtype=F32, scale=0.05).abs(),
                                                         return_attn_probs=True, **det), q, k, v)
            self.grads(f"flash_attn_kvpacked_func d{d}", lambda q, kv: x.flash_attn_kvpacked_func(q, kv, **det), q, kv)
            self.grads(f"flash_attn_kvpacked_func d{d} sink",
                       lambda q, kv, s: x.flash_attn_kvpacked_func(q, kv, sink=s, window_size=(16, 0), deterministic=True),
                       q, kv, sink)
            self.grads(f"flash_attn_varlen_func d{d}",
                       lambda q, k, v: x.flash_attn_varlen_func(q, k, v, cq, ck, 33, 80, **det), vq, vk, vv)
            self.grads(f"flash_attn_varlen_func d{d} sink",
                       lambda q, k, v, s: x.flash_attn_varlen_func(q, k, v, cq, ck, 33, 80, sink=s, **det), vq, vk, vv, sink)
            torch.manual_seed(98)
            self.grads(f"flash_attn_varlen_func d{d} dropout return_attn_probs",
                       lambda q, k, v: x.flash_attn_varlen_func(q, k, v, cq, ck, 33, 80, 0.1, return_attn_probs=True, **det),
                       vq, vk, vv)
            self.grads(f"flash_attn_varlen_kvpacked_func d{d}",
                       lambda q, kv: x.flash_attn_varlen_kvpacked_func(q, kv, cq, ck, 33, 80, **det), vq, vkv)
            self.grads(f"flash_attn_varlen_kvpacked_func d{d} sink",
                       lambda q, kv, s: x.flash_attn_varlen_kvpacked_func(q, kv, cq, ck, 33, 80, sink=s, **det), vq, vkv, sink)
        # ---- caches (forward only)
        q = rand("dq", B, 1, H, 64)
        kc, vc = rand("dkc", B, 128, HK, 64), rand("dvc", B, 128, HK, 64)
        kn, vn = rand("dkn", B, 1, HK, 64), rand("dvn", B, 1, HK, 64)
        pages = torch.randperm(16, generator=torch.Generator().manual_seed(5)).to(torch.int32).view(2, 8).to(DEV)
        for s in (None, sink):
            tag = "" if s is None else " sink"
            self.line(f"flash_attn_with_kvcache int cache_seqlens{tag}",
                      *x.flash_attn_with_kvcache(q, kc, vc, cache_seqlens=77, return_softmax_lse=True, sink=s))
            c1, c2 = kc.clone(), vc.clone()
            self.line(f"flash_attn_with_kvcache append rotary{tag}",
                      x.flash_attn_with_kvcache(q, c1, c2, kn, vn, rand("cos", 128, 16), rand("sin", 128, 16),
                                                cache_seqlens=i32(50, 100), causal=True, sink=s), c1, c2)
            self.line(f"flash_attn_with_kvcache leftpad cache_batch_idx{tag}",
                      x.flash_attn_with_kvcache(q, kc, vc, cache_seqlens=i32(50, 100), cache_leftpad=i32(3, 5),
                                                cache_batch_idx=i32(1, 0), sink=s))
            q8 = rand("dq", B, 1, H, 128)
            k8, v8 = (rand(n, 16, 16, HK, 128).to(F8) for n in ("dk8", "dv8"))
            self.line(f"flash_attn_with_kvcache fp8 cache int cache_seqlens{tag}",
                      *x.flash_attn_with_kvcache(q8, k8, v8, cache_seqlens=77, block_table=pages, k_scale=0.5,
                                                 v_scale=0.25, return_softmax_lse=True, sink=s))
            c1, c2 = k8.clone(), v8.clone()
            self.line(f"flash_attn_with_kvcache fp8 cache append rotary{tag}",
                      x.flash_attn_with_kvcache(q8, c1, c2, rand("dkn8", B, 1, HK, 128), rand("dvn8", B, 1, HK, 128),
                                                rand("cos", 128, 16), rand("sin", 128, 16), cache_seqlens=i32(50, 100),
                                                block_table=pages, k_scale=0.5, v_scale=0.25, causal=True, sink=s), c1, c2)
        # ---- fp8 q / k / v (forward only)
        qb, kb, vb = (rand(n, B, 64, hh, 128) for n, hh in (("8q", H), ("8k", HK), ("8v", HK)))
        q8, k8, v8 = qb.to(F8), kb.to(F8), vb.to(F8)
        dev = torch.full((1,), 0.75, dtype=F32, device=DEV)
        self.line("flash_attn_fp8_func floats", *x.flash_attn_fp8_func(q8, k8, v8, 0.5, None, 1.25, causal=True, return_lse=True))
        self.line("flash_attn_fp8_func device descale", x.flash_attn_fp8_func(q8, k8, v8, 0.5, dev, None, out_dtype=F16))
        self.line("flash_attn_fp8_func quantize head", x.flash_attn_fp8_func(qb, kb, vb, quantize="head", causal=True))
        self.line("flash_attn_func fp8", *x.flash_attn_func(q8, k8, v8, causal=True, return_attn_probs=True, k_descale=dev))
        qb, kb, vb = (rand(n, t, hh, 128) for n, t, hh in (("8vq", 50, H), ("8vk", 130, HK), ("8vv", 130, HK)))
        q8, k8, v8 = qb.to(F8), kb.to(F8), vb.to(F8)
        self.line("flash_attn_varlen_fp8_func floats", *x.flash_attn_varlen_fp8_func(q8, k8, v8, cq, ck, 33, 80, 0.5, None, 1.25,
                                                                                     causal=True, return_lse=True))
        self.line("flash_attn_varlen_fp8_func device descale seqused_k",
                  x.flash_attn_varlen_fp8_func(q8, k8, v8, cq, ck, 33, 80, None, dev, 2.0, seqused_k=i32(40, 70)))
        self.line("flash_attn_varlen_fp8_func quantize tensor",
                  x.flash_attn_varlen_fp8_func(qb, kb, vb, cq, ck, 33, 80, quantize="tensor", causal=True))
        self.line("flash_attn_varlen_func fp8", *x.flash_attn_varlen_func(q8, k8, v8, cq, ck, 33, 80, causal=True,
                                                                         return_attn_probs=True, v_descale=dev))
        self.line("quantize_fp8 head packed", *x.quantize_fp8(qb, "head", 2, cq, max_seqlen=33))
        self.line("quantize_fp8 tensor", *x.quantize_fp8(qb[None], "tensor"))

    def run(self):
        self.dense_fwd()
        self.varlen()
        self.decode()
        self.fp8()
        self.backward()
        self.wrappers()

    # ------------------------------------------------------------------ host time per call
    def timed(self, n):
        lens = i32(100, 128)
        q, k, v = self.qkv(64, sq=1, sk=128)
        vq, vk, vv = rand("vq", B, H, 64), rand("vk", 2 * 128, HK, 64), rand("vv", 2 * 128, HK, 64)
        cq, ck = cu(1, 1), cu(128, 128)
        q8 = rand("dq", B, 1, H, 128)
        pages = torch.arange(16, dtype=torch.int32, device=DEV).view(2, 8)
        k8, v8 = (rand(nm, 16, 16, HK, 128).to(F8).view(torch.uint8) for nm in ("dk8", "dv8"))
        calls = {
            "fwd": lambda: self.pa.fwd(q, k, v, None, None, 0.0, 0.125, False, -1, -1, 0.0, False, None),
            "varlen_fwd": lambda: self.pa.varlen_fwd(vq, vk, vv, None, cq, ck, None, None, None, 1, 128, 0.0, 0.125,
                                                     False, False, -1, -1, 0.0, False, None),
            "fwd_kvcache": lambda: self.pa.fwd_kvcache(q, k, v, None, None, lens, None, None, None, None, None, None,
                                                       0.125, False, -1, -1, 0.0, False, 0),
            "fwd_kvcache_fp8": lambda: self.pa.fwd_kvcache_fp8(q8, k8, v8, lens, pages, 0.5, 0.25, 0.088, False, -1,
                                                               -1, 0),
        }
        for name, call in calls.items():
            for _ in range(200):
                call()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                call()
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            print(f"{name}: {1e6 * (t1 - t0) / n:.2f} us/call enqueued, {1e6 * (t2 - t0) / n:.2f} us/call with the "
                  f"final synchronise ({n} calls)", flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    help="the tree whose built package is traced (default: this one)")
    ap.add_argument("--time", action="store_true", help="host microseconds per call instead of the trace")
    ap.add_argument("-n", type=int, default=3000, help="--time: calls per op")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    import xf_flash_attention_cutlass_amd as xfa
    from xf_flash_attention_cutlass_amd import capi
    assert os.path.abspath(xfa.__file__).startswith(os.path.abspath(a.root)), xfa.__file__
    t = Trace(xfa, capi)
    if a.time:
        t.timed(a.n)
    else:
        t.run()
        print("trace complete")


if __name__ == "__main__":
    main()
