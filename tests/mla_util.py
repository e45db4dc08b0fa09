"""Shared helpers of the MLA decode tests (not a conftest: imported explicitly).

MLA decode ("absorbed" multi-head latent attention): every query head attends over one shared
576-wide latent row per token, and the value is the first 512 features of the same row.

* `make_cache`: per-sequence latent rows -> a paged cache behind a random, non-identity block table
  (`decode_util.build_cache` with K given as V too; only `kc` is used), everything the kernel must
  not depend on set to a chosen fill.
* `oracle`: per sequence `orc.attention_ref` / `orc.attention_lse_ref` with v = k[..., :512]; the
  low-precision twin is `upcast=False, reorder_ops=True`.  A softmax scale other than 576^-1/2 is
  carried by q pre-multiplied with `q_mul` (a power of two: exact in every dtype), the float64 twin
  likewise.
* `judge_each` / `assert_case`: the project's kvcache rule (`decode_util.judge`) applied PER
  SEQUENCE: a batch-wide maximum is set by the one-key sequences and hides the long ones.
* `emulate`: a correct split MLA decode on the CPU (`decode_util.emulate_decode` over the 576-wide
  row as K and V, its first 512 output columns), with the defects of DEFECTS plantable.
* `run`: fmha_mla_decode through the C ABI into NaN-filled outputs; asserts the kernel and mapping.
"""
from __future__ import annotations

import ctypes as C

import torch

from oracle import attention_ref as orc
from tests.decode_util import DEV, Oracle, build_cache, emulate_decode, judge, make_q  # noqa: F401

D, DV = 576, 512
PAGE = 16
WIDTH = 1024 // PAGE
# tile counts 17, 10, 3, 2, 1, 1, 1, 1, 0: a full ring, the remainder, one tile, an empty split
# and an empty sequence; 2, 1 and 0 keys are fewer than seqlen_q = 3 under causal
LENS = [517, 300, 65, 33, 32, 31, 2, 1, 0]
# (heads, seqlen_q, causal): one row tile; 24 rows = a tile straddling positions and a partial
# tile; 8 row tiles; 80 rows = 5 tiles over 2 positions
SHAPES = {"h16_sq1": (16, 1, False), "h8_sq3_causal": (8, 3, True), "h128_sq1": (128, 1, False),
          "h40_sq2_causal": (40, 2, True)}
DEFECTS = ("v_shift", "no_rope", "causal_off", "scale192")


def make_cache(lens, dtype, fill="nan", seed=0, page=PAGE, width=WIDTH):
    gen = torch.Generator().manual_seed(500 + seed)
    ks = [torch.randn(n, 1, D, generator=gen) for n in lens]
    return build_cache(ks, ks, page, width, False, dtype, fill, seed=seed)


def oracle(c, q, causal=False, q_mul=1.0) -> Oracle:
    """Per sequence over its keys, v = k[..., :512].  ref: the fp32-upcast oracle in q's dtype;
    ref64: float64; pt: the low-precision twin over the cache in q's dtype; lse fp32 [b, h, sq]."""
    b, sq, h, _ = q.shape
    ref = torch.zeros(b, sq, h, DV, dtype=q.dtype)
    pt = torch.zeros(b, sq, h, DV, dtype=q.dtype)
    ref64 = torch.zeros(b, sq, h, DV, dtype=torch.float64)
    lse = torch.full((b, h, sq), float("inf"), dtype=torch.float32)
    for i in range(b):
        n = c.kx[i].shape[0]
        if n == 0:
            continue
        qi = (q[i:i + 1].float() * q_mul).to(q.dtype)
        k = c.kx[i][None]
        v = k[..., :DV]
        kw = dict(causal=causal)
        ref[i] = orc.attention_ref(qi, k, v, **kw)[0][0]
        ref64[i] = orc.attention_ref(q[i:i + 1].double() * q_mul, k.double(), v.double(), upcast=False, **kw)[0][0]
        pt[i] = orc.attention_ref(qi, k.to(q.dtype), v.to(q.dtype), upcast=False, reorder_ops=True, **kw)[0][0]
        lse[i] = orc.attention_lse_ref(qi, k, **kw)[0]
    return Oracle(ref, ref64, pt, lse)


def judge_each(o, lse, ora: Oracle):
    """`decode_util.judge` (max|o - ref| <= 3 max|pt - ref| + 1e-5, LSE within 1e-3 with the oracle's
    +inf pattern, no NaN) per sequence.  Returns (all ok, [figures per sequence])."""
    figs, good = [], True
    for i in range(o.shape[0]):
        one = Oracle(*(x[i:i + 1] for x in ora))
        ok, f = judge(o[i:i + 1], lse[i:i + 1], one)
        f["ok"] = ok
        f["ratio"] = f["err"] / f["bound"]
        figs.append(f)
        good = good and ok
    return good, figs


def assert_case(name, o, lse, ora, report=None):
    ok, figs = judge_each(o, lse, ora)
    worst = max(figs, key=lambda f: f["ratio"])
    print(f"{name}: worst o err / bound {worst['ratio']:.3f} ({worst['err']:.3e} / {worst['bound']:.3e}); "
          f"lse err {max(f['lse_err'] for f in figs):.3e}")
    if report is not None:
        report(dict(case=name, metric="o", err=worst["err"], bound=worst["bound"]))
        report(dict(case=name, metric="lse", err=max(f["lse_err"] for f in figs), bound=1e-3))
    assert ok, f"{name}: {[(i, f) for i, f in enumerate(figs) if not f['ok']]}"
    return worst["ratio"]


def emulate(c, q, splits, causal=False, defect=None):
    """A correct split MLA decode on the CPU (32-key tiles, `splits` equal ranges, fp32 accumulation,
    P rounded to q's dtype, the combine), or one with a planted defect:
    v_shift: V taken from columns 64-575; no_rope: the 64 rotary columns dropped from the scores;
    causal_off: every row sees one key too many; scale192: the scale of a 192-wide head."""
    assert defect is None or defect in DEFECTS
    window = (-1, 0) if causal else (-1, -1)
    if defect == "causal_off":
        assert causal
        window = (-1, 1)
    if defect == "no_rope":
        q = q.clone()
        q[..., DV:] = 0
    if defect == "scale192":
        q = (q.float() * (D / 192.0) ** 0.5).to(q.dtype)
    o, lse = emulate_decode(c, q, splits, window=window)
    return (o[..., D - DV:] if defect == "v_shift" else o[..., :DV]).contiguous(), lse


def expected_splits(num_splits, batch, row_tiles, max_sk, num_cus):
    """The host's split count."""
    tiles = max(1, (max_sk + 31) // 32)
    s = num_splits if num_splits > 0 else min(128, -(-4 * num_cus // (batch * row_tiles)))
    return max(1, min(s, tiles, 128))


def run(c, q, causal=False, num_splits=0, scale=None, o=None, lse=None, qd=None, want_lse=True):
    """One fmha_mla_decode call on a device copy of the cache.  o / lse / qd: device tensors to use
    (views are fine); else NaN-filled outputs are made.  Returns (o, lse, kernel, splits)."""
    from xf_flash_attention_cutlass_amd import capi
    L = capi.lib()
    b, sq, h, d = q.shape
    qd = q.to(DEV) if qd is None else qd
    kc, tab = c.kc.to(DEV), c.table.to(DEV)
    lens = torch.tensor(c.lens, dtype=torch.int32).to(DEV)
    if o is None:
        o = torch.full((b, sq, h, DV), float("nan"), dtype=q.dtype, device=DEV)
    if lse is None and want_lse:
        lse = torch.full((b, h, sq), float("nan"), dtype=torch.float32, device=DEV)
    st = (C.c_int64 * 6)(qd.stride(0), qd.stride(1), qd.stride(2), o.stride(0), o.stride(1), o.stride(2))
    L.fmha_mla_decode(qd.data_ptr(), kc.data_ptr(), o.data_ptr(), capi.ptr(lse), tab.data_ptr(),
                      tab.stride(0), lens.data_ptr(), sq, c.width * c.page, b, h, D, DV, c.page, st,
                      D ** -0.5 if scale is None else scale, -1, 0 if causal else -1, num_splits,
                      q.dtype == torch.float16, capi.stream_handle())
    capi.check()
    torch.cuda.synchronize()
    kern, splits = L.fmha_last_kernel().decode(), L.fmha_last_num_splits()
    tiles = (sq * h + 15) // 16
    want = "fmha_mla_decode_kernel<%s>" % ("tiles" if tiles > 1 else "splits")
    assert kern.startswith(want), f"ran {kern!r}, wanted {want!r}"
    items = b * splits * tiles
    assert "grid=%dx1x1 block=256" % ((items + 3) // 4) in kern, kern
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert splits == expected_splits(num_splits, b, tiles, c.width * c.page, cus), (splits, num_splits)
    return o, lse, kern, splits
