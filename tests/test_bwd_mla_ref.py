"""CPU: the MLA prefill backward (ABI 2.13) - what it computes, the rule it is
held to, its surface and every refusal that needs no launch.

* In float64 the only route the library had before - V and dO zero-padded to 192 columns, the
  gradient at D = 192, dV sliced to 128 - equals the two-width oracle to 1e-10, and its padded dV
  columns are 0: the oracle the GPU tests use is the padded route's result.
* For every case of the GPU table (tests/bwd_mla_util.py CASES), `emulate_bwd_mla` - a correct
  kernel's arithmetic - passes `bwd_util.check_grads` against `bwd_util.ref_grads` per sequence:
  the rule is satisfiable on exactly the inputs the GPU sees.  The ratios are printed (pytest -s).
* Each planted two-width defect is rejected on a case from the table.
* The 2.13 surface, the code objects' scratch, and the refusals of the C entries (fake pointers: no
  launch) and of the Python wrappers.
"""
import ctypes as C
import inspect
import re

import pytest
import torch

from oracle import attention_ref as orc
from tests import bwd_mla_util as mu
from tests import bwd_util as bu
from xf_flash_attention_cutlass_amd import capi

DTS = list(mu.DTYPES)


def test_padded_route_is_the_oracle_in_float64():
    gen = torch.Generator().manual_seed(7)
    q = torch.randn(2, 37, 6, mu.DQK, generator=gen, dtype=torch.float64)
    k = torch.randn(2, 53, 2, mu.DQK, generator=gen, dtype=torch.float64)
    v = torch.randn(2, 53, 2, mu.DV, generator=gen, dtype=torch.float64)
    g = torch.randn(2, 37, 6, mu.DV, generator=gen, dtype=torch.float64)
    pad = (0, mu.DQK - mu.DV)
    for window in ((-1, -1), (-1, 0), (11, 0), (-1, 5)):
        a = [x.clone().requires_grad_(True) for x in (q, k, v)]
        want = torch.autograd.grad(orc.attention_ref(*a, window_size=window, upcast=False)[0], a, g)
        b = [x.clone().requires_grad_(True) for x in (q, k, torch.nn.functional.pad(v, pad))]
        got = torch.autograd.grad(orc.attention_ref(*b, window_size=window, upcast=False)[0], b,
                                  torch.nn.functional.pad(g, pad))
        assert (got[0] - want[0]).abs().max().item() <= 1e-10
        assert (got[1] - want[1]).abs().max().item() <= 1e-10
        assert (got[2][..., :mu.DV] - want[2]).abs().max().item() <= 1e-10
        assert got[2][..., mu.DV:].abs().max().item() == 0.0


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("case", mu.CASES, ids=[c.name for c in mu.CASES])
def test_correct_emulation_passes_the_rule_on_every_gpu_case(case, dt):
    dtype = mu.DTYPES[dt]
    mu.check_case(f"emulate {case.name} {dt}", mu.emulate_case(case, dtype), case, dtype)


# the case each defect is planted on: the full 113 x 300 one, and the causal one (sk != sq) for the
# alignment of the mask
DEFECT_CASE = {d: "d113x300_causal" if d == "topleft" else "d113x300_full" for d in mu.DEFECTS}


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("defect", mu.DEFECTS)
def test_planted_defects_are_rejected(defect, dt):
    case, dtype = mu.CASE[DEFECT_CASE[defect]], mu.DTYPES[dt]
    with pytest.raises(AssertionError) as e:
        mu.check_case(f"defect {defect} {dt}", mu.emulate_case(case, dtype, defect), case, dtype)
    print(f"defect {defect} {dt}: {str(e.value)[:300]}")


# ------------------------------------------------------------------ surface ---------------
SYMS = ("fmha_bwd_mla", "fmha_varlen_bwd_mla")


def test_surface_2_13():
    import xf_flash_attention_cutlass_amd as xfa
    from tests.test_abi import header_symbols
    for sym in SYMS:
        assert sym in header_symbols() and sym in capi.EXPORTED and hasattr(capi.lib(), sym)
        assert getattr(capi.lib(), sym).argtypes == capi._SIGS[sym]
    ver = capi.lib().fmha_version().decode().split()[1]
    assert tuple(int(x) for x in ver.split(".")) >= (2, 13)
    for op in ("bwd_mla", "varlen_bwd_mla"):
        assert callable(getattr(xfa.paged_attn, op))
        assert getattr(xfa.paged_attn, op) is getattr(xfa.paged_attn, "_" + op)
        assert op not in dir(xfa.paged_attn)
    for name in ("flash_attn_mla_func", "flash_attn_mla_varlen_func"):
        assert name in xfa.__all__ and callable(getattr(xfa, name))
    sig = inspect.signature(xfa.flash_attn_mla_func).parameters
    assert list(sig) == ["q", "k", "v", "causal", "window_size", "softmax_scale", "deterministic",
                         "return_attn_probs"]
    assert list(inspect.signature(xfa.flash_attn_mla_varlen_func).parameters)[:7] == [
        "q", "k", "v", "cu_seqlens_q", "cu_seqlens_k", "max_seqlen_q", "max_seqlen_k"]


def _msgpack_uint(blob, i):
    t = blob[i]
    if t < 0x80:
        return t
    return int.from_bytes(blob[i + 1:i + 1 + {0xcc: 1, 0xcd: 2, 0xce: 4}[t]], "big")


def test_code_objects_have_no_scratch():
    """All 18 instances (bf16 / fp16 x {pre, dkdv x MASK x PACKED, dq x MASK x PACKED}) are in the
    library's gfx950 code object with private_segment_fixed_size 0 and no spilled register; the
    dK/dV and dQ kernels run one wave a SIMD (at most 512 registers)."""
    blob = open(capi.LIB_PATH, "rb").read()
    seen = {}
    for m in re.finditer(rb"\.name\xd9?.?(_ZN3xfa\d+fmha_bwd_mla_(?:pre|dkdv|dq)_kernel\w+)", blob):
        lo, hi = m.end(), m.end() + 600       # (a kernel's keys are sorted: these four follow .name)
        at = {key: blob.find(key, lo, hi) for key in (b".private_segment_fixed_size", b".vgpr_spill_count",
                                                      b".sgpr_spill_count", b".vgpr_count")}
        assert all(i > 0 for i in at.values()), m.group(1)
        seen[m.group(1).decode()] = {key.decode(): _msgpack_uint(blob, i + len(key)) for key, i in at.items()}
    print(seen)
    for kern, count in (("pre", 1), ("dkdv", 4), ("dq", 4)):
        for dt in ("IDF16b", "IDF16_"):
            hits = [v for n, v in seen.items() if f"fmha_bwd_mla_{kern}_kernel{dt}" in n]
            assert len(hits) == count, (kern, dt, list(seen))
            for v in hits:
                assert v[".private_segment_fixed_size"] == 0, (kern, dt, v)
                assert v[".vgpr_spill_count"] == 0 and v[".sgpr_spill_count"] == 0, (kern, dt, v)
                assert v[".vgpr_count"] <= 512, (kern, dt, v)


# ------------------------------------------------------------------ refusals --------------
FAKE = 0x10000        # 16-byte aligned, never dereferenced: every case fails before a launch
PTRS = dict(dout=FAKE, q=FAKE + (1 << 30), k=FAKE + (1 << 29), v=FAKE + (3 << 28), out=FAKE + (1 << 27),
            lse=FAKE + (1 << 26), dq=FAKE + (1 << 25), dk=FAKE + (1 << 24), dv=FAKE + (1 << 23), softmax_d=None)
ORDER = ("q", "k", "v", "out", "dout", "dq", "dk", "dv")


def _strides(per, sq=64, sk=64, h=4, hk=2):
    st = []
    for n in ORDER:
        rows, heads = (sq, h) if n in ("q", "out", "dout", "dq") else (sk, hk)
        w = 192 if n in ("q", "k", "dq", "dk") else 128
        st += [rows * heads * w, heads * w, w][3 - per:]
    return st


def _st(per, name, i, val):
    st = _strides(per)
    st[ORDER.index(name) * per + i] = val
    return st


def _dense(sq=64, sk=64, b=2, h=4, hk=2, dqk=192, dv_=128, st=None, null_st=False, **ptrs):
    L = capi.lib()
    p = dict(PTRS, **ptrs)
    st = _strides(3) if st is None else st
    L.fmha_bwd_mla(*(p[n] for n in ("dout", "q", "k", "v", "out", "lse", "dq", "dk", "dv", "softmax_d")), sq, sk,
                   b, h, hk, dqk, dv_, None if null_st else (C.c_int64 * 24)(*st), 192 ** -0.5, -1, 0, False, None)
    return L.fmha_last_status(), L.fmha_last_error().decode(), L.fmha_last_kernel().decode()


def _varlen(cq=FAKE + (1 << 22), ck=FAKE + (1 << 21), max_q=64, max_k=64, total_q=128, total_k=128, b=2, h=4,
            hk=2, dqk=192, dv_=128, st=None, null_st=False, **ptrs):
    L = capi.lib()
    p = dict(PTRS, **ptrs)
    st = _strides(2) if st is None else st
    L.fmha_varlen_bwd_mla(*(p[n] for n in ("dout", "q", "k", "v", "out", "lse", "dq", "dk", "dv", "softmax_d")),
                          cq, ck, max_q, max_k, total_q, total_k, b, h, hk, dqk, dv_,
                          None if null_st else (C.c_int64 * 16)(*st), 192 ** -0.5, -1, 0, False, None)
    return L.fmha_last_status(), L.fmha_last_error().decode(), L.fmha_last_kernel().decode()


COMMON = [
    (dict(dqk=128, dv_=128), "MLA prefill supports (head_size_qk, head_size_v) = (192, 128) only (got (128, 128))"),
    (dict(dqk=192, dv_=192), "(192, 128) only (got (192, 192))"),
    (dict(q=None), "q/k/v/o must be non-null device pointers"),
    (dict(v=None), "q/k/v/o must be non-null device pointers"),
    (dict(out=None), "q/k/v/o must be non-null device pointers"),
    (dict(dout=None), "dout must be a non-null device pointer"),
    (dict(lse=None), "softmax_lse must be a non-null device pointer"),
    (dict(dq=None), "dq must be a non-null device pointer"),
    (dict(dk=None), "dk must be a non-null device pointer"),
    (dict(dv=None), "dv must be a non-null device pointer"),
    (dict(b=0), "batch size must be positive (got 0)"),
    (dict(h=3, hk=2), "Number of heads in key/value must divide number of heads in query (h=3, hk=2)"),
    (dict(k=FAKE + 8), "q/k/v/o must be 16-byte aligned device pointers"),
    (dict(dout=FAKE + 8), "dout must be a 16-byte aligned device pointer"),
    (dict(dk=FAKE + 8), "dk must be a 16-byte aligned device pointer"),
    (dict(lse=FAKE + 2), "softmax_lse and softmax_d must be 4-byte aligned device pointers"),
    (dict(softmax_d=FAKE + 2), "softmax_lse and softmax_d must be 4-byte aligned device pointers"),
    (dict(null_st=True), "strides must be non-null"),
]


@pytest.mark.parametrize("over,msg", COMMON + [
    (dict(sk=0), "seqlen_q/seqlen_k must be positive (64, 0)"),
    (dict(sq=0), "seqlen_q/seqlen_k must be positive (0, 64)"),
    (dict(st=_st(3, "dout", 1, -512)), "strides must be non-negative: dout stride 1 is -512"),
    (dict(st=_st(3, "dq", 1, 772)), "strides must be multiples of 8 elements (16 bytes): dq stride 1 is 772"),
    (dict(st=_st(3, "dv", 1, 120)), "dv row stride must be at least its head size 128 (got 120)"),
    (dict(st=_st(3, "dk", 1, 128)), "dk row stride must be at least its head size 192 (got 128)"),
    (dict(st=_st(3, "k", 1, 128)), "k row stride must be at least its head size 192 (got 128)"),
    (dict(st=_st(3, "out", 1, 1 << 26)), "out: one sequence spans"),
], ids=lambda x: None if isinstance(x, str) else "-".join(f"{k}" for k in x))
def test_dense_entry_refusals(over, msg):
    status, got, kern = _dense(**over)
    assert status == 1 and msg in got, (status, got)
    assert kern == ""


@pytest.mark.parametrize("over,msg", COMMON + [
    (dict(cq=None), "cu_seqlens_q and cu_seqlens_k must be given"),
    (dict(ck=None), "cu_seqlens_q and cu_seqlens_k must be given"),
    (dict(cq=FAKE + 2), "cu_seqlens_q and cu_seqlens_k must be 4-byte aligned device pointers"),
    (dict(max_q=0), "max_seqlen_q must be positive (got 0)"),
    (dict(max_k=0), "max_seqlen_k must be positive (got 0): nothing to attend to"),
    (dict(total_q=0), "total_q and total_k must be positive (0, 128)"),
    (dict(total_k=0), "total_q and total_k must be positive (128, 0)"),
    (dict(st=_st(2, "q", 0, -768)), "strides must be non-negative: q stride 0 is -768"),
    (dict(st=_st(2, "dv", 0, 120)), "dv row stride must be at least its head size 128 (got 120)"),
    (dict(st=_st(2, "dout", 1, 132)), "strides must be multiples of 8 elements (16 bytes): dout stride 1 is 132"),
], ids=lambda x: None if isinstance(x, str) else "-".join(f"{k}" for k in x))
def test_varlen_entry_refusals(over, msg):
    status, got, kern = _varlen(**over)
    assert status == 1 and msg in got, (status, got)
    assert kern == ""


def test_a_refusal_is_cleared_by_the_next_call():
    assert _dense(dqk=128)[0] == 1
    status, msg, _ = _varlen(dq=None)
    assert status == 1 and msg == "dq must be a non-null device pointer"


def _t(*shape, dtype=torch.bfloat16, grad=False):
    return torch.zeros(*shape, dtype=dtype, requires_grad=grad)


def test_wrapper_refusals_by_name():
    import xf_flash_attention_cutlass_amd as xfa
    q, k, v = _t(1, 8, 4, 192), _t(1, 8, 2, 192), _t(1, 8, 2, 128)
    cu = torch.tensor([0, 8], dtype=torch.int32)
    with pytest.raises(NotImplementedError, match=r"\(192, 192, 128\) only \(got \(128, 128, 128\)\)"):
        xfa.flash_attn_mla_func(_t(1, 8, 4, 128), _t(1, 8, 2, 128), v)
    with pytest.raises(NotImplementedError, match=r"\(192, 192, 128\) only \(got \(192, 192, 192\)\)"):
        xfa.flash_attn_mla_varlen_func(q[0], k[0], _t(8, 2, 192), cu, cu, 8, 8)
    with pytest.raises(NotImplementedError, match="q.dtype=torch.float32"):
        xfa.flash_attn_mla_func(q.float(), k.float(), v.float())
    # past the wrapper's checks: the op refuses CPU tensors, with or without a gradient asked for
    with pytest.raises(RuntimeError, match="must be on CUDA"):
        xfa.flash_attn_mla_func(q, k, v, causal=True, deterministic=True)
    with pytest.raises(RuntimeError, match="must be on CUDA"):
        xfa.flash_attn_mla_varlen_func(_t(8, 4, 192, grad=True), k[0], v[0], cu, cu, 8, 8)
    # flash_attn_func keeps its refusal at this shape and now names the way out
    for fn, args in ((xfa.flash_attn_func, (_t(1, 8, 4, 192, grad=True), k, v)),
                     (xfa.flash_attn_varlen_func, (_t(8, 4, 192, grad=True), k[0], v[0], cu, cu, 8, 8))):
        with pytest.raises(NotImplementedError, match="q.requires_grad") as e:
            fn(*args)
        assert "flash_attn_mla_func" in str(e.value) and "flash_attn_mla_varlen_func" in str(e.value)
