"""CPU: the MLA prefill forward (ABI 2.12) - what it computes, the rule it is held
to, its surface and every refusal that needs no launch.

* In float64, the only route the library had before - V zero-padded to 192 columns, attention at
  D = 192, the output sliced to 128 - equals `attention_ref` with the 128-wide V to 1e-10: the
  oracle the GPU tests use is the padded route's result.
* `fwd_mla_util.emulate` restates the kernel's arithmetic tile by tile (64-key tiles, fp32
  accumulation, P rounded to the dtype, deferred rescale).  The correct emulation passes the
  project's forward rule per sequence; each planted defect (V taken as K's first 128 columns,
  scores over the first 128 features only, the scale of a 128-wide head, causal aligned top-left
  when sk != sq, output d-tile 3 dropped) is rejected on the longest sequence.  The ratios are
  printed (pytest -s) and recorded in DESIGN.md §3.11.
* The 2.12 surface and the refusals of the C entries and of the Python wrappers.
"""
import ctypes as C
import inspect
import re

import pytest
import torch

from oracle import attention_ref as orc
from tests import fwd_mla_util as mu
from xf_flash_attention_cutlass_amd import capi

H, HK = 6, 2


def test_padded_v_route_is_the_oracle_in_float64():
    g = torch.Generator().manual_seed(7)
    q = torch.randn(2, 37, H, mu.DQK, generator=g, dtype=torch.float64)
    k = torch.randn(2, 53, HK, mu.DQK, generator=g, dtype=torch.float64)
    v = torch.randn(2, 53, HK, mu.DV, generator=g, dtype=torch.float64)
    vp = torch.nn.functional.pad(v, (0, mu.DQK - mu.DV))
    for window in ((-1, -1), (-1, 0), (11, 0), (-1, 5)):
        want, _ = orc.attention_ref(q, k, v, window_size=window, upcast=False)
        got, _ = orc.attention_ref(q, k, vp, window_size=window, upcast=False)
        assert want.shape[-1] == mu.DV
        assert (got[..., :mu.DV] - want).abs().max().item() <= 1e-10
        assert got[..., mu.DV:].abs().max().item() == 0.0


@pytest.mark.parametrize("dt", list(mu.DTYPES))
@pytest.mark.parametrize("lens_k,window", [(mu.LENS_K, (-1, 0)), (mu.LENS_K, (-1, -1)), (mu.LENS_K_REV, (-1, 0)),
                                           (mu.LENS_K, (37, 0)), (mu.LENS_K, (-1, 20))],
                         ids=["causal", "full", "causal_rev", "w37_0", "w-1_20"])
def test_correct_emulation_passes_the_rule(dt, lens_k, window):
    q, k, v = mu.make_packed(mu.LENS_Q, lens_k, H, HK, mu.DTYPES[dt])
    seqs = mu.oracle(q, k, v, mu.LENS_Q, lens_k, window)
    o, lse = mu.emulate(q, k, v, mu.LENS_Q, lens_k, window)
    mu.assert_case(f"emulate {dt} {window} k{lens_k[0]}", o, lse, seqs, mu.LENS_Q)


@pytest.mark.parametrize("dt", list(mu.DTYPES))
@pytest.mark.parametrize("defect", mu.DEFECTS)
def test_planted_defects_are_rejected_on_the_longest_sequence(dt, defect):
    q, k, v = mu.make_packed(mu.LENS_Q, mu.LENS_K, H, HK, mu.DTYPES[dt])
    window = (-1, 0)
    seqs = mu.oracle(q, k, v, mu.LENS_Q, mu.LENS_K, window)
    o, lse = mu.emulate(q, k, v, mu.LENS_Q, mu.LENS_K, window, defect=defect)
    ok, figs = mu.judge_each(o, lse, seqs, mu.LENS_Q)
    longest = figs[0]                          # 300 queries over 333 keys
    print(f"defect {defect} {dt}: longest sequence o err / bound {longest['ratio']:.1f}, "
          f"lse err {longest['lse_err']:.3e}")
    assert not longest["ok"], (defect, longest)
    assert not ok


# ------------------------------------------------------------------ surface ---------------
SYMS = ("fmha_fwd_mla", "fmha_varlen_fwd_mla")


def test_surface_2_12():
    import xf_flash_attention_cutlass_amd as xfa
    from tests.test_abi import header_symbols
    for sym in SYMS:
        assert sym in header_symbols() and sym in capi.EXPORTED and hasattr(capi.lib(), sym)
    ver = capi.lib().fmha_version().decode().split()[1]
    assert tuple(int(x) for x in ver.split(".")) >= (2, 12)
    for op in ("fwd_mla", "varlen_fwd_mla"):
        assert callable(getattr(xfa.paged_attn, op))
        assert getattr(xfa.paged_attn, op) is getattr(xfa.paged_attn, "_" + op)
        assert op not in dir(xfa.paged_attn)
    for fn in (xfa.flash_attn_func, xfa.flash_attn_varlen_func):
        assert "MLA prefill" in fn.__doc__
    assert "block_table" in inspect.signature(xfa.flash_attn_varlen_func).parameters


def _msgpack_uint(blob, i):
    t = blob[i]
    if t < 0x80:
        return t
    return int.from_bytes(blob[i + 1:i + 1 + {0xcc: 1, 0xcd: 2, 0xce: 4}[t]], "big")


def test_code_objects_have_no_scratch_and_no_vector_spill():
    """The four instances (bf16 / fp16 x MASK) are in the library's gfx950 code object with
    private_segment_fixed_size 0 and no spilled vector register, in 144 KiB of dynamic LDS plus the
    item queue's 16 bytes.  (Scalars of the parameter block parked in VGPR lanes between items are
    counted as sgpr_spill_count; they cost no memory and are printed.)"""
    blob = open(capi.LIB_PATH, "rb").read()
    seen = {}
    for m in re.finditer(rb"\.name\xd9?.?(_ZN3xfa19fmha_fwd_mla_kernel\w+)", blob):
        lo, hi = m.start() - 600, m.end() + 600
        at = {key: blob.find(key, lo, hi) for key in (b".private_segment_fixed_size", b".vgpr_spill_count",
                                                      b".sgpr_spill_count", b".vgpr_count", b".group_segment_fixed_size")}
        assert all(i > 0 for i in at.values()), m.group(1)
        seen[m.group(1).decode()] = {key.decode(): _msgpack_uint(blob, i + len(key)) for key, i in at.items()}
    print(seen)
    for tag in ("IDF16bLi8ELb0E", "IDF16bLi8ELb1E", "IDF16_Li8ELb0E", "IDF16_Li8ELb1E"):
        hits = [v for n, v in seen.items() if tag in n]
        assert hits, (tag, list(seen))
        for v in hits:
            assert v[".private_segment_fixed_size"] == 0 and v[".vgpr_spill_count"] == 0, (tag, v)
            assert v[".vgpr_count"] <= 256 and v[".group_segment_fixed_size"] == 16, (tag, v)


# ------------------------------------------------------------------ refusals --------------
FAKE = 0x10000        # 16-byte aligned, never dereferenced: every case fails before a launch


def _dense(q=FAKE, k=FAKE + (1 << 30), v=FAKE + (1 << 29), o=FAKE + (3 << 28), lse=FAKE + (1 << 27), sq=64,
           sk=64, b=2, h=4, hk=2, dqk=192, dv=128, st=None, null_st=False, wl=-1, wr=0):
    L = capi.lib()
    if st is None:
        st = [sq * h * 192, h * 192, 192, sk * hk * 192, hk * 192, 192, sk * hk * 128, hk * 128, 128,
              sq * h * 128, h * 128, 128]
    L.fmha_fwd_mla(q, k, v, o, lse, sq, sk, b, h, hk, dqk, dv, None if null_st else (C.c_int64 * 12)(*st),
                   192 ** -0.5, wl, wr, False, None)
    return L.fmha_last_status(), L.fmha_last_error().decode(), L.fmha_last_kernel().decode()


def _varlen(q=FAKE, k=FAKE + (1 << 30), v=FAKE + (1 << 29), o=FAKE + (3 << 28), lse=FAKE + (1 << 27),
            cq=FAKE + (1 << 26), ck=FAKE + (1 << 25), used=None, max_q=64, max_k=64, total_q=128, b=2, h=4,
            hk=2, dqk=192, dv=128, st=None, null_st=False):
    L = capi.lib()
    if st is None:
        st = [h * 192, 192, hk * 192, 192, hk * 128, 128, h * 128, 128]
    L.fmha_varlen_fwd_mla(q, k, v, o, lse, cq, ck, used, max_q, max_k, total_q, b, h, hk, dqk, dv,
                          None if null_st else (C.c_int64 * 8)(*st), 192 ** -0.5, -1, 0, False, None)
    return L.fmha_last_status(), L.fmha_last_error().decode(), L.fmha_last_kernel().decode()


def _st(i, val, n=12):
    st = ([64 * 4 * 192, 4 * 192, 192, 64 * 2 * 192, 2 * 192, 192, 64 * 2 * 128, 2 * 128, 128,
           64 * 4 * 128, 4 * 128, 128] if n == 12 else [4 * 192, 192, 2 * 192, 192, 2 * 128, 128, 4 * 128, 128])
    st[i] = val
    return st


COMMON = [
    (dict(dqk=128, dv=128), "(192, 128) only"),
    (dict(dqk=192, dv=192), "(192, 128) only"),
    (dict(dqk=576, dv=512), "(192, 128) only"),
    (dict(q=None), "non-null"),
    (dict(v=None), "non-null"),
    (dict(o=None), "non-null"),
    (dict(b=0), "batch size"),
    (dict(h=3, hk=2), "must divide"),
    (dict(k=FAKE + 8), "16-byte aligned"),
    (dict(null_st=True), "strides must be non-null"),
    (dict(lse=FAKE + 2), "4-byte aligned"),
]


@pytest.mark.parametrize("over,needle", COMMON + [
    (dict(sk=0), "positive"),
    (dict(sq=0), "positive"),
    (dict(st=_st(1, -768)), "non-negative"),
    (dict(st=_st(4, 388)), "multiples of 8"),
    (dict(st=_st(7, 120)), "at least its head size 128"),
    (dict(st=_st(4, 128)), "at least its head size 192"),
    (dict(st=_st(4, 1 << 26), sk=64), "32-bit offsets"),
])
def test_dense_entry_refusals(over, needle):
    status, msg, kern = _dense(**over)
    assert status != 0 and needle in msg, (status, msg)
    assert kern == ""


@pytest.mark.parametrize("over,needle", COMMON + [
    (dict(cq=None), "cu_seqlens_q and cu_seqlens_k"),
    (dict(ck=None), "cu_seqlens_q and cu_seqlens_k"),
    (dict(max_k=0), "nothing to attend to"),
    (dict(max_q=0), "max_seqlen_q"),
    (dict(total_q=0), "total_q"),
    (dict(st=_st(0, -768, 8)), "non-negative"),
    (dict(st=_st(2, 388, 8)), "multiples of 8"),
    (dict(st=_st(4, 120, 8)), "at least its head size 128"),
    (dict(used=FAKE + 2), "4-byte aligned"),
])
def test_varlen_entry_refusals(over, needle):
    status, msg, kern = _varlen(**over)
    assert status != 0 and needle in msg, (status, msg)
    assert kern == ""


def test_a_refusal_is_cleared_by_the_next_call():
    assert _dense(dqk=128)[0] != 0
    status, msg, _ = _dense(b=0)
    assert status != 0 and "batch size" in msg


def _t(*shape, dtype=torch.bfloat16, grad=False):
    return torch.zeros(*shape, dtype=dtype, requires_grad=grad)


@pytest.mark.parametrize("kw,exc,needle", [
    (dict(dropout_p=0.1), NotImplementedError, "dropout_p"),
    (dict(alibi_slopes=torch.zeros(4)), NotImplementedError, "alibi_slopes"),
    (dict(softcap=30.0), NotImplementedError, "softcap"),
    (dict(sink=torch.zeros(4)), NotImplementedError, "sink"),
])
def test_flash_attn_func_refuses_by_argument_name(kw, exc, needle):
    import xf_flash_attention_cutlass_amd as xfa
    q, k, v = _t(1, 8, 4, 192), _t(1, 8, 2, 192), _t(1, 8, 2, 128)
    with pytest.raises(exc, match=needle):
        xfa.flash_attn_func(q, k, v, **kw)
    cu = torch.tensor([0, 8], dtype=torch.int32)
    with pytest.raises(exc, match=needle):
        xfa.flash_attn_varlen_func(q[0], k[0], v[0], cu, cu, 8, 8, **kw)


def test_wrappers_refuse_other_pairs_block_table_grad_and_cpu():
    import xf_flash_attention_cutlass_amd as xfa
    cu = torch.tensor([0, 8], dtype=torch.int32)
    for dq, dk, dv in ((192, 192, 64), (128, 128, 64), (192, 128, 128), (576, 576, 512)):
        q, k, v = _t(1, 8, 4, dq), _t(1, 8, 2, dk), _t(1, 8, 2, dv)
        with pytest.raises(NotImplementedError, match=r"\(192, 128\) only"):
            xfa.flash_attn_func(q, k, v)
        with pytest.raises(NotImplementedError, match=r"\(192, 128\) only"):
            xfa.flash_attn_varlen_func(q[0], k[0], v[0], cu, cu, 8, 8)
    q, k, v = _t(8, 4, 192), _t(8, 2, 192), _t(8, 2, 128)
    with pytest.raises(NotImplementedError, match="block_table"):
        xfa.flash_attn_varlen_func(q, k, v, cu, cu, 8, 8, block_table=torch.zeros(1, 1, dtype=torch.int32))
    for i, name in enumerate("qkv"):
        args = [_t(1, 8, 4, 192, grad=i == 0), _t(1, 8, 2, 192, grad=i == 1), _t(1, 8, 2, 128, grad=i == 2)]
        with pytest.raises(NotImplementedError, match=f"{name}.requires_grad"):
            xfa.flash_attn_func(*args)
        with torch.no_grad(), pytest.raises(RuntimeError, match="must be on CUDA"):
            xfa.flash_attn_func(*args)           # past the wrapper's checks: the op refuses CPU tensors
    with pytest.raises(RuntimeError, match="must be on CUDA"):
        xfa.flash_attn_func(_t(1, 8, 4, 192), _t(1, 8, 2, 192), _t(1, 8, 2, 128), causal=True)
    with pytest.raises(NotImplementedError, match="fp8"):
        xfa.flash_attn_func(_t(1, 8, 4, 192).to(torch.float8_e4m3fn), _t(1, 8, 2, 192).to(torch.float8_e4m3fn),
                            _t(1, 8, 2, 128).to(torch.float8_e4m3fn))


def test_equal_head_sizes_do_not_reach_the_new_path():
    """v as wide as q takes the branch it always took: the op the wrapper reaches is `fwd`, whose
    own check fires on a CPU tensor (no MLA message)."""
    import xf_flash_attention_cutlass_amd as xfa
    q, k, v = _t(1, 8, 4, 192), _t(1, 8, 2, 192), _t(1, 8, 2, 192)
    with pytest.raises(RuntimeError) as e:
        xfa.flash_attn_func(q, k, v)
    assert "MLA" not in str(e.value)
