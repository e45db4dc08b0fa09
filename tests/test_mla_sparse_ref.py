"""CPU: the sparse MLA decode (ABI 2.11) - its surface, the refusals of both
entries that need no device, the code objects of both kernels, and the pass rule of the GPU tests
against planted defects.

* fmha_mla_decode_sparse and fmha_mla_decode_sparse_fp8 are declared, exported and bound, the
  version is >= 2.11, neither op is in dir(paged_attn), and flash_mla_with_kvcache takes `indices`
  as a keyword-only argument that defaults to None;
* each refusal is reported through fmha_last_error with nothing launched (fake aligned pointers:
  nothing can be written); an empty batch is accepted;
* both instances of both kernels are in the gfx950 code object with no scratch and no spill;
* the per-(batch, pos) rule of tests/mla_sparse_util.py accepts a correct sparse split decode
  emulated on the CPU and rejects each of six planted defects, at topk 65 and 300, 16 heads,
  seqlen_q 2, both dtypes, over the 16-bit rows and the fp8 operand.
"""
import ctypes as C
import inspect
import re

import pytest
import torch

from tests import mla_sparse_util as su
from tests.test_mla_ref import _msgpack_uint
from xf_flash_attention_cutlass_amd import capi

DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
SYMS = ("fmha_mla_decode_sparse", "fmha_mla_decode_sparse_fp8")


# ------------------------------------------------------------------ surface ---------------
def test_surface_2_11():
    import xf_flash_attention_cutlass_amd as xfa
    from tests.test_abi import header_symbols
    for sym in SYMS:
        assert sym in header_symbols() and sym in capi.EXPORTED and hasattr(capi.lib(), sym)
    ver = capi.lib().fmha_version().decode().split()[1]
    assert tuple(int(x) for x in ver.split(".")) >= (2, 11)
    for op in ("mla_decode_sparse", "mla_decode_sparse_fp8"):
        assert callable(getattr(xfa.paged_attn, op))
        assert getattr(xfa.paged_attn, op) is getattr(xfa.paged_attn, "_" + op)
        assert op not in dir(xfa.paged_attn)
    par = inspect.signature(xfa.flash_mla_with_kvcache).parameters
    assert list(par)[-1] == "indices"
    assert par["indices"].kind is inspect.Parameter.KEYWORD_ONLY and par["indices"].default is None
    assert "indices" in xfa.flash_mla_with_kvcache.__doc__


def test_wrapper_refuses_causal_with_indices_and_cpu_tensors():
    import xf_flash_attention_cutlass_amd as xfa
    q = torch.zeros(1, 1, 16, 576, dtype=torch.bfloat16)
    kv = torch.zeros(4, 16, 1, 576, dtype=torch.bfloat16)
    ind = torch.zeros(1, 1, 8, dtype=torch.int32)
    with pytest.raises(ValueError, match="causal"):
        xfa.flash_mla_with_kvcache(q, kv, None, None, causal=True, indices=ind)
    with pytest.raises(RuntimeError, match="must be on CUDA"):
        xfa.flash_mla_with_kvcache(q, kv, None, None, indices=ind)
    with pytest.raises(TypeError):
        xfa.flash_mla_with_kvcache(q, kv, None, None, 512, None, False, 0, None, ind)   # keyword only


def test_code_objects_have_no_scratch_and_no_spill():
    """Both instances of both sparse kernels are in the library's gfx950 code object with
    private_segment_fixed_size 0 and no spilled register (scalar or vector)."""
    blob = open(capi.LIB_PATH, "rb").read()
    seen = {}
    for m in re.finditer(rb"\.name\xd9?.?(_ZN3xfa29fmha_mla_decode_sparse_kernel\w+|_ZN3xfa33fmha_mla_decode_sparse_fp8_kernel\w+)", blob):
        i = blob.find(b".private_segment_fixed_size", m.end(), m.end() + 64)
        s = blob.find(b".sgpr_spill_count", i, i + 400)
        k = blob.find(b".vgpr_spill_count", i, i + 400)
        assert i > 0 and s > 0 and k > 0, m.group(1)
        seen[m.group(1).decode()] = (_msgpack_uint(blob, i + 27), _msgpack_uint(blob, s + 17), _msgpack_uint(blob, k + 17))
    print(seen)
    for tag in ("decode_sparse_kernelIDF16_E", "decode_sparse_kernelIDF16bE",
                "decode_sparse_fp8_kernelIDF16_E", "decode_sparse_fp8_kernelIDF16bE"):
        hits = [v for n, v in seen.items() if tag in n]
        assert hits and all(v == (0, 0, 0) for v in hits), (tag, seen)


# ------------------------------------------------------------------ refusals --------------
FAKE = 0x10000        # 16-byte aligned, never dereferenced: every case fails before a launch


def _sparse(sym, q=FAKE, kv=FAKE + (1 << 30), o=FAKE + (1 << 29), lse=FAKE + (3 << 28), ind=FAKE + (1 << 27),
            ind_b=300, ind_r=300, topk=300, sq=1, batch=2, heads=16, d=576, dv=512, blocks=64, page=16,
            strides="dense", splits=0):
    L = capi.lib()
    if strides == "dense":
        strides = [sq * heads * d, heads * d, d, sq * heads * dv, heads * dv, dv]
    st = None if strides is None else (C.c_int64 * 6)(*strides)
    getattr(L, sym)(q, kv, o, lse, ind, ind_b, ind_r, topk, sq, batch, heads, d, dv, blocks, page, st,
                    576 ** -0.5, splits, False, None)
    return L.fmha_last_status(), L.fmha_last_error().decode(), L.fmha_last_kernel().decode()


def _st(**over):
    s = [16 * 576, 16 * 576, 576, 16 * 512, 16 * 512, 512]
    for i, val in over.items():
        s[int(i[1:])] = val
    return s


@pytest.mark.parametrize("sym", SYMS)
@pytest.mark.parametrize("over,needle", [
    (dict(q=None), "q, kv_cache and o must be non-null"),
    (dict(kv=None), "q, kv_cache and o must be non-null"),
    (dict(o=None), "q, kv_cache and o must be non-null"),
    (dict(ind=None), "indices"),
    (dict(strides=None), "strides must be a non-null"),
    (dict(d=512), "(576, 512) only"),
    (dict(d=656), "(576, 512) only"),
    (dict(dv=576), "(576, 512) only"),
    (dict(topk=0), "topk must be at least 1"),
    (dict(topk=-5), "topk must be at least 1"),
    (dict(blocks=0), "num_blocks must be at least 1"),
    (dict(blocks=-1), "num_blocks must be at least 1"),
    (dict(page=24), "positive multiple of 16"),
    (dict(page=0), "positive multiple of 16"),
    (dict(page=-16), "positive multiple of 16"),
    (dict(heads=0), "at least 1"),
    (dict(sq=0), "at least 1"),
    (dict(batch=-1), "non-negative"),
    (dict(splits=129), "at most 128"),
    (dict(strides=_st(s2=580)), "multiples of 8"),
    (dict(strides=_st(s5=0)), "the output's positive"),
    (dict(strides=_st(s0=-9216)), "non-negative multiples of 8"),
    (dict(q=FAKE + 8), "16-byte aligned"),
    (dict(kv=FAKE + (1 << 30) + 8), "16-byte aligned"),
    (dict(o=FAKE + (1 << 29) + 2), "16-byte aligned"),
    (dict(ind=FAKE + (1 << 27) + 2), "4-byte aligned"),
    (dict(lse=FAKE + (3 << 28) + 1), "4-byte aligned"),
    (dict(ind_b=-300), "indices strides must be non-negative"),
    (dict(ind_r=-1), "indices strides must be non-negative"),
    (dict(batch=1 << 20, heads=128, sq=16), "more than one launch covers"),
])
def test_sparse_refusals(sym, over, needle):
    st, msg, kern = _sparse(sym, **over)
    assert st != 0 and needle in msg, msg
    assert kern == "" and capi.lib().fmha_last_num_splits() == 0     # nothing was launched


@pytest.mark.parametrize("sym", SYMS)
def test_sparse_accepts_empty_batch(sym):
    """batch_size == 0 passes every check, launches nothing and succeeds."""
    st, msg, kern = _sparse(sym, batch=0)
    assert st == 0 and msg == "" and kern == ""
    st, msg, kern = _sparse(sym, batch=0, topk=0)          # ... but is validated in full
    assert st != 0 and "topk" in msg


# ------------------------------------------------------------------ the pass rule ---------
_PROBLEMS = {}
SPLITS = 2       # 65 entries: tiles {0, 1} and {2}; 300: 5 + 5


def _problem(kind, dt, topk):
    """16 heads, seqlen_q 2, a batch of 2; (batch 0, pos 0) holds a whole invalid tile in the middle
    of its first split range, (batch 1, pos 0) duplicates; invalid values are sprinkled everywhere."""
    key = (kind, dt, topk)
    if key not in _PROBLEMS:
        p = su.make_problem(kind, DTYPES[dt], 16, 2, topk, b=2, seed=topk, invalid=0.15,
                            specials=("duplicates", "duplicates"))
        ind = p.indices.clone()
        ind[0, 0, su.TILE:2 * su.TILE] = torch.tensor([-1, su.num_slots(p), su.INT_MAX, su.INT_MIN]).repeat(8).int()
        p = su.with_indices(p, ind)
        table = torch.randperm(p.nblocks, generator=torch.Generator().manual_seed(3))
        _PROBLEMS[key] = (p, su.oracle(p), table)
    return _PROBLEMS[key]


@pytest.mark.parametrize("topk", [65, 300])
@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("kind", ["kv16", "fp8"])
def test_rule_accepts_the_correct_emulation(kind, dt, topk):
    p, ora, _ = _problem(kind, dt, topk)
    for splits in (1, SPLITS, 3):
        o, lse = su.emulate(p, splits)
        ok, figs = su.judge_each(o, lse, ora)
        print(kind, dt, topk, splits, [round(f["ratio"], 3) for f in figs], max(f["lse_err"] for f in figs))
        assert ok, figs
        assert max(f["ratio"] for f in figs) <= 0.6              # well inside: room for the kernel


@pytest.mark.parametrize("defect", su.DEFECTS)
@pytest.mark.parametrize("topk", [65, 300])
@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("kind", ["kv16", "fp8"])
def test_rule_rejects_planted_defect(kind, dt, topk, defect):
    p, ora, table = _problem(kind, dt, topk)
    o, lse = su.emulate(p, SPLITS, defect, table)
    ok, figs = su.judge_each(o, lse, ora)
    worst = max(f["ratio"] for f in figs)
    print(kind, dt, topk, defect, [round(f["ratio"], 2) for f in figs], [f["lse_err"] for f in figs])
    assert not ok and worst > 1.0


def test_the_inputs_exercise_every_defect():
    """What makes the defects visible: every (batch, pos) has its own slots, invalid entries of all
    four kinds, a duplicate, an invalid middle tile, and a last tile that is not full."""
    p, _, table = _problem("kv16", "bf16", 65)
    ind = p.indices.long()
    n = su.num_slots(p)
    assert not torch.equal(ind[0, 0], ind[0, 1]) and not torch.equal(ind[0, 1], ind[1, 0])
    for bad in (-1, n, su.INT_MAX, su.INT_MIN):
        assert (ind == bad).any()
    assert not su.valid_mask(ind[0, 0, 32:64], n).any() and su.valid_mask(ind[0, 0, :32], n).any()
    v = ind[1, 0][su.valid_mask(ind[1, 0], n)]
    assert v.unique().numel() < v.numel()
    assert ind.shape[-1] % su.TILE != 0 and not torch.equal(table, torch.arange(p.nblocks))
