"""CPU: the fp8 latent cache of the MLA decode (ABI 2.10) - the row and the
quantiser as tests/mla_fp8_util.py restates them, the pass rule of the GPU tests against planted
defects, the 2.10 surface, and the refusals of both new entries that need no device.

* pack / unpack of the 656-byte row round-trips; the quantiser gives descale 1.0 and zero bytes for
  an all-zero group and 0x7E / 0xFE for +-amax;
* the per-sequence rule of tests/mla_util.py, against the oracle over the operand (the dequantised
  rows rounded to q's dtype), accepts a correct split decode over that operand and rejects each of
  five planted defects - descales 1 and 2 swapped, descales ignored, the previous row's descales,
  descale 0 for all four groups, the rotary features read 16 bytes off - on a single 16-head
  sequence of 517, 65 and 33 keys, in both dtypes;
* fmha_mla_decode_fp8 and fmha_mla_cache_append_fp8 are declared, exported and bound, the version
  is >= 2.10, neither op is in dir(paged_attn), and each refusal is reported through
  fmha_last_error (fake pointers: nothing is launched, nothing can be written);
* the fp8 kernel's code objects have no scratch and no spilled register.
"""
import ctypes as C
import re

import pytest
import torch

from tests import mla_fp8_util as m8
from tests import mla_util as mu
from tests.test_mla_ref import _msgpack_uint
from xf_flash_attention_cutlass_amd import capi

DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}


# ------------------------------------------------------------------ row and quantiser -----
@pytest.mark.parametrize("dt", list(DTYPES))
def test_pack_unpack_round_trip(dt):
    g = torch.Generator().manual_seed(1)
    b8 = torch.randint(0, 256, (37, 512), generator=g, dtype=torch.uint8)
    ds = torch.rand(37, 4, generator=g) + 0.01
    rope = torch.randn(37, 64, generator=g).to(DTYPES[dt])
    rows = m8.pack_rows(b8, ds, rope)
    assert rows.shape == (37, m8.ROW) and rows.dtype == torch.uint8
    b8b, dsb, ropeb = m8.unpack_rows(rows, DTYPES[dt])
    assert torch.equal(b8b, b8) and torch.equal(dsb, ds) and torch.equal(ropeb, rope)
    # the layout: bytes 0..511, then the four descales, then the rotary features
    assert torch.equal(rows[:, 512:516].contiguous().view(torch.float32)[:, 0], ds[:, 0])
    assert torch.equal(rows[:, 654:656].contiguous().view(DTYPES[dt])[:, 0], rope[:, 63])


@pytest.mark.parametrize("dt", list(DTYPES))
def test_quantiser_zero_group_and_amax(dt):
    g = torch.Generator().manual_seed(2)
    x = torch.randn(5, 512, generator=g).to(DTYPES[dt])
    x[1, 128:256] = 0                                   # an all-zero group
    x[2, 256:384] = x[2, 256:384].clamp(-1, 1)
    x[2, 300], x[2, 301] = 3.5, -3.5                    # +-amax of its group
    b8, ds = m8.quantize_ref(x)
    assert ds.dtype == torch.float32 and ds.shape == (5, 4)
    assert ds[1, 1].item() == 1.0 and int(b8[1, 128:256].max()) == 0
    assert ds[2, 2].item() == torch.tensor(3.5) / 448.0
    assert b8[2, 300].item() == 0x7E and b8[2, 301].item() == 0xFE
    # every group reaches +-448 somewhere (its amax), nothing is NaN (0x7F / 0xFF)
    mag = (b8 & 0x7F).reshape(5, 4, 128).amax(-1)
    assert torch.equal(mag == 0x7E, ds != 1.0) and int((b8 & 0x7F).max()) == 0x7E
    # the operand reproduces the input to e4m3's 2^-4 relative step of the group's amax
    rows = m8.pack_rows(b8, ds, torch.zeros(5, 64, dtype=DTYPES[dt]))
    op = m8.operand(rows, DTYPES[dt])[:, :512]
    amax = x.float().reshape(5, 4, 128).abs().amax(-1, keepdim=True).expand(5, 4, 128).reshape(5, 512)
    assert ((op - x.float()).abs() <= amax / 16 + 1e-6).all()


# ------------------------------------------------------------------ the pass rule ---------
_PROBLEMS = {}


def _problem(dt, n):
    if (dt, n) not in _PROBLEMS:
        c = m8.make_cache8([n], DTYPES[dt], seed=n)
        q = mu.make_q(1, 1, 16, mu.D, DTYPES[dt], n)
        _PROBLEMS[dt, n] = (c, q, mu.oracle(c, q, False))
    return _PROBLEMS[dt, n]


@pytest.mark.parametrize("n", [517, 65, 33])
@pytest.mark.parametrize("dt", list(DTYPES))
def test_rule_accepts_decode_over_the_operand(dt, n):
    c, q, ora = _problem(dt, n)
    o, lse = mu.emulate(m8.as_cache16(c), q, 3)
    ok, figs = mu.judge_each(o, lse, ora)
    print(dt, n, round(figs[0]["ratio"], 3), figs[0]["lse_err"])
    assert ok, figs
    assert figs[0]["ratio"] <= 0.6                       # well inside: the rule has room for the kernel


@pytest.mark.parametrize("defect", m8.DEFECTS)
@pytest.mark.parametrize("n", [517, 65, 33])
@pytest.mark.parametrize("dt", list(DTYPES))
def test_rule_rejects_planted_defect(dt, n, defect):
    c, q, ora = _problem(dt, n)
    o, lse = mu.emulate(m8.as_cache16(c, defect), q, 3)
    ok, figs = mu.judge_each(o, lse, ora)
    print(dt, n, defect, round(figs[0]["ratio"], 2), figs[0]["lse_err"])
    assert not ok and figs[0]["ratio"] > 1.0


def test_groups_of_the_inputs_differ():
    """What makes the swap defects visible: the descales of a row differ by large factors."""
    c, _, _ = _problem("bf16", 65)
    _, ds, _ = m8.unpack_rows(c.rows[0], torch.bfloat16)
    assert (ds[:, 2] > 32 * ds[:, 1]).all() and (ds[:, 3] > 4 * ds[:, 1]).all()
    assert ds[40:, 0].mean() > 2 * ds[:20, 0].mean()


# ------------------------------------------------------------------ surface ---------------
def test_surface_2_10():
    import xf_flash_attention_cutlass_amd as xfa
    from tests.test_abi import header_symbols
    for sym in ("fmha_mla_decode_fp8", "fmha_mla_cache_append_fp8"):
        assert sym in header_symbols() and sym in capi.EXPORTED and hasattr(capi.lib(), sym)
    ver = capi.lib().fmha_version().decode().split()[1]
    assert tuple(int(x) for x in ver.split(".")) >= (2, 10)
    for op in ("mla_decode_fp8", "mla_cache_append_fp8"):
        assert callable(getattr(xfa.paged_attn, op))
        assert getattr(xfa.paged_attn, op) is getattr(xfa.paged_attn, "_" + op)
        assert op not in dir(xfa.paged_attn)
    assert xfa.mla_fp8_cache_row_bytes == m8.ROW == 656
    for name in ("mla_cache_append_fp8", "mla_fp8_cache_row_bytes"):
        assert name in xfa.__all__
    assert callable(xfa.mla_cache_append_fp8)


def test_fp8_code_objects_have_no_scratch_and_no_spill():
    """Both instances of the fp8 decode kernel and of the append kernel are in the library's gfx950
    code object with private_segment_fixed_size 0 and no spilled register (scalar or vector)."""
    blob = open(capi.LIB_PATH, "rb").read()
    seen = {}
    for m in re.finditer(rb"\.name\xd9?.?(_ZN3xfa26fmha_mla_decode_fp8_kernel\w+|_ZN3xfa26fmha_mla_append_fp8_kernel\w+)", blob):
        i = blob.find(b".private_segment_fixed_size", m.end(), m.end() + 64)
        s = blob.find(b".sgpr_spill_count", i, i + 400)
        k = blob.find(b".vgpr_spill_count", i, i + 400)
        assert i > 0 and s > 0 and k > 0, m.group(1)
        seen[m.group(1).decode()] = (_msgpack_uint(blob, i + 27), _msgpack_uint(blob, s + 17), _msgpack_uint(blob, k + 17))
    print(seen)
    for tag in ("decode_fp8_kernelIDF16_E", "decode_fp8_kernelIDF16bE", "append_fp8_kernelIDF16_E", "append_fp8_kernelIDF16bE"):
        hits = [v for n, v in seen.items() if tag in n]
        assert hits and all(v == (0, 0, 0) for v in hits), (tag, seen)


# ------------------------------------------------------------------ refusals --------------
FAKE = 0x10000        # 16-byte aligned, never dereferenced: every case fails before a launch


def _decode8(q=FAKE, kv=FAKE + (1 << 30), o=FAKE + (1 << 29), lse=FAKE + (3 << 28), table=FAKE + (1 << 27),
             lens=FAKE + (1 << 26), bt_stride=64, sq=1, max_sk=1024, batch=2, heads=16, d=576, dv=512,
             page=16, strides="dense", window=(-1, -1), splits=0):
    L = capi.lib()
    if strides == "dense":
        strides = [sq * heads * d, heads * d, d, sq * heads * dv, heads * dv, dv]
    st = None if strides is None else (C.c_int64 * 6)(*strides)
    L.fmha_mla_decode_fp8(q, kv, o, lse, table, bt_stride, lens, sq, max_sk, batch, heads, d, dv, page, st,
                          576 ** -0.5, window[0], window[1], splits, False, None)
    return L.fmha_last_status(), L.fmha_last_error().decode(), L.fmha_last_kernel().decode()


def _st(**over):
    s = [16 * 576, 16 * 576, 576, 16 * 512, 16 * 512, 512]
    for i, val in over.items():
        s[int(i[1:])] = val
    return s


@pytest.mark.parametrize("over,needle", [
    (dict(q=None), "q, kv_cache and o must be non-null"),
    (dict(kv=None), "q, kv_cache and o must be non-null"),
    (dict(o=None), "q, kv_cache and o must be non-null"),
    (dict(table=None), "block_table"),
    (dict(lens=None), "cache_seqlens must be a non-null"),
    (dict(strides=None), "strides must be a non-null"),
    (dict(d=512), "(576, 512) only"),
    (dict(d=656), "(576, 512) only"),
    (dict(dv=576), "(576, 512) only"),
    (dict(page=24), "multiple of 16"),
    (dict(page=0), "multiple of 16"),
    (dict(window=(-1, 5)), "(-1, -1) and (-1, 0)"),
    (dict(window=(64, 0)), "(-1, -1) and (-1, 0)"),
    (dict(heads=0), "at least 1"),
    (dict(sq=0), "at least 1"),
    (dict(batch=-1), "non-negative"),
    (dict(splits=129), "at most 128"),
    (dict(max_sk=1025), "max_seqlen_k must lie in"),
    (dict(strides=_st(s2=580)), "multiples of 8"),
    (dict(strides=_st(s5=0)), "the output's positive"),
    (dict(q=FAKE + 8), "16-byte aligned"),
    (dict(kv=FAKE + (1 << 30) + 8), "16-byte aligned"),
    (dict(lens=FAKE + (1 << 26) + 2), "4-byte aligned"),
    (dict(page=3273632, max_sk=64), "kv_cache page: one sequence spans"),     # x 656 bytes: past the limit
])
def test_decode_fp8_refusals(over, needle):
    st, msg, kern = _decode8(**over)
    assert st != 0 and needle in msg, msg
    assert kern == "" and capi.lib().fmha_last_num_splits() == 0     # nothing was launched


def test_decode_fp8_slab_is_judged_at_656_bytes():
    """A page the 16-bit entry refuses (its slab is 1152 bytes a row) but whose 656-byte rows fit
    passes every check here (an empty batch: validated in full, nothing launched)."""
    st, msg, kern = _decode8(page=1864144, max_sk=64, batch=0)
    assert st == 0 and msg == "" and kern == ""
    L = capi.lib()
    stv = (C.c_int64 * 6)(*_st())
    L.fmha_mla_decode(FAKE, FAKE + (1 << 30), FAKE + (1 << 29), None, FAKE + (1 << 27), 64, FAKE + (1 << 26), 1, 64,
                      0, 16, 576, 512, 1864144, stv, 576 ** -0.5, -1, -1, 0, False, None)
    assert L.fmha_last_status() != 0 and "kv_cache page" in L.fmha_last_error().decode()


def test_decode_fp8_accepts_empty_batch():
    st, msg, kern = _decode8(batch=0)
    assert st == 0 and msg == "" and kern == ""


def _append8(latent=FAKE, ls=576, pe=FAKE + 1024, ps=576, cache=FAKE + (1 << 30), slots=FAKE + (1 << 27),
             tokens=8, blocks=4, page=16):
    L = capi.lib()
    L.fmha_mla_cache_append_fp8(latent, ls, pe, ps, cache, slots, tokens, blocks, page, False, None)
    return L.fmha_last_status(), L.fmha_last_error().decode()


@pytest.mark.parametrize("over,needle", [
    (dict(latent=None), "must be non-null"),
    (dict(pe=None), "must be non-null"),
    (dict(cache=None), "must be non-null"),
    (dict(slots=None), "must be non-null"),
    (dict(ls=580), "multiples of 8"),
    (dict(ps=68), "multiples of 8"),
    (dict(ls=-576), "non-negative multiples of 8"),
    (dict(latent=FAKE + 8), "16-byte aligned"),
    (dict(pe=FAKE + 1024 + 2), "16-byte aligned"),
    (dict(cache=FAKE + (1 << 30) + 4), "16-byte aligned"),
    (dict(slots=FAKE + (1 << 27) + 4), "8-byte aligned"),
    (dict(page=24), "multiple of 16"),
    (dict(page=0), "multiple of 16"),
    (dict(tokens=-1), "non-negative"),
    (dict(blocks=-1), "non-negative"),
])
def test_append_fp8_refusals(over, needle):
    st, msg = _append8(**over)
    assert st != 0 and needle in msg, msg


def test_append_fp8_accepts_zero_tokens():
    """num_tokens == 0 passes validation, launches nothing and succeeds (no pointer is read)."""
    st, msg = _append8(tokens=0)
    assert st == 0 and msg == ""


def test_python_refusals():
    import xf_flash_attention_cutlass_amd as xfa
    q = torch.zeros(1, 1, 16, 576, dtype=torch.bfloat16)
    kv8 = torch.zeros(4, 16, 1, 656, dtype=torch.uint8)
    tab = torch.zeros(1, 4, dtype=torch.int32)
    lens = torch.zeros(1, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="must be on CUDA"):
        xfa.flash_mla_with_kvcache(q, kv8, tab, lens)
    with pytest.raises(RuntimeError, match="must be on CUDA"):
        xfa.flash_mla_with_kvcache(q, kv8.view(torch.float8_e4m3fn), tab, lens)
    with pytest.raises(RuntimeError, match="must be on CUDA"):
        xfa.mla_cache_append_fp8(q[0, 0, :, :512], q[0, 0, :, 512:], kv8, torch.zeros(16, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="fp16 or bf16"):
        xfa.mla_cache_append_fp8(q[0, 0, :, :512].float(), q[0, 0, :, 512:], kv8, torch.zeros(16, dtype=torch.int64))
    assert "656" in xfa.flash_mla_with_kvcache.__doc__ and "slot_mapping" in xfa.mla_cache_append_fp8.__doc__
