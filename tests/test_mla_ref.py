"""CPU: MLA decode — its semantics in float64, the pass rule of the GPU tests
against planted defects, the 2.9 surface, and the refusals of fmha_mla_decode that need no device.

* absorbed attention over the latent cache (what fmha_mla_decode computes: scores over the 576-wide
  row, values its first 512 features) equals explicit MLA, which decompresses K / V per head with
  W_UK / W_UV and shares one rotary key, to 1e-10 in float64;
* the per-sequence rule of tests/mla_util.py accepts a correct split decode (`emulate`) and rejects
  each of its four planted defects, already on the 517-key sequence;
* fmha_mla_decode is declared, exported and bound, the version is >= 2.9, and each refusal of the
  entry is reported through fmha_last_error (fake pointers: nothing is launched).
"""
import ctypes as C

import pytest
import torch

from oracle import attention_ref as orc
from tests import mla_util as mu
from xf_flash_attention_cutlass_amd import capi


# ------------------------------------------------------------------ semantics -------------
@pytest.mark.parametrize("causal", [False, True])
def test_absorbed_equals_explicit_mla(causal):
    g = torch.Generator().manual_seed(3)
    b, sq, sk, h, dn, dr, dc, dv = 2, 3, 37, 5, 24, 64, 512, 20
    f64 = dict(generator=g, dtype=torch.float64)
    c_kv = torch.randn(b, sk, dc, **f64)                    # compressed KV, shared by the heads
    k_rope = torch.randn(b, sk, dr, **f64)                  # rotary key, shared by the heads
    w_uk = torch.randn(h, dc, dn, **f64) / dc ** 0.5        # per-head up-projections
    w_uv = torch.randn(h, dc, dv, **f64) / dc ** 0.5
    q_nope = torch.randn(b, sq, h, dn, **f64)
    q_rope = torch.randn(b, sq, h, dr, **f64)
    scale = (dn + dr) ** -0.5                               # the model's scale, not 576^-1/2
    # explicit: K_h = [c W_UK_h, k_rope], V_h = c W_UV_h
    k = torch.cat([torch.einsum("bsc,hcn->bshn", c_kv, w_uk), k_rope[:, :, None].expand(b, sk, h, dr)], -1)
    v = torch.einsum("bsc,hcv->bshv", c_kv, w_uv)
    q = torch.cat([q_nope, q_rope], -1)
    want, _ = orc.attention_ref(q, k, v, causal=causal, upcast=False)       # default scale = `scale`
    want_lse = orc.attention_lse_ref(q, k, causal=causal)
    # absorbed: q_h -> [W_UK_h q_nope_h, q_rope_h] over the latent row [c, k_rope]; the value is the
    # row's first 512 features, W_UV_h applied to the output
    q_abs = torch.cat([torch.einsum("bthn,hcn->bthc", q_nope, w_uk), q_rope], -1)
    latent = torch.cat([c_kv, k_rope], -1)[:, :, None]                      # [b, sk, 1, 576]
    assert q_abs.shape[-1] == mu.D and latent.shape[-1] == mu.D
    q_scaled = q_abs * (scale * mu.D ** 0.5)                # the oracle's 576^-1/2 turned into `scale`
    o_lat, _ = orc.attention_ref(q_scaled, latent, latent[..., :mu.DV], causal=causal, upcast=False)
    got = torch.einsum("bthc,hcv->bthv", o_lat, w_uv)
    assert (got - want).abs().max().item() <= 1e-10
    got_lse = torch.logsumexp(torch.einsum("bthd,bsd->bhts", q_abs, latent[:, :, 0]).masked_fill(
        orc.local_mask(sq, sk, (-1, 0)) if causal else torch.zeros(sq, sk, dtype=torch.bool), float("-inf")) * scale, -1)
    assert (got_lse - want_lse.double()).abs().max().item() <= 1e-5         # (the oracle's LSE is fp32)


# ------------------------------------------------------------------ the pass rule ---------
RULE_CASES = [("h16_sq1", torch.bfloat16, 1), ("h16_sq1", torch.float16, 3),
              ("h8_sq3_causal", torch.bfloat16, 3), ("h8_sq3_causal", torch.float16, 1)]


def _problem(shape, dtype):
    h, sq, causal = mu.SHAPES[shape]
    c = mu.make_cache(mu.LENS, dtype, seed=11)
    q = mu.make_q(len(mu.LENS), sq, h, mu.D, dtype, 11)
    return c, q, causal, mu.oracle(c, q, causal)


_PROBLEMS = {}


def _cached(shape, dtype):
    if (shape, dtype) not in _PROBLEMS:
        _PROBLEMS[shape, dtype] = _problem(shape, dtype)
    return _PROBLEMS[shape, dtype]


@pytest.mark.parametrize("shape,dtype,splits", RULE_CASES)
def test_rule_accepts_correct_split_decode(shape, dtype, splits):
    c, q, causal, ora = _cached(shape, dtype)
    o, lse = mu.emulate(c, q, splits, causal)
    ok, figs = mu.judge_each(o, lse, ora)
    print([round(f["ratio"], 3) for f in figs])
    assert ok, figs
    assert max(f["ratio"] for f in figs) <= 0.6              # well inside: the rule has room for the kernel


@pytest.mark.parametrize("defect", mu.DEFECTS)
def test_rule_rejects_planted_defect(defect):
    shape = "h8_sq3_causal" if defect == "causal_off" else "h16_sq1"
    c, q, causal, ora = _cached(shape, torch.bfloat16)
    o, lse = mu.emulate(c, q, 3, causal, defect=defect)
    ok, figs = mu.judge_each(o, lse, ora)
    print(defect, [round(f["ratio"], 2) for f in figs])
    assert not ok
    assert not figs[0]["ok"] and figs[0]["ratio"] > 1.0       # already on the 517-key sequence


def test_batch_wide_rule_would_hide_long_sequences():
    """Why the rule is per sequence: the allowance of the whole batch comes from its short
    sequences (a softmax over 2 keys has weights of order 1, over 517 of order 1/517)."""
    c, q, causal, ora = _cached("h16_sq1", torch.bfloat16)
    per = [(ora.pt[i].float() - ora.ref[i].float()).abs().max().item() for i in range(len(mu.LENS))]
    assert max(per) > 3 * per[0]


# ------------------------------------------------------------------ surface ---------------
def test_surface_2_9():
    import xf_flash_attention_cutlass_amd as xfa
    from tests.test_abi import header_symbols
    assert "fmha_mla_decode" in header_symbols()
    assert "fmha_mla_decode" in capi.EXPORTED
    assert hasattr(capi.lib(), "fmha_mla_decode")
    ver = capi.lib().fmha_version().decode().split()[1]
    assert tuple(int(x) for x in ver.split(".")) >= (2, 9)
    assert callable(xfa.paged_attn.mla_decode)
    assert xfa.paged_attn.mla_decode is xfa.paged_attn._mla_decode
    assert "mla_decode" not in dir(xfa.paged_attn)
    assert "flash_mla_with_kvcache" in xfa.__all__ and callable(xfa.flash_mla_with_kvcache)


def _msgpack_uint(blob, j):
    t = blob[j]
    return t if t < 0x80 else int.from_bytes(blob[j + 1:j + 1 + {0xcc: 1, 0xcd: 2, 0xce: 4}[t]], "big")


def test_code_objects_have_no_scratch():
    """Every instance of the decode kernel and of the 512-wide combine is in the library's gfx950
    code object with private_segment_fixed_size 0 and no spilled register, read from the kernels'
    metadata (the msgpack note: .name, then .private_segment_fixed_size, ... .vgpr_spill_count)."""
    import re
    blob = open(capi.LIB_PATH, "rb").read()
    seen = {}
    for m in re.finditer(rb"\.name\xd9?.?(_ZN3xfa22fmha_mla_decode_kernel\w+|_ZN3xfa19fmha_combine_kernelILi512E\w+)", blob):
        key = b".private_segment_fixed_size"
        i = blob.find(key, m.end(), m.end() + 64)
        assert i > 0, m.group(1)
        k = blob.find(b".vgpr_spill_count", i, i + 400)
        assert k > 0, m.group(1)
        seen[m.group(1).decode()] = (_msgpack_uint(blob, i + len(key)), _msgpack_uint(blob, k + 17))
    print(seen)
    for tag in ("decode_kernelIDF16_E", "decode_kernelIDF16bE", "Li512EDF16_E", "Li512EDF16bE"):
        hits = [v for n, v in seen.items() if tag in n]
        assert hits and all(v == (0, 0) for v in hits), (tag, seen)


# ------------------------------------------------------------------ refusals --------------
FAKE = 0x10000        # 16-byte aligned, never dereferenced: every case fails before a launch


def _mla(q=FAKE, kv=FAKE + (1 << 30), o=FAKE + (1 << 29), lse=FAKE + (3 << 28), table=FAKE + (1 << 27),
         lens=FAKE + (1 << 26), bt_stride=64, sq=1, max_sk=1024, batch=2, heads=16, d=576, dv=512,
         page=16, strides="dense", window=(-1, -1), splits=0):
    L = capi.lib()
    if strides == "dense":
        strides = [sq * heads * d, heads * d, d, sq * heads * dv, heads * dv, dv]
    st = None if strides is None else (C.c_int64 * 6)(*strides)
    L.fmha_mla_decode(q, kv, o, lse, table, bt_stride, lens, sq, max_sk, batch, heads, d, dv, page, st,
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
    (dict(d=128, dv=128), "(576, 512) only"),
    (dict(dv=576), "(576, 512) only"),
    (dict(page=24), "multiple of 16"),
    (dict(page=0), "multiple of 16"),
    (dict(window=(-1, 5)), "(-1, -1) and (-1, 0)"),
    (dict(window=(64, 0)), "(-1, -1) and (-1, 0)"),
    (dict(window=(0, -1)), "(-1, -1) and (-1, 0)"),
    (dict(heads=0), "at least 1"),
    (dict(sq=0), "at least 1"),
    (dict(batch=-1), "non-negative"),
    (dict(splits=129), "at most 128"),
    (dict(max_sk=1025), "max_seqlen_k must lie in"),
    (dict(strides=_st(s2=580)), "multiples of 8"),
    (dict(strides=_st(s0=-576 * 16)), "non-negative"),
    (dict(strides=_st(s5=0)), "the output's positive"),
    (dict(strides=_st(s3=16 * 512 + 4)), "multiples of 8"),
    (dict(q=FAKE + 8), "16-byte aligned"),
    (dict(kv=FAKE + (1 << 30) + 2), "16-byte aligned"),
    (dict(o=FAKE + (1 << 29) + 4), "16-byte aligned"),
    (dict(lens=FAKE + (1 << 26) + 2), "4-byte aligned"),
    (dict(page=1864144, max_sk=64), "kv_cache page: one sequence spans"),
])
def test_mla_refusals(over, needle):
    st, msg, kern = _mla(**over)
    assert st != 0 and needle in msg, msg
    assert kern == "" and capi.lib().fmha_last_num_splits() == 0     # nothing was launched


def test_mla_accepts_empty_batch():
    """batch_size == 0 passes validation, launches nothing and succeeds (no pointer is read)."""
    st, msg, kern = _mla(batch=0)
    assert st == 0 and msg == "" and kern == ""


def test_mla_python_refusals():
    import xf_flash_attention_cutlass_amd as xfa
    q = torch.zeros(1, 1, 16, 576, dtype=torch.bfloat16)
    kv = torch.zeros(4, 16, 1, 576, dtype=torch.bfloat16)
    tab = torch.zeros(1, 4, dtype=torch.int32)
    lens = torch.zeros(1, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="fp16 or bf16"):
        xfa.flash_mla_with_kvcache(q.float(), kv, tab, lens)
    with pytest.raises(RuntimeError, match="must be on CUDA"):
        xfa.flash_mla_with_kvcache(q, kv, tab, lens)
    assert "softmax_lse" in xfa.flash_mla_with_kvcache.__doc__
