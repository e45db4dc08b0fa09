"""GPU: fmha_mla_sparse_fwd_fp8 (sparse MLA attention of new tokens over the fp8 latent cache,
DESIGN.md §3.10.4) against the CPU oracle over the dequantised operand (tests/mla_fp8_util.operand)
per position, under tests/mla_util.py's rule unchanged - a 64 x 16 cache of 656-byte rows viewed
flat whose every slot no query references is 0xFF bytes (NaN in every format of the row), into
NaN-filled outputs, three positions with an index set of their own and invalid values sprinkled in;
bit identity with the sparse fp8 decode at num_splits = 1; strided views, kv rows 672 bytes apart,
the four surfaces; refusals.  Every C-ABI call asserts the kernel and its grid."""
import ctypes as C

import pytest
import torch

import xf_flash_attention_cutlass_amd as xfa
from tests import mla_fp8_util as m8
from tests import mla_sparse_util as su
from tests import mla_util as mu
from xf_flash_attention_cutlass_amd import capi

pytestmark = pytest.mark.gpu

DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
SQ, SCALE, ROW = 3, mu.D ** -0.5, m8.ROW
_POOL, _PROBLEM = {}, {}


def problem(dt, heads, topk, specials=()):
    """(problem with b = 1, oracle, the oracle's largest scaled score [SQ, heads]), computed once."""
    key = (dt, heads, topk, specials)
    if key not in _PROBLEM:
        pool = _POOL[dt] if dt in _POOL else _POOL.setdefault(dt, su.make_pool("fp8", DTYPES[dt], 1024, 12))
        p = su.make_problem("fp8", DTYPES[dt], heads, SQ, topk, b=1, seed=topk, pool=pool)
        if specials:        # make_indices shapes (batch i, pos 0): three batches of one position, reshaped
            ind = su.make_indices(SQ, 1, topk, su.num_slots(p), topk, 0.1, specials).reshape(1, SQ, topk)
            ind[ind == 0] = 1   # slot 0, which every invalid lane loads, stays unreferenced: 0xFF bytes
            p = su.with_indices(p, ind)
        ml = torch.stack([(p.q[0, i].double() @ k[:, 0].double().T * SCALE).amax(-1) if len(k) else
                          torch.full((heads,), float("-inf"), dtype=torch.float64) for i, k in enumerate(p.kx)])
        _PROBLEM[key] = (p, su.oracle(p), ml.float())
    return _PROBLEM[key]


def nan(*shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device=mu.DEV)


def flat(p):
    return su.device_cache(p).view(-1, 1, ROW)


def run(p, kv, qd=None, o=None, want=(True, True)):
    """One fmha_mla_sparse_fwd_fp8 call through the C ABI into NaN-filled outputs: (o, lse, max_logits)."""
    L = capi.lib()
    _, sq, h, _ = p.q.shape
    qd = p.q[0].to(mu.DEV) if qd is None else qd
    ind = p.indices[0].to(mu.DEV)
    o = nan(sq, h, mu.DV, dtype=p.dtype) if o is None else o
    lse, ml = (nan(sq, h) if w else None for w in want)
    st = (C.c_int64 * 4)(qd.stride(0), qd.stride(1), o.stride(0), o.stride(1))
    L.fmha_mla_sparse_fwd_fp8(qd.data_ptr(), kv.data_ptr(), o.data_ptr(), capi.ptr(lse), capi.ptr(ml), ind.data_ptr(),
                              ind.stride(0), ind.shape[-1], sq, kv.shape[0], h, mu.D, mu.DV, kv.stride(0), st, SCALE,
                              p.dtype == torch.float16, capi.stream_handle())
    capi.check()
    torch.cuda.synchronize()
    kern = L.fmha_last_kernel().decode()
    assert kern.startswith("fmha_mla_sparse_fwd_fp8_kernel") and "grid=%dx1x1 block=256" % (sq * ((h + 63) // 64)) in kern, kern
    return o, lse, ml


def check(name, p, ora, ml_ref, o, lse, ml, report=None):
    su.assert_case(name, o.cpu()[None], lse.cpu().T[None], ora, report)
    ml, empty = ml.cpu(), torch.isinf(ml_ref)
    print(f"{name}: max_logits err {(ml - ml_ref)[~empty].abs().max().item():.3e}")
    assert torch.equal(ml[empty], ml_ref[empty]) and ((ml - ml_ref)[~empty].abs() <= 1e-3).all()


@pytest.mark.parametrize("topk", [1, 31, 32, 33, 65, 200])
@pytest.mark.parametrize("heads", [16, 40, 64, 128])
@pytest.mark.parametrize("dt", list(DTYPES))
def test_parity(dt, heads, topk, parity_report):
    """heads: one live wave, a partial tile with three live waves, a full workgroup, two workgroups a
    position; topk: 1, 2, 3 and 7 tiles - the prologue alone, both images, wraps, a ragged last tile."""
    p, ora, ml_ref = problem(dt, heads, topk)
    o, lse, ml = run(p, flat(p))
    check(f"mla-sparse-fwd-fp8-{dt}-h{heads}-topk{topk}", p, ora, ml_ref, o, lse, ml, parity_report)


@pytest.mark.parametrize("heads", [16, 40, 64, 128])
@pytest.mark.parametrize("dt", list(DTYPES))
def test_invalid_patterns(dt, heads, parity_report):
    """topk 200: position 0 holds a whole invalid tile, position 1 only invalid entries, position 2
    duplicates.  Slot 0 is 0xFF bytes, so an invalid lane's row dequantises to NaN before it is zeroed."""
    p, ora, ml_ref = problem(dt, heads, 200, ("tile_invalid", "all_invalid", "duplicates"))
    assert not su.valid_mask(p.indices[0, 0, 96:128].long(), su.num_slots(p)).any() and p.kx[1].shape[0] == 0
    kv = flat(p)
    assert not (p.indices == 0).any() and (kv[0] == 0xFF).all()
    o, lse, ml = run(p, kv)
    check(f"mla-sparse-fwd-fp8-{dt}-h{heads}-specials", p, ora, ml_ref, o, lse, ml, parity_report)
    assert (o[1] == 0).all() and (lse[1] == float("inf")).all() and (ml[1] == float("-inf")).all()


@pytest.mark.parametrize("topk", [33, 200])
@pytest.mark.parametrize("heads", [16, 128])
@pytest.mark.parametrize("dt", list(DTYPES))
def test_equals_the_sparse_fp8_decode_bit_for_bit(dt, heads, topk):
    """The same image bytes, tiles in the same order, the same arithmetic: out and lse equal the
    sparse fp8 decode kernel's at batch 1, seqlen_q = s_q and one split."""
    p, _, _ = problem(dt, heads, topk)
    kc = su.device_cache(p)
    o, lse, _ = run(p, kc.view(-1, 1, ROW))
    o0, l0 = xfa.flash_mla_with_kvcache(p.q.to(mu.DEV), kc, None, None, num_splits=1, indices=p.indices.to(mu.DEV))
    assert "sparse_fp8_kernel" in capi.lib().fmha_last_kernel().decode() and capi.lib().fmha_last_num_splits() == 1
    assert torch.equal(o, o0[0]) and torch.equal(lse, l0[0].T)


def test_strided_views_and_surfaces():
    """q and out as views inside NaN arenas (the out arena untouched outside out), kv rows 672 bytes
    apart with 0xFF between them; the C ABI, the pybind op and the wrapper (a uint8 and a
    float8_e4m3fn view) give the same bits; lse and max_logits may each be null."""
    (p, ora, ml_ref), h = problem("bf16", 40, 65), 40
    kv = torch.full((su.num_slots(p), 1, 672), 0xFF, dtype=torch.uint8, device=mu.DEV)[..., :ROW]
    kv.copy_(flat(p))
    qa = nan(SQ + 1, h + 2, mu.D + 64, dtype=p.dtype)
    qv = qa[1:, 1:h + 1, 64:]
    qv.copy_(p.q[0])
    oa = nan(SQ + 2, h + 1, mu.DV + 128, dtype=p.dtype)
    ov = oa[1:SQ + 1, :h, 64:64 + mu.DV]
    assert kv.stride(0) == 672 and not qv.is_contiguous() and not ov.is_contiguous()
    o, lse, ml = run(p, kv, qd=qv, o=ov)
    check("mla-sparse-fwd-fp8-strided", p, ora, ml_ref, ov, lse, ml)
    inside = torch.zeros_like(oa, dtype=torch.bool)
    inside[1:SQ + 1, :h, 64:64 + mu.DV] = True
    ind = p.indices[0].to(mu.DEV)
    o1, ml1, lse1 = xfa.paged_attn.mla_sparse_fwd_fp8(qv, kv, ind, SCALE, 512, None)
    o2, ml2, lse2 = xfa.flash_mla_sparse_fwd(qv, kv, ind[:, None])
    out = nan(SQ, h, mu.DV, dtype=p.dtype)
    o3, ml3, lse3 = xfa.flash_mla_sparse_fwd(p.q[0].to(mu.DEV), kv.view(torch.float8_e4m3fn), ind, SCALE, out=out)
    assert o3 is out and torch.isnan(oa[~inside]).all()
    for a, b, c in ((o1, ml1, lse1), (o2, ml2, lse2), (o3, ml3, lse3)):
        assert torch.equal(a, ov) and torch.equal(b, ml) and torch.equal(c, lse)
    for want in ((False, True), (True, False), (False, False)):
        o4, l4, m4 = run(p, kv, want=want)
        assert torch.equal(o4, ov) and (l4 is None or torch.equal(l4, lse)) and (m4 is None or torch.equal(m4, ml))


@pytest.mark.parametrize("case", ["u8_d576", "kv_heads2", "stride664", "int64_indices", "topk0", "dv576"])
def test_refused_calls_leave_outputs_untouched(case):
    p, _, _ = problem("bf16", 16, 33)
    q, kv, ind = p.q[0].to(mu.DEV), flat(p), p.indices[0].to(mu.DEV)
    out = nan(SQ, 16, mu.DV, dtype=p.dtype)
    args = dict(q=q, kv=kv, indices=ind, d_v=512)
    args.update({"u8_d576": dict(kv=kv[..., :mu.D]), "kv_heads2": dict(kv=kv.view(-1, 2, ROW)),
                 "stride664": dict(kv=torch.zeros(len(kv), 1, 664, dtype=torch.uint8, device=mu.DEV)[..., :ROW]),
                 "int64_indices": dict(indices=ind.long()), "topk0": dict(indices=ind[:, :0]),
                 "dv576": dict(d_v=576)}[case])
    with pytest.raises(RuntimeError):
        xfa.flash_mla_sparse_fwd(args["q"], args["kv"], args["indices"], SCALE, args["d_v"], out=out)
    torch.cuda.synchronize()
    assert torch.isnan(out).all()
    xfa.flash_mla_sparse_fwd(q, kv, ind, SCALE, out=out)
    assert not torch.isnan(out).any()
