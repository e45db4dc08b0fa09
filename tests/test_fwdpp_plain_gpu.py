"""GPU: the plain body of the 32x32x16 ping-pong forward (gen_fwdpp.py PLAIN, fwdpp_plain_item_*;
knob fwd_plain) against the full body.

The plain body is the full one generated without the score features and the left window, with two
reductions of its own (no per-step key limit, tile 0's max without the key test where the whole
tile is visible): the same arithmetic in the same order.  Every case runs the same launch under
fwd_plain = 1 and 0, asserts from fmha_last_kernel() which body ran (` body=plain` / ` body=full`),
and asserts O and LSE equal bit for bit; one case per group is also held to the oracle by the
suite's rule (test.py:975, orc.parity_ok) and the LSE to the fp32 log-sum-exp.  All D = 128.
"""
import pytest
import torch

from oracle import attention_ref as orc
from tests import softmax_stress_util as su

pytestmark = pytest.mark.gpu
DEV = "cuda"
SC = 128 ** -0.5


def _L():
    from xf_flash_attention_cutlass_amd import capi
    return capi.lib()


def _launch(fn, w4, plain, slack=None):
    """fn() under fwd_w4 = w4, fwd_plain = plain (and fwd_slack): the kernel id after the launch"""
    from xf_flash_attention_cutlass_amd import capi
    with su._option("fwd_w4", w4), su._option("fwd_plain", plain), \
            su._option("fwd_slack", 8 if slack is None else slack):
        fn()
        capi.check()
        torch.cuda.synchronize()
        return _L().fmha_last_kernel().decode()


def _body(kern):
    assert kern.startswith(("fmha_fwdpp_kernel ", "fmha_fwdpp_paged_kernel ")), kern
    return kern.split(" body=")[1].split()[0]


def _dense(q, k, v, window, w4, plain, slack=None, slopes=None, softcap=0.0):
    """fmha_fwd, one split: (O, LSE, kernel id)"""
    from xf_flash_attention_cutlass_amd import capi
    b, sq, h, _ = q.shape
    sk, hk = k.shape[1], k.shape[2]
    qd, kd, vd = (x.to(DEV).contiguous() for x in (q, k, v))
    o = torch.full_like(qd, float("nan"))
    lse = torch.full((b, h, sq), float("nan"), device=DEV, dtype=torch.float32)
    sl = slopes.to(DEV).contiguous() if slopes is not None else None
    kern = _launch(lambda: _L().fmha_fwd(qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), o.data_ptr(), capi.ptr(sl),
                                         sq, sk, b, h, hk, 128, 0.0, capi.stream_handle(), None, SC, None,
                                         lse.data_ptr(), window[0], window[1], softcap, False,
                                         q.dtype == torch.float16, 1), w4, plain, slack)
    return o.cpu(), lse.cpu(), kern


def _pair(run):
    """run(plain) -> (O, LSE, kernel id): both bodies ran and agree bit for bit; the plain one's"""
    o1, l1, k1 = run(1)
    o0, l0, k0 = run(0)
    assert _body(k1) == "plain" and _body(k0) == "full", (k1, k0)
    assert k1.replace(" body=plain", "") == k0.replace(" body=full", ""), (k1, k0)   # same schedule
    assert torch.equal(o1, o0), "O differs between the bodies"
    assert torch.equal(l1, l0), "LSE differs between the bodies"
    return o1, l1


def _oracle(o, lse, q, k, v, window):
    w = (-1, 0) if window == (-1, 0) else window
    causal = window == (-1, 0)
    kw = dict(causal=True) if causal else dict(window_size=w)
    ref, _ = orc.attention_ref(q, k, v, **kw)
    pt, _ = orc.attention_ref(q, k, v, upcast=False, reorder_ops=True, **kw)
    ok, err, bound = orc.parity_ok(o.float(), ref, pt, 2.0, 1e-5)
    print(f"max|out-ref| = {err:.3g}, bound {bound:.3g}")
    assert ok, f"max|out-ref| = {err:.3g} > {bound:.3g}"
    lref = orc.attention_lse_ref(q, k, **kw)
    fin = torch.isfinite(lref)
    assert torch.equal(torch.isinf(lse) & (lse > 0), ~fin), "the +inf pattern of the LSE differs"
    assert (lse[fin] - lref[fin]).abs().max().item() < 1e-3
    return fin


def _qkv(b, h, hk, sq, sk, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(b, sq, h, 128, generator=g).to(dtype), torch.randn(b, sk, hk, 128, generator=g).to(dtype),
            torch.randn(b, sk, hk, 128, generator=g).to(dtype))


BF, FP = torch.bfloat16, torch.float16
DENSE = [
    # id, b, h, hk, sq, sk, window (wl, wr), fwd_w4, dtype, oracle
    # two row blocks (600 packed rows), a ragged last tile, masked tiles at several wave positions
    ("causal-300", 2, 4, 2, 300, 300, (-1, 0), 4, BF, True),
    ("causal-300-f16", 2, 4, 2, 300, 300, (-1, 0), 4, FP, False),
    # offset diagonal: the first tiles wholly visible (the unmasked first max)
    ("causal-300x900", 2, 4, 2, 300, 900, (-1, 0), 4, BF, True),
    ("causal-300x900-f16", 2, 4, 2, 300, 900, (-1, 0), 4, FP, False),
    # rows and whole waves without a visible key (tw < 0): O = 0, LSE = +inf
    ("causal-600x200", 2, 4, 2, 600, 200, (-1, 0), 4, BF, True),
    # non-causal: right window only; no window (fwd_w4 = 2 forces the 32x32x16 body)
    ("right200-1024", 1, 4, 4, 1024, 1024, (-1, 200), 2, BF, True),
    ("right200-1024-f16", 1, 4, 4, 1024, 1024, (-1, 200), 2, FP, False),
    ("full-513x1025", 1, 8, 2, 513, 1025, (-1, -1), 2, BF, True),
    ("full-513x1025-f16", 1, 8, 2, 513, 1025, (-1, -1), 2, FP, False),
]


@pytest.mark.parametrize("name,b,h,hk,sq,sk,window,w4,dtype,oracle", DENSE, ids=[c[0] for c in DENSE])
def test_plain_body_equals_full_dense(name, b, h, hk, sq, sk, window, w4, dtype, oracle):
    q, k, v = _qkv(b, h, hk, sq, sk, dtype, sq + sk)
    o, lse = _pair(lambda plain: _dense(q, k, v, window, w4, plain))
    if oracle:
        fin = _oracle(o, lse, q, k, v, window)
        if sq > sk and window == (-1, 0):      # rows before the diagonal's start see no key
            assert not fin[:, :, :sq - sk].any() and fin[:, :, sq - sk:].all()
            assert (o[:, :sq - sk] == 0).all()


def _varlen(q, k, v, cu_q, cu_k, used, causal, dtype, plain):
    from xf_flash_attention_cutlass_amd import capi
    h, hk = q.shape[1], k.shape[1]
    nb = cu_q.numel() - 1
    mq, mk = int((cu_q[1:] - cu_q[:-1]).max()), int((cu_k[1:] - cu_k[:-1]).max())
    qd, kd, vd, cq, ck, us = (x.to(DEV).contiguous() for x in (q, k, v, cu_q, cu_k, used))
    o = torch.full_like(qd, float("nan"))
    lse = torch.full((h, q.shape[0]), float("nan"), device=DEV, dtype=torch.float32)
    kern = _launch(lambda: _L().fmha_varlen_fwd_ex(
        qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), o.data_ptr(), lse.data_ptr(), cq.data_ptr(), ck.data_ptr(),
        us.data_ptr(), None, 0, 0, None, 0, mq, mk, q.shape[0], nb, h, hk, 128, SC, -1, 0 if causal else -1, 0.0,
        dtype == FP, capi.stream_handle(), 0.0, None), 4 if causal else 2, plain)
    return o.cpu(), lse.cpu(), kern


@pytest.mark.parametrize("causal,dtype", [(True, BF), (False, BF), (True, FP)])
def test_plain_body_equals_full_varlen(causal, dtype):
    """Packed sequences of lengths 1, 0, 65, 300, 257 (q and k), the 300-key one used up to key 211
    only (seqused_k shorter than its cu_seqlens_k span); the bf16 launches per sequence against
    the oracle"""
    lens = [1, 0, 65, 300, 257]
    used = torch.tensor([1, 0, 65, 211, 257], dtype=torch.int32)
    cu = torch.tensor([0] + list(torch.tensor(lens).cumsum(0)), dtype=torch.int32)
    g = torch.Generator().manual_seed(77)
    tot, h, hk = int(cu[-1]), 4, 2
    q = torch.randn(tot, h, 128, generator=g).to(dtype)
    k, v = (torch.randn(tot, hk, 128, generator=g).to(dtype) for _ in range(2))
    o, lse = _pair(lambda plain: _varlen(q, k, v, cu, cu, used, causal, dtype, plain))
    if dtype != BF:
        return
    for i, n in enumerate(lens):
        a, e, u = int(cu[i]), int(cu[i + 1]), int(used[i])
        if n == 0:
            continue
        _oracle(o[a:e][None], lse[:, a:e][None], q[a:e][None], k[a:a + u][None], v[a:a + u][None],
                (-1, 0) if causal else (-1, -1))


@pytest.mark.parametrize("slack", [0, 8])
def test_plain_body_equals_full_rare_path(slack):
    """Keys growing along the sequence (softmax_stress_util `growing40`): rows' running maxima jump
    by more than 2^fwd_slack at tiles after tile 0, so V phases of both kinds (unmasked tiles under
    the offset diagonal, masked ones on it) take the rare path (redo_block: its FEATURES branch with
    SHIFT = 0 in the full body, its plain branch — with the key limit formed there — in the plain one)"""
    q, k, v = _qkv(1, 4, 2, 300, 900, BF, 5)
    q, k = su.apply_pattern("growing40", q, k)
    big, n = su.tile_jumps(q, k, su.mask_of((900, 0), 300, 900), slack=float(slack))
    assert n > 0 and big > 8, (big, n)
    o, lse = _pair(lambda plain: _dense(q, k, v, (-1, 0), 4, plain, slack=slack))
    if slack == 8:
        _oracle(o, lse, q, k, v, (-1, 0))


def test_launches_the_plain_body_must_not_take():
    """ALiBi, softcap and a left window keep the full body, a paged cache the paged one, under
    fwd_plain = 1; and the plain causal launch beside them takes the plain one"""
    from xf_flash_attention_cutlass_amd import capi
    q, k, v = _qkv(1, 4, 4, 300, 300, BF, 3)
    slopes = torch.linspace(0.05, 0.5, 4).view(1, 4)
    assert _body(_dense(q, k, v, (-1, 0), 4, 1)[2]) == "plain"
    assert _body(_dense(q, k, v, (-1, 0), 4, 1, slopes=slopes)[2]) == "full"
    assert _body(_dense(q, k, v, (-1, 0), 4, 1, softcap=30.0)[2]) == "full"
    assert _body(_dense(q, k, v, (100, 0), 4, 1)[2]) == "full"
    assert _body(_dense(q, k, v, (100, -1), 2, 1)[2]) == "full"
    # a paged cache of 16-key pages, prefill of 300 rows
    page, nbp = 16, 19
    kc = torch.zeros(nbp, page, 4, 128, dtype=BF)
    vc = torch.zeros(nbp, page, 4, 128, dtype=BF)
    kc.view(-1, 4, 128)[:300], vc.view(-1, 4, 128)[:300] = k[0], v[0]
    table = torch.arange(nbp, dtype=torch.int32).view(1, nbp)
    qd, kd, vd, td = (x.to(DEV).contiguous() for x in (q, kc, vc, table))
    sl = torch.tensor([300], dtype=torch.int32, device=DEV)
    o = torch.empty_like(qd)
    lse = torch.empty(1, 4, 300, device=DEV, dtype=torch.float32)
    kern = _launch(lambda: _L().fmha_page_kvcache_fwd_ex(
        qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), o.data_ptr(), lse.data_ptr(), td.data_ptr(), nbp,
        sl.data_ptr(), 300, 300, 1, 4, 4, 128, page, SC, -1, 0, 0.0, None, 0, 1, 0, 1.0, 1.0, None, False,
        capi.stream_handle()), 4, 1)
    assert kern.startswith("fmha_fwdpp_paged_kernel ") and _body(kern) == "paged", kern
    # ... and computes what the plain body computes over the same rows
    od, ld, _ = _dense(q, k, v, (-1, 0), 4, 1)
    assert torch.equal(o.cpu(), od) and torch.equal(lse.cpu(), ld)
