"""GPU: the MLA prefill forward (fmha_fwd_mla_kernel: head size 192 for Q K^T, 128 for V; DESIGN.md
§3.11) against the oracle, per sequence, under the project's forward rule (tests/fwd_mla_util.py).
Every output starts NaN-filled and every launch asserts the kernel id.

The sizes are the smallest that reach every path of a 64-key-tile, 256-row-item kernel: q lengths
[300, 113, 1, 31] over k lengths [333, 203, 147, 0] (6 key tiles = the full ring, a remainder and a
ragged last tile; sk > sq; sk >> sq = 1; an empty sequence) and the k lengths reversed against q (sk
< sq under causal: rows that see no key); heads (6, 2) (G = 3: a 32-row wave tile straddles
positions, and 300 x 3 = 900 rows are 4 items, the last partial) and (3, 3).
"""
import ctypes as C

import pytest
import torch

from tests import fwd_mla_util as mu
from tests import softmax_stress_util as su

pytestmark = pytest.mark.gpu
DEV = mu.DEV
DTS = list(mu.DTYPES)


def _dev(*xs):
    return tuple(x.to(DEV) for x in xs)


# ------------------------------------------------------------------ varlen ---------------------
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("h,hk", [(6, 2), (3, 3)], ids=["h6_hk2", "h3_hk3"])
@pytest.mark.parametrize("lens_k,causal", [(mu.LENS_K, True), (mu.LENS_K, False), (mu.LENS_K_REV, True)],
                         ids=["causal", "full", "causal_rev"])
def test_varlen(dt, h, hk, lens_k, causal, parity_report):
    q, k, v = mu.make_packed(mu.LENS_Q, lens_k, h, hk, mu.DTYPES[dt], seed=h)
    window = mu.window_of(causal, (-1, -1))
    seqs = mu.oracle(q, k, v, mu.LENS_Q, lens_k, window)
    o, lse, _ = mu.run_varlen(*_dev(q, k, v), mu.LENS_Q, lens_k, h, hk, window)
    mu.assert_case(f"fwd_mla varlen {dt} h{h}/{hk} k{lens_k[0]} causal={causal}", o.cpu(), lse.cpu(), seqs,
                   mu.LENS_Q, parity_report)


@pytest.mark.parametrize("dt", DTS)
def test_varlen_seqused_k(dt, parity_report):
    h, hk = 6, 2
    used = [200, 203, 64, 0]                   # shorter than cu_seqlens_k; a whole number of tiles once
    q, k, v = mu.make_packed(mu.LENS_Q, mu.LENS_K, h, hk, mu.DTYPES[dt], seed=3)
    seqs = mu.oracle(q, k, v, mu.LENS_Q, mu.LENS_K, (-1, 0), used_k=used)
    o, lse, _ = mu.run_varlen(*_dev(q, k, v), mu.LENS_Q, mu.LENS_K, h, hk, (-1, 0), used_k=used)
    mu.assert_case(f"fwd_mla varlen seqused_k {dt}", o.cpu(), lse.cpu(), seqs, mu.LENS_Q, parity_report)


# every tile count at which the key loop takes another path: 1 tile (no pipeline), 2 (no third tile
# in the prologue), 3 and 4 (one and two steps issue nothing), 5 (the K ring wraps), 8, and 13 (K
# buffer 12 % 4 and V buffer 12 % 3 meet again: the whole period of the two rings)
LENS_K_TILES = [64, 128, 129, 256, 320, 449, 832]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
def test_varlen_every_tile_count(dt, causal, parity_report):
    h, hk = 4, 2
    lens_q = [40] * len(LENS_K_TILES)
    q, k, v = mu.make_packed(lens_q, LENS_K_TILES, h, hk, mu.DTYPES[dt], seed=31)
    window = mu.window_of(causal, (-1, -1))
    seqs = mu.oracle(q, k, v, lens_q, LENS_K_TILES, window)
    o, lse, _ = mu.run_varlen(*_dev(q, k, v), lens_q, LENS_K_TILES, h, hk, window)
    mu.assert_case(f"fwd_mla varlen tile counts {dt} causal={causal}", o.cpu(), lse.cpu(), seqs, lens_q, parity_report)


@pytest.mark.parametrize("window", [(400, 0), (400, 40)], ids=["w400_0", "w400_40"])
def test_dense_wide_left_window(window, parity_report):
    """G = 1, so an item is 256 positions and its left limits span 256 keys: the later items run
    four or five tiles in the per-wave masked loop, then two tiles every row sees in full and the
    edge tiles through the pipeline; the first item has no left edge at all."""
    b, sq, sk, h, hk = 1, 600, 700, 2, 2
    q, k, v = mu.make_packed([sq], [sk], h, hk, torch.bfloat16, seed=33)
    seqs = mu.oracle(q, k, v, [sq], [sk], window)
    qd, kd, vd = _dev(q.view(b, sq, h, -1), k.view(b, sk, hk, -1), v.view(b, sk, hk, -1))
    o, lse, _ = mu.run_dense(qd, kd, vd, window)
    o, lse = mu.dense_as_packed(o.cpu(), lse.cpu())
    mu.assert_case(f"fwd_mla dense left window {window}", o, lse, seqs, [sq], parity_report)


# ------------------------------------------------------------------ dense ----------------------
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("window", [(-1, 0), (37, 0), (-1, 20)], ids=["causal", "w37_0", "w-1_20"])
def test_dense(dt, window, parity_report):
    b, sq, sk, h, hk = 2, 257, 333, 6, 2
    q, k, v = mu.make_packed([sq] * b, [sk] * b, h, hk, mu.DTYPES[dt], seed=11)
    seqs = mu.oracle(q, k, v, [sq] * b, [sk] * b, window)
    qd, kd, vd = _dev(q.view(b, sq, h, -1), k.view(b, sk, hk, -1), v.view(b, sk, hk, -1))
    o, lse, _ = mu.run_dense(qd, kd, vd, window)
    o, lse = mu.dense_as_packed(o.cpu(), lse.cpu())
    mu.assert_case(f"fwd_mla dense {dt} window={window}", o, lse, seqs, [sq] * b, parity_report)


# ------------------------------------------------------------------ ownership ------------------
def _fill_value(fill, dtype):
    return {"zero": 0.0, "nan": float("nan"), "max": torch.finfo(dtype).max}[fill]


def _arena_case(dt, fill, causal):
    """q, k, v and o as strided views inside arenas filled with `fill`: a spare head after the real
    ones, FRONT rows before and BACK rows after, K's row pitch (hk + 1) x 192 and V's (hk + 1) x
    128 + 64; the LSE inside a longer fp32 arena."""
    dtype = mu.DTYPES[dt]
    h, hk, front, back = 6, 2, 5, 70
    q, k, v = mu.make_packed(mu.LENS_Q, mu.LENS_K, h, hk, dtype, seed=21)
    tq, tk = q.shape[0], k.shape[0]
    val = _fill_value(fill, dtype)
    aq = torch.full((front + tq + back, h + 1, mu.DQK), val, dtype=dtype, device=DEV)
    ak = torch.full((front + tk + back, hk + 1, mu.DQK), val, dtype=dtype, device=DEV)
    av = torch.full((front + tk + back, (hk + 1) * mu.DV + 64), val, dtype=dtype, device=DEV)
    ao = torch.full((front + tq + back, h + 1, mu.DV), val, dtype=dtype, device=DEV)
    al = torch.full((8 + h * tq + 8,), val if fill != "max" else torch.finfo(torch.float32).max,
                    dtype=torch.float32, device=DEV)
    qv, kv_, ov = aq[front:front + tq, :h], ak[front:front + tk, :hk], ao[front:front + tq, :h]
    vv = av[front:front + tk, :hk * mu.DV].view(tk, hk, mu.DV)
    lv = al[8:8 + h * tq].view(h, tq)
    qv.copy_(q.to(DEV)); kv_.copy_(k.to(DEV)); vv.copy_(v.to(DEV))
    assert kv_.stride(0) != vv.stride(0) and vv.stride(0) == (hk + 1) * mu.DV + 64
    before = (ao.clone(), al.clone(), aq.clone(), ak.clone(), av.clone())
    window = mu.window_of(causal, (-1, -1))
    mu.run_varlen(qv, kv_, vv, mu.LENS_Q, mu.LENS_K, h, hk, window, o=ov, lse=lv)
    # nothing outside o's and LSE's owned elements changed (bit patterns: NaN fills compare equal)
    own_o = torch.zeros_like(ao, dtype=torch.bool)
    own_o[front:front + tq, :h] = True
    own_l = torch.zeros_like(al, dtype=torch.bool)
    own_l[8:8 + h * tq] = True
    bits = lambda x: x.view(torch.int16 if x.element_size() == 2 else torch.int32)  # noqa: E731
    assert torch.equal(bits(ao)[~own_o], bits(before[0])[~own_o]), "o arena changed outside o"
    assert torch.equal(bits(al)[~own_l], bits(before[1])[~own_l]), "lse arena changed outside lse"
    for got, was, name in ((aq, before[2], "q"), (ak, before[3], "k"), (av, before[4], "v")):
        assert torch.equal(bits(got), bits(was)), f"{name} arena was written"
    return (q, k, v), ov.contiguous().cpu(), lv.contiguous().cpu()


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
def test_ownership_in_poisoned_arenas(dt, causal, parity_report):
    res = {fill: _arena_case(dt, fill, causal) for fill in ("zero", "nan", "max")}
    (q, k, v), o0, l0 = res["zero"]
    for fill in ("nan", "max"):
        assert torch.equal(res[fill][1].view(torch.int16), o0.view(torch.int16)), f"o differs under fill {fill}"
        assert torch.equal(res[fill][2].view(torch.int32), l0.view(torch.int32)), f"lse differs under fill {fill}"
    seqs = mu.oracle(q, k, v, mu.LENS_Q, mu.LENS_K, mu.window_of(causal, (-1, -1)))
    mu.assert_case(f"fwd_mla arenas {dt} causal={causal}", o0, l0, seqs, mu.LENS_Q, parity_report)


# ------------------------------------------------------------------ reproducibility, graph -----
@pytest.mark.parametrize("dt", DTS)
def test_two_calls_and_a_graph_replay_are_bit_equal(dt):
    h, hk = 6, 2
    q, k, v = _dev(*mu.make_packed(mu.LENS_Q, mu.LENS_K, h, hk, mu.DTYPES[dt], seed=5))
    o1, l1, _ = mu.run_varlen(q, k, v, mu.LENS_Q, mu.LENS_K, h, hk, (-1, 0))
    o2, l2, _ = mu.run_varlen(q, k, v, mu.LENS_Q, mu.LENS_K, h, hk, (-1, 0))
    assert torch.equal(o1.view(torch.int16), o2.view(torch.int16)) and torch.equal(l1.view(torch.int32), l2.view(torch.int32))
    o = torch.full_like(o1, float("nan"))
    lse = torch.full_like(l1, float("nan"))
    cus = (mu.cu(mu.LENS_Q).to(DEV), mu.cu(mu.LENS_K).to(DEV))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):              # warm-up on the capture stream: its item-queue counters exist
        mu.run_varlen(q, k, v, mu.LENS_Q, mu.LENS_K, h, hk, (-1, 0), o=o, lse=lse, sync=False, cus=cus)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    o.fill_(float("nan")); lse.fill_(float("nan"))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        mu.run_varlen(q, k, v, mu.LENS_Q, mu.LENS_K, h, hk, (-1, 0), o=o, lse=lse, sync=False, cus=cus)
    torch.cuda.synchronize()
    assert torch.isnan(o).all(), "the capture itself must not run the kernel"
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(o.view(torch.int16), o1.view(torch.int16)) and torch.equal(lse.view(torch.int32), l1.view(torch.int32))


# ------------------------------------------------------------------ surface --------------------
@pytest.mark.parametrize("dt", DTS)
def test_surface_c_abi_pybind_and_wrappers_agree(dt):
    """The test that fails without the feature: before it, every one of these calls is refused with
    a shape error."""
    import xf_flash_attention_cutlass_amd as xfa
    h, hk = 6, 2
    q, k, v = _dev(*mu.make_packed(mu.LENS_Q, mu.LENS_K, h, hk, mu.DTYPES[dt], seed=9))
    cq, ck = mu.cu(mu.LENS_Q).to(DEV), mu.cu(mu.LENS_K).to(DEV)
    mq, mk = max(mu.LENS_Q), max(mu.LENS_K)
    o_c, l_c, _ = mu.run_varlen(q, k, v, mu.LENS_Q, mu.LENS_K, h, hk, (-1, 0))
    o_p, l_p = xfa.paged_attn.varlen_fwd_mla(q, k, v, None, cq, ck, None, mq, mk, mu.DQK ** -0.5, True, -1, -1)
    o_w, l_w, none = xfa.flash_attn_varlen_func(q, k, v, cq, ck, mq, mk, causal=True, return_attn_probs=True)
    o_w2 = xfa.flash_attn_varlen_func(q, k, v, cq, ck, mq, mk, causal=True)
    assert none is None and o_w.shape == (sum(mu.LENS_Q), h, mu.DV) and l_w.shape == (h, sum(mu.LENS_Q))
    for o, l in ((o_p, l_p), (o_w, l_w)):
        assert torch.equal(o.view(torch.int16), o_c.view(torch.int16)) and torch.equal(l.view(torch.int32), l_c.view(torch.int32))
    assert torch.equal(o_w2.view(torch.int16), o_c.view(torch.int16))
    assert not o_w.requires_grad
    # dense: the first sequence alone as a batch of one
    qd, kd, vd = q[None, :300], k[None, :333], v[None, :333]
    o_c, l_c, _ = mu.run_dense(qd, kd, vd, (-1, 0))
    o_p, l_p = xfa.paged_attn.fwd_mla(qd, kd, vd, None, mu.DQK ** -0.5, True, -1, -1)
    o_w, l_w, none = xfa.flash_attn_func(qd, kd, vd, causal=True, return_attn_probs=True)
    assert none is None and o_w.shape == (1, 300, h, mu.DV) and l_w.shape == (1, h, 300)
    for o, l in ((o_p, l_p), (o_w, l_w)):
        assert torch.equal(o.view(torch.int16), o_c.view(torch.int16)) and torch.equal(l.view(torch.int32), l_c.view(torch.int32))
    # ... and the packed call's first sequence is the dense call
    assert torch.equal(o_c[0].view(torch.int16), o_w2[:300].view(torch.int16))


@pytest.mark.parametrize("dt", DTS)
def test_non_default_scale(dt, parity_report):
    import xf_flash_attention_cutlass_amd as xfa
    h, hk = 6, 2
    q, k, v = mu.make_packed(mu.LENS_Q, mu.LENS_K, h, hk, mu.DTYPES[dt], seed=13)
    seqs = mu.oracle(q, k, v, mu.LENS_Q, mu.LENS_K, (-1, 0), q_mul=0.5)     # half the default scale
    scale = 0.5 * mu.DQK ** -0.5
    qd, kd, vd = _dev(q, k, v)
    o, lse, _ = mu.run_varlen(qd, kd, vd, mu.LENS_Q, mu.LENS_K, h, hk, (-1, 0), scale=scale)
    mu.assert_case(f"fwd_mla varlen scale/2 {dt}", o.cpu(), lse.cpu(), seqs, mu.LENS_Q, parity_report)
    cq, ck = mu.cu(mu.LENS_Q).to(DEV), mu.cu(mu.LENS_K).to(DEV)
    o_w = xfa.flash_attn_varlen_func(qd, kd, vd, cq, ck, max(mu.LENS_Q), max(mu.LENS_K), softmax_scale=scale, causal=True)
    assert torch.equal(o_w.view(torch.int16), o.view(torch.int16))


def test_refusals_leave_the_outputs_untouched():
    """Every refusal of the C entries that needs real tensors, and the ops' own, with o and LSE still
    NaN (the refusals on fake pointers are tests/test_fwd_mla_ref.py's)."""
    import xf_flash_attention_cutlass_amd as xfa
    from xf_flash_attention_cutlass_amd import capi
    L = capi.lib()
    h, hk, dtype = 6, 2, torch.bfloat16
    q, k, v = _dev(*mu.make_packed(mu.LENS_Q, mu.LENS_K, h, hk, dtype))
    tq = q.shape[0]
    o = torch.full((tq, h, mu.DV), float("nan"), dtype=dtype, device=DEV)
    lse = torch.full((h, tq), float("nan"), dtype=torch.float32, device=DEV)
    cq, ck = mu.cu(mu.LENS_Q).to(DEV), mu.cu(mu.LENS_K).to(DEV)
    st = [q.stride(0), q.stride(1), k.stride(0), k.stride(1), v.stride(0), v.stride(1), o.stride(0), o.stride(1)]

    def call(dqk=mu.DQK, dv=mu.DV, heads_k=hk, qp=None, stv=None, max_k=333):
        L.fmha_varlen_fwd_mla(q.data_ptr() if qp is None else qp, k.data_ptr(), v.data_ptr(), o.data_ptr(),
                              lse.data_ptr(), cq.data_ptr(), ck.data_ptr(), None, 300, max_k, tq, 4, h, heads_k,
                              dqk, dv, (C.c_int64 * 8)(*(stv or st)), mu.DQK ** -0.5, -1, 0, False,
                              capi.stream_handle())
        return L.fmha_last_status(), L.fmha_last_error().decode()

    bad_v = list(st); bad_v[4] = 120
    bad_k = list(st); bad_k[2] = 388
    for kw, needle in ((dict(dqk=128, dv=128), "(192, 128) only"), (dict(dqk=192, dv=192), "(192, 128) only"),
                       (dict(heads_k=4), "must divide"), (dict(qp=q.data_ptr() + 2), "16-byte aligned"),
                       (dict(stv=bad_v), "at least its head size"), (dict(stv=bad_k), "multiples of 8"),
                       (dict(max_k=0), "nothing to attend to")):
        status, msg = call(**kw)
        assert status != 0 and needle in msg, (kw, msg)
        assert L.fmha_last_kernel() == b""
    # the ops: no padded copies - a misaligned or non-unit-stride input is refused, not copied
    mq, mk = 300, 333
    q_odd = torch.zeros(tq * h * mu.DQK + 8, dtype=dtype, device=DEV)[1:1 + tq * h * mu.DQK].view(tq, h, mu.DQK)
    q_t = torch.zeros(tq, mu.DQK, h, dtype=dtype, device=DEV).transpose(1, 2)
    for args, needle in (((q_odd, k, v), "16-byte aligned"), ((q_t, k, v), "contiguous last dimension"),
                         ((q, k, v.float()), "dtype of q"), ((q, k[:, :1].expand(-1, 4, -1), v), "same number of heads"),
                         ((q[:, :5], k, v), "must divide")):
        with pytest.raises(RuntimeError, match=needle):
            xfa.paged_attn.varlen_fwd_mla(*args, o, cq, ck, None, mq, mk, mu.DQK ** -0.5, True, -1, -1)
    with pytest.raises(RuntimeError, match="out must have shape"):
        xfa.paged_attn.varlen_fwd_mla(q, k, v, o[:, :, :64], cq, ck, None, mq, mk, mu.DQK ** -0.5, True, -1, -1)
    with pytest.raises(RuntimeError, match="seqused_k"):
        xfa.paged_attn.varlen_fwd_mla(q, k, v, o, cq, ck, ck, mq, mk, mu.DQK ** -0.5, True, -1, -1)
    # the wrappers (the named arguments are tests/test_fwd_mla_ref.py's; here on the device)
    with pytest.raises(NotImplementedError, match="dropout_p"):
        xfa.flash_attn_varlen_func(q, k, v, cq, ck, mq, mk, dropout_p=0.1)
    with pytest.raises(NotImplementedError, match="q.requires_grad"):
        xfa.flash_attn_varlen_func(q.clone().requires_grad_(), k, v, cq, ck, mq, mk)
    torch.cuda.synchronize()
    assert torch.isnan(o).all() and torch.isnan(lse).all()


# ------------------------------------------------------------------ schedules ------------------
H_S, S_S = 19, 1100
KNOBS = (b"fwd_persistent", b"fwd_order", b"fwd_dyn", b"fwd_xcdq")


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _batch():
    """test_fwd_sched_gpu's: the smallest batch with more items than CUs and a unit count that is
    no multiple of 8 (1100 rows = 5 items of 256, the last partial)."""
    b = 1
    while not (b * H_S * ((S_S + mu.ROWS - 1) // mu.ROWS) > _cus() and (b * H_S) % 8):
        b += 1
    return b


def test_every_schedule_gives_the_baseline():
    from xf_flash_attention_cutlass_amd import capi
    L = capi.lib()
    b = _batch()
    g = torch.Generator().manual_seed(19)
    q = torch.randn(b, S_S, H_S, mu.DQK, generator=g).bfloat16()
    k = torch.randn(b, S_S, H_S, mu.DQK, generator=g).bfloat16()
    v = torch.randn(b, S_S, H_S, mu.DV, generator=g).bfloat16()
    qd, kd, vd = _dev(q, k, v)

    def run(options, persistent, xcdq):
        for knob, val in options.items():
            assert L.fmha_set_option(knob, val) == 0, L.fmha_last_error()
        o, lse, kern = mu.run_dense(qd, kd, vd, (-1, 0))
        assert kern.startswith(f"{mu.KERNEL} persistent={persistent} xcdq={xcdq} "), kern
        return o.cpu(), lse.cpu()

    pairs = 2 if _cus() % 8 == 0 else 1
    old = {knob: L.fmha_get_option(knob) for knob in KNOBS}
    try:
        base = run({b"fwd_persistent": 0}, 0, 0)
        # order, dyn, xcdq; the dynamic queues twice (their counters reset themselves)
        for order, dyn, xcdq in [(0, 0, 1), (1, 0, 1), (1, 2, 1), (1, 2, 1), (1, 2, 0), (1, 2, 0)]:
            want = (3, int(xcdq and _cus() % 8 == 0 and b * H_S >= 8)) if dyn == 2 else (pairs if order else 1, 0)
            got = run({b"fwd_persistent": 1, b"fwd_order": order, b"fwd_dyn": dyn, b"fwd_xcdq": xcdq}, *want)
            assert torch.equal(got[0].view(torch.int16), base[0].view(torch.int16)), (order, dyn, xcdq)
            assert torch.equal(got[1].view(torch.int32), base[1].view(torch.int32)), (order, dyn, xcdq)
    finally:
        for knob, val in old.items():
            L.fmha_set_option(knob, val)
    # the baseline against the oracle, two sampled (batch, head) pairs
    for bi, hi in ((0, 0), (b - 1, H_S - 1)):
        s = mu.oracle_one(q[bi, :, hi:hi + 1], k[bi, :, hi:hi + 1], v[bi, :, hi:hi + 1], (-1, 0))
        ok, f = su.judge(base[0][bi:bi + 1, :, hi:hi + 1], base[1][bi:bi + 1, hi:hi + 1], su.Refs(s.ref, s.pt, s.lse, None))
        print(f"fwd_mla schedules baseline ({bi}, {hi}): o err {f['err']:.3e} bound {f['bound']:.3e}; lse err {f['lse_err']:.3e}")
        assert ok, f


# ------------------------------------------------------------------ chunked prefill ------------
@pytest.mark.parametrize("dt", DTS)
def test_chunked_prefill_composes_with_merge_attn_states(dt, parity_report):
    """One sequence, 203 cached and 113 new tokens: the new queries over the cached keys (full) and
    over the new keys (causal), merged, against the oracle over all 316 keys."""
    import xf_flash_attention_cutlass_amd as xfa
    h, hk, cached, new = 6, 2, 203, 113
    q, k, v = mu.make_packed([new], [cached + new], h, hk, mu.DTYPES[dt], seed=17)
    seqs = mu.oracle(q, k, v, [new], [cached + new], (-1, 0))
    qd, kd, vd = _dev(q, k, v)
    o_a, l_a, _ = mu.run_varlen(qd, kd[:cached], vd[:cached], [new], [cached], h, hk, (-1, -1))
    o_b, l_b, _ = mu.run_varlen(qd, kd[cached:], vd[cached:], [new], [new], h, hk, (-1, 0))
    o, lse = xfa.merge_attn_states([o_a, o_b], [l_a, l_b], packed=True)
    mu.assert_case(f"fwd_mla chunked prefill {dt}", o.cpu(), lse.cpu(), seqs, [new], parity_report)
