"""GPU: the fp8 (e4m3fn) forward over packed variable-length batches (fmha_varlen_fwd_fp8,
paged_attn.varlen_fwd_fp8, flash_attn_varlen_fp8_func).

The main check needs no tolerance: an item of the varlen launch computes exactly what the dense
kernel computes for that sequence alone (the same tiles, limits and descriptor extents), so every
sequence's rows of O and of the LSE must equal, bit for bit, the dense fp8 call on that sequence
(batch 1).  Against the oracle the project's fp8 rule holds unchanged (tests/test_fp8_gpu.py):
max|out - ref| <= 3 x max|pt - ref| + 1e-3, the LSE within 1e-3 and its inf pattern equal.
"""
import itertools

import pytest
import torch

from oracle import attention_ref as orc

pytestmark = pytest.mark.gpu
DEV = "cuda"

LEN_Q = [113, 300, 1, 257, 64, 65]
LEN_K = [203, 300, 777, 40, 64, 129]
FP8_MAX_BYTE = 0x7E          # e4m3fn 448, the largest finite value


@pytest.fixture(scope="module")
def xfa():
    import xf_flash_attention_cutlass_amd as m
    return m


def _lib():
    from xf_flash_attention_cutlass_amd import capi
    return capi.lib()


def _cu(lens):
    return torch.tensor([0] + list(itertools.accumulate(lens)), dtype=torch.int32)


def _packed(len_q, len_k, h, hk, seed):
    """packed fp8 q/k/v (per-tensor scales) on the device, with their cu_seqlens"""
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(sum(len_q), h, 128, generator=g)
    k = torch.randn(sum(len_k), hk, 128, generator=g)
    v = torch.randn(sum(len_k), hk, 128, generator=g)
    (q8, qs), (k8, ks), (v8, vs) = [orc.quantize_fp8(x) for x in (q, k, v)]
    return dict(q8=q8.to(DEV), k8=k8.to(DEV), v8=v8.to(DEV), qs=qs, ks=ks, vs=vs,
                cu_q=_cu(len_q).to(DEV), cu_k=_cu(len_k).to(DEV), len_q=list(len_q),
                len_k=list(len_k), h=h, hk=hk)


def _varlen(xfa, c, causal=False, window=(-1, -1), out_dtype=torch.bfloat16, seqused_k=None,
            poison=True):
    """the pybind call into a NaN-filled out_; returns (out, lse) after checking no NaN is left"""
    total_q = c["q8"].shape[0]
    out_ = torch.full((total_q, c["h"], 128), float("nan"), device=DEV, dtype=out_dtype)
    out, lse = xfa.paged_attn.varlen_fwd_fp8(
        c["q8"], c["k8"], c["v8"], out_ if poison else None, c["cu_q"], c["cu_k"], seqused_k,
        max(c["len_q"]), max(max(c["len_k"]), 1), c["qs"], c["ks"], c["vs"], 128 ** -0.5, causal,
        window[0], window[1], out_dtype == torch.float16)
    torch.cuda.synchronize()
    assert lse.shape == (c["h"], total_q) and out.shape == (total_q, c["h"], 128)
    assert not torch.isnan(out).any() and not torch.isnan(lse).any()
    return out, lse


def _dense_seq(xfa, c, i, causal, window, out_dtype, len_k=None):
    """flash_attn_fp8_func on sequence i alone: (out [sq, h, 128], lse [h, sq])"""
    q0, q1 = int(c["cu_q"][i]), int(c["cu_q"][i + 1])
    k0 = int(c["cu_k"][i])
    k1 = k0 + (len_k[i] if len_k is not None else int(c["cu_k"][i + 1]) - k0)
    out, lse = xfa.flash_attn_fp8_func(c["q8"][q0:q1][None], c["k8"][k0:k1][None],
                                       c["v8"][k0:k1][None], c["qs"], c["ks"], c["vs"],
                                       causal=causal, window_size=window, out_dtype=out_dtype,
                                       return_lse=True)
    return out[0], lse[0]


def _assert_equal_dense(xfa, c, out, lse, causal, window, out_dtype, seqs=None, len_k=None):
    for i in (range(len(c["len_q"])) if seqs is None else seqs):
        q0, q1 = int(c["cu_q"][i]), int(c["cu_q"][i + 1])
        d_out, d_lse = _dense_seq(xfa, c, i, causal, window, out_dtype, len_k)
        assert torch.equal(out[q0:q1], d_out), f"O of sequence {i} differs from its dense run"
        assert torch.equal(lse[:, q0:q1], d_lse), f"LSE of sequence {i} differs from its dense run"


def _assert_varlen_kernel():
    """a varlen launch without a left window runs the kernel fp8_w4 selects: 1 the 4-wave kernel,
    0 the 8-wave compiler-scheduled one; 2 (the dense-only ping-pong kernel of the variants build)
    falls through to the 4-wave kernel"""
    L = _lib()
    kern = L.fmha_last_kernel().decode()
    want = {0: "fmha_fwd_fp8_kernel", 1: "fmha_fwd8w_kernel", 2: "fmha_fwd8w_kernel"}
    assert kern.startswith(want[L.fmha_get_option(b"fp8_w4")]), kern


@pytest.fixture(scope="module")
def ragged():
    return _packed(LEN_Q, LEN_K, 8, 2, seed=11)


@pytest.mark.parametrize("out_dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("causal", [False, True])
def test_varlen_bit_identical_to_dense(xfa, ragged, causal, out_dtype):
    out, lse = _varlen(xfa, ragged, causal=causal, out_dtype=out_dtype)
    _assert_varlen_kernel()
    _assert_equal_dense(xfa, ragged, out, lse, causal, (-1, -1), out_dtype)


@pytest.mark.parametrize("window", [(64, 0), (100, 17)])
def test_varlen_left_windows(xfa, ragged, window):
    out, lse = _varlen(xfa, ragged, window=window)
    L = _lib()
    assert L.fmha_last_kernel().decode().startswith("fmha_fwd_fp8_kernel")
    # The dense runs of the sequences shorter than the window lose their left window (wl >=
    # seqlen_k) and would go to the 4-wave kernel, whose softmax schedule rounds differently:
    # compare against the dense launches of the same (8-wave) kernel.
    w4 = L.fmha_get_option(b"fp8_w4")
    assert L.fmha_set_option(b"fp8_w4", 0) == 0
    try:
        _assert_equal_dense(xfa, ragged, out, lse, False, window, torch.bfloat16)
    finally:
        L.fmha_set_option(b"fp8_w4", w4)


@pytest.mark.parametrize("causal,window", [(True, (-1, -1)), (False, (100, 17))])
def test_varlen_oracle_parity(xfa, ragged, causal, window, parity_report):
    c = ragged
    out, lse = _varlen(xfa, c, causal=causal, window=window)
    out, lse = out.cpu().float(), lse.cpu()
    q8, k8, v8 = c["q8"].cpu(), c["k8"].cpu(), c["v8"].cpu()
    for i in range(len(c["len_q"])):
        q0, q1 = int(c["cu_q"][i]), int(c["cu_q"][i + 1])
        k0, k1 = int(c["cu_k"][i]), int(c["cu_k"][i + 1])
        s = [q8[q0:q1][None], k8[k0:k1][None], v8[k0:k1][None]]
        qd, kd, vd = s[0].float() * c["qs"], s[1].float() * c["ks"], s[2].float() * c["vs"]
        ref, _ = orc.attention_ref(qd, kd, vd, causal=causal, window_size=window)
        pt = orc.attention_fp8_pt(*s, c["qs"], c["ks"], c["vs"], causal=causal,
                                  window_size=window).to(torch.bfloat16)
        ok, err, bound = orc.parity_ok(out[q0:q1][None], ref, pt, 3.0, 1e-3)
        parity_report({"case": f"fp8 varlen seq{i} {q1 - q0}x{k1 - k0} c{causal} w{window}",
                       "err": err, "bound": bound, "ok": bool(ok)})
        assert ok, f"sequence {i}: max|out-ref|={err:.3g} > {bound:.3g}"
        lref = orc.attention_lse_ref(qd, kd, causal=causal, window_size=window)[0]
        fin = torch.isfinite(lref)
        got = lse[:, q0:q1]
        assert torch.equal(torch.isinf(got), ~fin), f"sequence {i}: inf pattern of the LSE"
        if fin.any():
            assert (got[fin] - lref[fin]).abs().max().item() < 1e-3, f"sequence {i}: LSE"


@pytest.mark.parametrize("causal", [False, True])
def test_varlen_empty_sequences(xfa, causal):
    c = _packed([50, 0, 70], [60, 30, 0], 8, 2, seed=12)
    out, lse = _varlen(xfa, c, causal=causal)
    _assert_varlen_kernel()
    # sequence 2 has no keys: O = 0, LSE = +inf; sequence 1 has no rows: nothing of it exists
    assert torch.equal(out[50:], torch.zeros_like(out[50:]))
    assert torch.equal(lse[:, 50:], torch.full_like(lse[:, 50:], float("inf")))
    _assert_equal_dense(xfa, c, out, lse, causal, (-1, -1), torch.bfloat16, seqs=[0])
    # and with the empty-key sequence in the middle, both neighbours still match
    c = _packed([50, 70, 33], [60, 0, 90], 8, 2, seed=13)
    out, lse = _varlen(xfa, c, causal=causal)
    assert torch.equal(out[50:120], torch.zeros_like(out[50:120]))
    assert torch.equal(lse[:, 50:120], torch.full_like(lse[:, 50:120], float("inf")))
    _assert_equal_dense(xfa, c, out, lse, causal, (-1, -1), torch.bfloat16, seqs=[0, 2])


@pytest.mark.parametrize("causal", [False, True])
def test_varlen_seqused_k(xfa, causal):
    used, slot = [128, 37, 0, 65], 128
    len_q = [100, 64, 33, 129]
    c = _packed(len_q, [slot] * 4, 8, 2, seed=14)
    # the truncated batch: the used rows of every slot, packed
    keep = torch.cat([torch.arange(i * slot, i * slot + u) for i, u in enumerate(used)]).to(DEV)
    t = dict(c, k8=c["k8"][keep].contiguous(), v8=c["v8"][keep].contiguous(),
             cu_k=_cu(used).to(DEV), len_k=used)
    want_out, want_lse = _varlen(xfa, t, causal=causal)
    # rows past seqused_k hold the largest finite e4m3 value: a read of them shows
    for name in ("k8", "v8"):
        x = c[name].view(torch.uint8)
        for i, u in enumerate(used):
            x[i * slot + u:(i + 1) * slot] = FP8_MAX_BYTE
    su = torch.tensor(used, dtype=torch.int32, device=DEV)
    out, lse = _varlen(xfa, c, causal=causal, seqused_k=su)
    _assert_varlen_kernel()
    assert torch.equal(out, want_out)
    assert torch.equal(lse, want_lse)
    # flash_attn_varlen_fp8_func passes seqused_k through
    o2 = xfa.flash_attn_varlen_fp8_func(c["q8"], c["k8"], c["v8"], c["cu_q"], c["cu_k"], max(len_q),
                                        slot, c["qs"], c["ks"], c["vs"], causal=causal,
                                        seqused_k=su)
    assert torch.equal(o2, want_out)


def test_varlen_schedules(xfa):
    """more items than CUs (12 x 8 x 3 row blocks > 256): every schedule gives the same bits"""
    g = torch.Generator().manual_seed(15)
    len_q = torch.randint(1, 701, (12,), generator=g).tolist()
    len_k = torch.randint(1, 701, (12,), generator=g).tolist()
    len_q[0] = 700                      # three 256-row blocks per (sequence, head)
    c = _packed(len_q, len_k, 8, 8, seed=15)
    L = _lib()
    dyn, pers = L.fmha_get_option(b"fwd_dyn"), L.fmha_get_option(b"fwd_persistent")
    outs = []
    try:
        for d, p, runs in ((0, pers, 1), (1, pers, 1), (2, pers, 2), (dyn, 0, 1)):
            assert L.fmha_set_option(b"fwd_dyn", d) == 0
            assert L.fmha_set_option(b"fwd_persistent", p) == 0
            for _ in range(runs):        # twice at fwd_dyn = 2: the counters reset themselves
                outs.append(_varlen(xfa, c, causal=True))
                kern = L.fmha_last_kernel().decode()
                _assert_varlen_kernel()
                if p == 0:
                    assert "persistent=0" in kern, kern
                elif d >= 1:
                    assert "persistent=3" in kern, kern
                else:
                    assert "persistent=3" not in kern, kern
    finally:
        L.fmha_set_option(b"fwd_dyn", dyn)
        L.fmha_set_option(b"fwd_persistent", pers)
    for out, lse in outs[1:]:
        assert torch.equal(out, outs[0][0])
        assert torch.equal(lse, outs[0][1])
    # the static schedule is itself right: the longest and the shortest sequence against dense
    i_min = min(range(12), key=lambda i: len_q[i])
    _assert_equal_dense(xfa, c, *outs[0], True, (-1, -1), torch.bfloat16, seqs=[0, i_min])


def test_varlen_routing_and_capi(xfa, ragged):
    """flash_attn_varlen_func with float8 inputs routes to flash_attn_varlen_fp8_func; the C ABI
    gives the same bytes into NaN-filled buffers"""
    from xf_flash_attention_cutlass_amd import capi
    c = ragged
    mq, mk = max(LEN_Q), max(LEN_K)
    a, a_lse, _ = xfa.flash_attn_varlen_func(c["q8"], c["k8"], c["v8"], c["cu_q"], c["cu_k"], mq, mk,
                                             causal=True, return_attn_probs=True,
                                             q_descale=c["qs"], k_descale=c["ks"],
                                             v_descale=c["vs"])
    b, b_lse = xfa.flash_attn_varlen_fp8_func(c["q8"], c["k8"], c["v8"], c["cu_q"], c["cu_k"], mq, mk,
                                              c["qs"], c["ks"], c["vs"], causal=True,
                                              return_lse=True)
    total_q = sum(LEN_Q)
    out = torch.full((total_q, 8, 128), float("nan"), device=DEV, dtype=torch.bfloat16)
    lse = torch.full((8, total_q), float("nan"), device=DEV)
    L = capi.lib()
    L.fmha_varlen_fwd_fp8(c["q8"].data_ptr(), c["k8"].data_ptr(), c["v8"].data_ptr(),
                          out.data_ptr(), lse.data_ptr(), c["cu_q"].data_ptr(),
                          c["cu_k"].data_ptr(), None, c["qs"], c["ks"], c["vs"], mq, mk, total_q,
                          len(LEN_Q), 8, 2, 128, 128 ** -0.5, -1, 0, False, capi.stream_handle())
    capi.check()
    torch.cuda.synchronize()
    _assert_varlen_kernel()
    assert not torch.isnan(out).any() and not torch.isnan(lse).any()
    assert a.dtype == torch.bfloat16
    assert torch.equal(a, b) and torch.equal(a_lse, b_lse)
    assert torch.equal(a, out) and torch.equal(a_lse, lse)
    f16 = xfa.flash_attn_varlen_func(c["q8"], c["k8"], c["v8"], c["cu_q"], c["cu_k"], mq, mk,
                                     q_descale=c["qs"], k_descale=c["ks"], v_descale=c["vs"],
                                     out_dtype=torch.float16)
    assert f16.dtype == torch.float16
