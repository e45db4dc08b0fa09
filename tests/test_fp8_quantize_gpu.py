"""GPU: fmha_quantize_fp8 against its specification, byte for byte.

Reference (tests/fp8_quant_util.quantize_ref, CPU): ds = amax.float() / 448 (1.0 for an all-zero or
empty set), bytes = (x.float() * (1 / ds)).clamp(-448, 448).to(float8_e4m3fn).  Descales and bytes
must match exactly: the divide is a correctly rounded fp32 divide on both sides, and torch's e4m3
rounding is the v_cvt_pk_fp8_f32 rounding the fp8 kernels' numerics model already rests on
(tests/fp8_model.py).  The C entry writes into caller buffers that are larger than needed and
filled with 0x55 / a sentinel: nothing outside the result may change."""
import pytest
import torch

from tests.fp8_quant_util import quantize_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAD = 4096          # poisoned bytes in front of and behind x8


@pytest.fixture(scope="module")
def xfa():
    import xf_flash_attention_cutlass_amd as m
    return m


def _input(b, s, h, d, group, dtype, seed, h_full=None):
    """[b, s, h, d] (a head slice of an h_full tensor when given) with: head magnitudes spread over
    2^-6 .. 2^3, the exact +amax and -amax elements of the whole tensor planted in (batch 0, head
    group 0), elements below 2^-9 of every descale, and (with more than one head group) head
    group 1 of the last batch all zero."""
    g = torch.Generator().manual_seed(seed)
    hf = h_full or h
    full = torch.randn(b, s, hf, d, generator=g)
    full *= torch.exp2(torch.randint(-6, 4, (1, 1, hf, 1), generator=g).float())
    full = full.to(dtype)
    x = full[:, :, 1:1 + h] if h_full else full
    top = (x.float().abs().max() * 2).to(dtype)
    x[0, 0, 0, 0] = top
    x[0, s // 2, group - 1, d - 2] = -top
    # below 2^-9 x descale = amax x 2^-9 / 448 of any set: they round to zero or the least subnormal
    tiny = (x.float().abs().amax(dim=(1, 3), keepdim=True) * 2.0 ** -19).to(dtype)
    x[:, s - 1:, :, 1::3] = tiny.expand(b, 1, h, d)[..., 1::3]
    x[:, s - 1:, :, 2::3] = -tiny.expand(b, 1, h, d)[..., 2::3] * 3
    if h // group > 1:
        x[b - 1, :, group:2 * group] = 0
    return x


def _run_c(x_dev, gran, group, cu=None, max_seqlen=None):
    """fmha_quantize_fp8 through the C ABI into poisoned buffers; returns (bytes, descale) after
    checking that nothing around them changed."""
    from xf_flash_attention_cutlass_amd import capi
    import ctypes
    L = capi.lib()
    packed = cu is not None
    h, d = x_dev.shape[-2], x_dev.shape[-1]
    b = cu.numel() - 1 if packed else x_dev.shape[0]
    s = (max_seqlen or x_dev.shape[0]) if packed else x_dev.shape[1]
    n = x_dev.numel()
    nscale = b * (h // group) if gran else 1
    buf = torch.full((PAD + n + PAD,), 0x55, dtype=torch.uint8, device=DEV)
    dsb = torch.full((nscale + 64,), -7.0, dtype=torch.float32, device=DEV)
    st = (0, x_dev.stride(0), x_dev.stride(1)) if packed else x_dev.stride()[:3]
    L.fmha_quantize_fp8(x_dev.data_ptr(), buf.data_ptr() + PAD, dsb.data_ptr(),
                        cu.data_ptr() if packed else None, b, s, h, group, d,
                        (ctypes.c_int64 * 3)(*st), gran, x_dev.dtype == torch.float16,
                        capi.stream_handle())
    capi.check()
    torch.cuda.synchronize()
    buf, dsb = buf.cpu(), dsb.cpu()
    assert bool((buf[:PAD] == 0x55).all()) and bool((buf[PAD + n:] == 0x55).all()), "wrote outside x8"
    assert bool((dsb[nscale:] == -7.0).all()), "wrote outside descale"
    return buf[PAD:PAD + n].view(x_dev.shape), dsb[:nscale]


CASES = [  # b, s, h, d, group, dtype, h_full
    (2, 97, 4, 128, 2, torch.bfloat16, 6),
    (2, 97, 4, 128, 2, torch.float16, 6),
    (1, 1, 1, 128, 1, torch.bfloat16, None),
    (2, 33, 2, 64, 1, torch.bfloat16, None),
    (1, 50, 2, 40, 2, torch.float16, None),
]


@pytest.mark.parametrize("gran", ["tensor", "head"])
@pytest.mark.parametrize("b,s,h,d,group,dtype,h_full", CASES)
def test_quantize_matches_reference_bytes(xfa, b, s, h, d, group, dtype, h_full, gran):
    x = _input(b, s, h, d, group, dtype, seed=b * 1000 + s, h_full=h_full)
    ref8, refd = quantize_ref(x, gran, group)
    refb = ref8.view(torch.uint8)
    x_dev = x.to(DEV)
    if h_full is not None:
        # the same values as a head-sliced (strided) view on the device
        full = torch.zeros(b, s, h_full, d, dtype=dtype, device=DEV)
        full[:, :, 1:1 + h] = x.to(DEV)
        x_dev = full[:, :, 1:1 + h]
        assert not x_dev.is_contiguous()
    got8, gotd = _run_c(x_dev, 1 if gran == "head" else 0, group)
    assert torch.equal(gotd, refd.flatten()), (gotd, refd)
    assert torch.equal(got8, refb), f"{int((got8 != refb).sum())} bytes differ"
    # the inputs' marks: +-amax are the largest e4m3 values, an all-zero group has descale 1.0
    assert 0x7E in refb[0, 0, 0] and 0xFE in refb[0, s // 2, group - 1]
    if gran == "head" and h // group > 1:
        assert float(gotd.view(b, h // group)[b - 1, 1]) == 1.0
        assert int(got8[b - 1, :, group:2 * group].max()) == 0
    # the Python entry gives the same tensors
    p8, pd = xfa.quantize_fp8(x_dev, gran, group)
    assert p8.dtype == torch.float8_e4m3fn and p8.shape == x.shape and p8.is_contiguous()
    assert pd.shape == refd.shape
    assert torch.equal(p8.cpu().view(torch.uint8), refb) and torch.equal(pd.cpu(), refd)


@pytest.mark.parametrize("gran", ["tensor", "head"])
@pytest.mark.parametrize("max_seqlen", [None, 128])
def test_quantize_packed(xfa, gran, max_seqlen):
    """cu_seqlens = [0, 5, 5, 133]: an empty sequence in the middle (descale 1.0), a short and a
    long one; per (sequence, head group) scales."""
    cu = [0, 5, 5, 133]
    h, d, group = 4, 128, 2
    x = _input(1, 133, h, d, group, torch.bfloat16, seed=5)[0]
    x[:5] *= 0.01                                  # the short sequence: its own, smaller scale
    # (head group 1 is all zero in the short sequence only: its descale there is 1.0)
    x[5:, group:] = torch.randn(128, h - group, d, generator=torch.Generator().manual_seed(6)).bfloat16()
    ref8, refd = quantize_ref(x, gran, group, cu if gran == "head" else None)
    cu_dev = torch.tensor(cu, dtype=torch.int32, device=DEV)
    got8, gotd = _run_c(x.to(DEV), 1 if gran == "head" else 0, group, cu_dev, max_seqlen)
    assert torch.equal(gotd, refd.flatten())
    assert torch.equal(got8, ref8.view(torch.uint8))
    if gran == "head":
        assert bool((gotd.view(3, 2)[1] == 1.0).all()) and float(gotd.view(3, 2)[0, 1]) == 1.0
    p8, pd = xfa.quantize_fp8(x.to(DEV), gran, group, cu_dev, max_seqlen=max_seqlen)
    assert torch.equal(p8.cpu().view(torch.uint8), ref8.view(torch.uint8)) and torch.equal(pd.cpu(), refd)


def test_quantize_then_forward_in_one_graph(xfa):
    """quantise (three calls) -> fmha_fwd_fp8_ex with the [b, hk] descales still on the device,
    captured once on a single stream; replayed after the inputs were overwritten in place, the
    graph gives the eager result of the new inputs bit for bit (no host value was baked in)."""
    b, s, h, hk = 2, 160, 4, 2
    g = torch.Generator().manual_seed(11)
    q, k, v = (torch.randn(b, s, n, 128, generator=g).bfloat16().to(DEV) for n in (h, hk, hk))

    def run():
        return xfa.flash_attn_fp8_func(q, k, v, causal=True, quantize="head", return_lse=True)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()                                     # this stream's scratch exists before the capture
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        out_g, lse_g = run()
    for t, scale in ((q, 3.0), (k, 0.25), (v, 7.0)):
        t.copy_((torch.randn(t.shape, generator=g) * scale).bfloat16())
    graph.replay()
    torch.cuda.synchronize()
    out_e, lse_e = run()
    torch.cuda.synchronize()
    assert torch.equal(out_g, out_e) and torch.equal(lse_g, lse_e)
    # ... and it is the quantised forward of the new inputs (not of the captured ones)
    q8, qd = xfa.quantize_fp8(q, "head", h // hk)
    k8, kd = xfa.quantize_fp8(k, "head", 1)
    v8, vd = xfa.quantize_fp8(v, "head", 1)
    out_x = xfa.flash_attn_fp8_func(q8, k8, v8, qd, kd, vd, causal=True)
    assert torch.equal(out_e, out_x)
