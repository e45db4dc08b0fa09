"""GPU: the fp8 forward with descales read on the device (fmha_fwd_fp8_ex /
fmha_varlen_fwd_fp8_ex): one element or FA3's [batch, heads_k] tensors, no host sync.

Inputs: the (batch, kv head) groups of q, k and v are multiplied by {1, 1/16, 8} in turn (q, k and
v take the factors one step apart, so every product of a q and a k factor occurs) and quantised
per (batch, kv head) on the CPU (tests/fp8_quant_util.quantize_ref, independent of the quantising
kernel).  Parity is tests/test_fp8_gpu.py's rule, max|out - ref| <= 3 max|pt - ref| + 1e-3 and
|LSE - ref| < 1e-3, against oracle.attention_fp8_pt / attention_ref with the scales broadcast as
[b, 1, h, 1] - applied per (batch, head) slice, so a wrong scale on a small head cannot hide under
a large head's error.  Bit identity: equal scales give equal bits whether passed by value, as
one-element device tensors or as a constant [b, hk] tensor.  Every kernel fp8_w4 selects runs the
same cases (2: the variants library through the C ABI), the kernel id asserted each time."""
import pytest
import torch

from oracle import attention_ref as orc
from tests.fp8_quant_util import per_head, quantize_ref, scale_groups, slice_parity

pytestmark = pytest.mark.gpu
DEV = "cuda"
KERNEL = {0: "fmha_fwd_fp8_kernel", 1: "fmha_fwd8w_kernel", 2: "fmha_fwd8pp_kernel"}
D = 128


@pytest.fixture(scope="module")
def xfa():
    import xf_flash_attention_cutlass_amd as m
    return m


def _lib():
    from xf_flash_attention_cutlass_amd import capi
    return capi.lib()


_VAR = {}


def _variants():
    if "lib" not in _VAR:
        from xf_flash_attention_cutlass_amd import capi
        _VAR["lib"] = capi.load(capi.VARIANTS_PATH)
    return _VAR["lib"]


class _fp8_w4:
    """fp8_w4 = value on `lib` for the block, the old value back afterwards"""

    def __init__(self, lib, value):
        self.lib, self.value = lib, value

    def __enter__(self):
        self.old = self.lib.fmha_get_option(b"fp8_w4")
        assert self.lib.fmha_set_option(b"fp8_w4", self.value) == 0, self.lib.fmha_last_error()

    def __exit__(self, *exc):
        self.lib.fmha_set_option(b"fp8_w4", self.old)


def _assert_kernel(lib, w4):
    kern = lib.fmha_last_kernel().decode()
    assert kern.startswith(KERNEL[w4]), kern


_CASES = {}


def _dense_case(b, h, hk, sq, sk):
    """per-head quantised inputs and the oracle's out / estimate / LSE, computed once per shape
    and causal flag (shared by the fp8_w4 settings; never modified)"""
    key = (b, h, hk, sq, sk)
    if key not in _CASES:
        g = torch.Generator().manual_seed(sq * 7 + sk)
        q = scale_groups(torch.randn(b, sq, h, D, generator=g), hk, shift=0)
        k = scale_groups(torch.randn(b, sk, hk, D, generator=g), hk, shift=1)
        v = scale_groups(torch.randn(b, sk, hk, D, generator=g), hk, shift=2)
        (q8, qd), (k8, kd), (v8, vd) = (quantize_ref(x, "head", grp) for x, grp in
                                        ((q, h // hk), (k, 1), (v, 1)))
        _CASES[key] = dict(q8=q8, k8=k8, v8=v8, qd=qd, kd=kd, vd=vd, ref={})
    return _CASES[key]


def _oracle(c, causal):
    if causal not in c["ref"]:
        h = c["q8"].shape[2]
        qs, ks, vs = per_head(c["qd"], h), c["kd"][:, None, :, None], c["vd"][:, None, :, None]
        qf, kf, vf = c["q8"].float() * qs, c["k8"].float() * ks, c["v8"].float() * vs
        ref, _ = orc.attention_ref(qf, kf, vf, causal=causal)
        pt = orc.attention_fp8_pt(c["q8"], c["k8"], c["v8"], qs, ks, vs, causal=causal).bfloat16()
        c["ref"][causal] = (ref, pt, orc.attention_lse_ref(qf, kf, causal=causal))
    return c["ref"][causal]


def _check_dense(c, causal, out, lse):
    ref, pt, lref = _oracle(c, causal)
    bad = slice_parity(out.cpu(), ref, pt, 3.0, 1e-3)
    assert not bad, f"(batch, head, err, bound): {bad}"
    fin = torch.isfinite(lref)
    assert torch.equal(torch.isinf(lse.cpu()), ~fin)
    assert (lse.cpu()[fin] - lref[fin]).abs().max().item() < 1e-3


DENSE = [(2, 4, 2, 113, 203, False), (2, 4, 2, 113, 203, True), (1, 8, 2, 300, 300, True)]


@pytest.mark.parametrize("w4", [1, 0])
@pytest.mark.parametrize("b,h,hk,sq,sk,causal", DENSE)
def test_dense_per_head_descales(xfa, b, h, hk, sq, sk, causal, w4):
    c = _dense_case(b, h, hk, sq, sk)
    dev = {n: c[n].to(DEV) for n in ("q8", "k8", "v8", "qd", "kd", "vd")}
    with _fp8_w4(_lib(), w4):
        out, lse = xfa.flash_attn_fp8_func(dev["q8"], dev["k8"], dev["v8"], dev["qd"], dev["kd"],
                                           dev["vd"], causal=causal, return_lse=True)
        torch.cuda.synchronize()
        _assert_kernel(_lib(), w4)
    _check_dense(c, causal, out, lse)


def _c_fwd(lib, ex, q8, k8, v8, scales, strides, causal):
    """fmha_fwd_fp8 (ex = False: scales are floats) or fmha_fwd_fp8_ex (device tensors and their
    (batch, head) strides) of `lib`; returns (out, lse)"""
    from xf_flash_attention_cutlass_amd import capi
    b, sq, h, _ = q8.shape
    sk, hk = k8.shape[1], k8.shape[2]
    out = torch.empty(b, sq, h, D, device=DEV, dtype=torch.bfloat16)
    lse = torch.empty(b, h, sq, device=DEV, dtype=torch.float32)
    tail = (sq, sk, b, h, hk, D, D ** -0.5, -1, 0 if causal else -1, False, capi.stream_handle())
    if ex:
        lib.fmha_fwd_fp8_ex(q8.data_ptr(), k8.data_ptr(), v8.data_ptr(), out.data_ptr(), lse.data_ptr(),
                            *(s.data_ptr() for s in scales), *strides, *tail)
    else:
        lib.fmha_fwd_fp8(q8.data_ptr(), k8.data_ptr(), v8.data_ptr(), out.data_ptr(), lse.data_ptr(),
                         *scales, *tail)
    assert lib.fmha_last_status() == 0, lib.fmha_last_error()
    torch.cuda.synchronize()
    return out, lse


@pytest.mark.parametrize("b,h,hk,sq,sk,causal", DENSE)
def test_dense_per_head_descales_pingpong(b, h, hk, sq, sk, causal):
    """fp8_w4 = 2 (the variants library): the same cases through the C ABI"""
    V = _variants()
    c = _dense_case(b, h, hk, sq, sk)
    dev = {n: c[n].to(DEV) for n in ("q8", "k8", "v8", "qd", "kd", "vd")}
    with _fp8_w4(V, 2):
        out, lse = _c_fwd(V, True, dev["q8"], dev["k8"], dev["v8"], (dev["qd"], dev["kd"], dev["vd"]),
                          (hk, 1), causal)
        _assert_kernel(V, 2)
    _check_dense(c, causal, out, lse)


def _const_scales(b, hk):
    vals = (0.013, 0.21, 1.7)
    floats = [float(torch.tensor(x, dtype=torch.float32)) for x in vals]
    one = [torch.tensor([x], dtype=torch.float32, device=DEV) for x in vals]
    full = [torch.full((b, hk), x, dtype=torch.float32, device=DEV) for x in vals]
    return floats, one, full


@pytest.mark.parametrize("w4", [1, 0])
@pytest.mark.parametrize("b,h,hk,sq,sk,causal", DENSE)
def test_dense_bit_identity(xfa, b, h, hk, sq, sk, causal, w4):
    """by value == one-element device tensors == a constant [b, hk] tensor, bit for bit"""
    c = _dense_case(b, h, hk, sq, sk)
    q8, k8, v8 = (c[n].to(DEV) for n in ("q8", "k8", "v8"))
    floats, one, full = _const_scales(b, hk)
    res = []
    with _fp8_w4(_lib(), w4):
        for ds in (floats, one, full):
            res.append(xfa.flash_attn_fp8_func(q8, k8, v8, *ds, causal=causal, return_lse=True))
            torch.cuda.synchronize()
            _assert_kernel(_lib(), w4)
    for out, lse in res[1:]:
        assert torch.equal(out, res[0][0]) and torch.equal(lse, res[0][1])


@pytest.mark.parametrize("b,h,hk,sq,sk,causal", DENSE[1:])
def test_dense_bit_identity_pingpong(b, h, hk, sq, sk, causal):
    V = _variants()
    c = _dense_case(b, h, hk, sq, sk)
    q8, k8, v8 = (c[n].to(DEV) for n in ("q8", "k8", "v8"))
    floats, one, full = _const_scales(b, hk)
    with _fp8_w4(V, 2):
        res = [_c_fwd(V, False, q8, k8, v8, floats, None, causal),
               _c_fwd(V, True, q8, k8, v8, one, (0, 0), causal),
               _c_fwd(V, True, q8, k8, v8, full, (hk, 1), causal)]
        _assert_kernel(V, 2)
    for out, lse in res[1:]:
        assert torch.equal(out, res[0][0]) and torch.equal(lse, res[0][1])


# ---- packed: lengths q [1, 0, 77, 130], k [64, 9, 77, 200]; "batch" is the sequence index
LQ, LK = [1, 0, 77, 130], [64, 9, 77, 200]
H, HK = 4, 2


def _cu(lens):
    return [0] + torch.tensor(lens).cumsum(0).tolist()


def _packed_case():
    if "packed" not in _CASES:
        g = torch.Generator().manual_seed(42)
        cq, ck = _cu(LQ), _cu(LK)
        nb = len(LQ)

        def groups(total, heads, cu, shift):     # [total, heads, D] scaled per (sequence, kv head)
            x = torch.randn(total, heads, D, generator=g)
            for i in range(nb):
                if cu[i + 1] > cu[i]:
                    x[cu[i]:cu[i + 1]] = scale_groups(x[None, cu[i]:cu[i + 1]], HK, shift=shift + i * HK)[0]
            return x
        q, k, v = groups(cq[-1], H, cq, 0), groups(ck[-1], HK, ck, 1), groups(ck[-1], HK, ck, 2)
        (q8, qd), (k8, kd), (v8, vd) = (quantize_ref(x, "head", grp, cu) for x, grp, cu in
                                        ((q, H // HK, cq), (k, 1, ck), (v, 1, ck)))
        _CASES["packed"] = dict(q8=q8, k8=k8, v8=v8, qd=qd, kd=kd, vd=vd, cq=cq, ck=ck, ref={})
    return _CASES["packed"]


def _check_packed(c, causal, out, lse):
    out, lse = out.cpu(), lse.cpu()
    cq, ck = c["cq"], c["ck"]
    if causal not in c["ref"]:
        refs = []
        for i in range(len(LQ)):
            if LQ[i] == 0:
                refs.append(None)
                continue
            q8, k8, v8 = c["q8"][None, cq[i]:cq[i + 1]], c["k8"][None, ck[i]:ck[i + 1]], c["v8"][None, ck[i]:ck[i + 1]]
            qs, ks, vs = (per_head(c["qd"][i:i + 1], H), c["kd"][i:i + 1, None, :, None],
                          c["vd"][i:i + 1, None, :, None])
            qf, kf, vf = q8.float() * qs, k8.float() * ks, v8.float() * vs
            ref, _ = orc.attention_ref(qf, kf, vf, causal=causal)
            pt = orc.attention_fp8_pt(q8, k8, v8, qs, ks, vs, causal=causal).bfloat16()
            refs.append((ref, pt, orc.attention_lse_ref(qf, kf, causal=causal)))
        c["ref"][causal] = refs
    for i, r in enumerate(c["ref"][causal]):
        if r is None:
            continue
        ref, pt, lref = r
        bad = slice_parity(out[None, cq[i]:cq[i + 1]], ref, pt, 3.0, 1e-3)
        assert not bad, f"sequence {i} (batch, head, err, bound): {bad}"
        got = lse[:, cq[i]:cq[i + 1]][None]
        fin = torch.isfinite(lref)
        assert torch.equal(torch.isinf(got), ~fin)
        assert (got[fin] - lref[fin]).abs().max().item() < 1e-3


def _packed_run(xfa, c, ds, causal):
    cq = torch.tensor(c["cq"], dtype=torch.int32, device=DEV)
    ck = torch.tensor(c["ck"], dtype=torch.int32, device=DEV)
    r = xfa.flash_attn_varlen_fp8_func(c["q8"].to(DEV), c["k8"].to(DEV), c["v8"].to(DEV), cq, ck,
                                       max(LQ), max(LK), *ds, causal=causal, return_lse=True)
    torch.cuda.synchronize()
    return r


@pytest.mark.parametrize("w4", [1, 0, 2])
@pytest.mark.parametrize("causal", [False, True])
def test_packed_per_head_descales(xfa, causal, w4):
    c = _packed_case()
    if w4 == 2:
        # the ping-pong kernel is dense only: under fp8_w4 = 2 a packed launch runs the 4-wave
        # kernel (the variants library, through the C ABI)
        from xf_flash_attention_cutlass_amd import capi
        V = _variants()
        dev = {n: c[n].to(DEV) for n in ("q8", "k8", "v8", "qd", "kd", "vd")}
        cq = torch.tensor(c["cq"], dtype=torch.int32, device=DEV)
        ck = torch.tensor(c["ck"], dtype=torch.int32, device=DEV)
        out = torch.zeros(sum(LQ), H, D, device=DEV, dtype=torch.bfloat16)
        lse = torch.zeros(H, sum(LQ), device=DEV, dtype=torch.float32)
        with _fp8_w4(V, 2):
            V.fmha_varlen_fwd_fp8_ex(dev["q8"].data_ptr(), dev["k8"].data_ptr(), dev["v8"].data_ptr(),
                                     out.data_ptr(), lse.data_ptr(), cq.data_ptr(), ck.data_ptr(), None,
                                     dev["qd"].data_ptr(), dev["kd"].data_ptr(), dev["vd"].data_ptr(),
                                     HK, 1, max(LQ), max(LK), sum(LQ), len(LQ), H, HK, D, D ** -0.5,
                                     -1, 0 if causal else -1, False, capi.stream_handle())
            assert V.fmha_last_status() == 0, V.fmha_last_error()
            torch.cuda.synchronize()
            _assert_kernel(V, 1)
    else:
        with _fp8_w4(_lib(), w4):
            out, lse = _packed_run(xfa, c, [c[n].to(DEV) for n in ("qd", "kd", "vd")], causal)
            _assert_kernel(_lib(), w4)
    _check_packed(c, causal, out, lse)


@pytest.mark.parametrize("w4", [1, 0])
@pytest.mark.parametrize("causal", [False, True])
def test_packed_bit_identity(xfa, causal, w4):
    c = _packed_case()
    floats, one, full = _const_scales(len(LQ), HK)
    with _fp8_w4(_lib(), w4):
        res = [_packed_run(xfa, c, ds, causal) for ds in (floats, one, full)]
        _assert_kernel(_lib(), w4)
    for out, lse in res[1:]:
        assert torch.equal(out, res[0][0]) and torch.equal(lse, res[0][1])
