"""GPU: fmha_merge_states (through `paged_attn.merge_states` and the C ABI) against
`merge_ref` in float64 on the same low-precision inputs.

Pass rule: elementwise |o - ref64| <= eps |ref64| + 1e-6 max|o_parts| with eps
from the tests' EPS table (one rounding of the result to the dtype; the second term covers the
fp32 evaluation of the weights and the sum); the LSE's +inf pattern equal to the reference's and
its finite values within LSE_ATOL = 1e-3 (the measured error goes to the parity report).

Every input mixes, by (batch, row, head), rows whose parts' LSEs are ordinary, differ by more than
100 (weights underflow to 0), are equal, have an absent part by +inf or by -inf (its O all NaN),
or have no part present at all (O = 0 exactly, LSE = +inf)."""
import ctypes as C

import pytest
import torch

from tests import bwd_util as bu
from tests import merge_ref as mr
from tests import sink_ref as sr
from xf_flash_attention_cutlass_amd import capi

pytestmark = pytest.mark.gpu
DEV = "cuda"
INF = float("inf")
NAN = float("nan")
B, H = 2, 3
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
NPATTERN = 6


@pytest.fixture(scope="module")
def pa():
    import xf_flash_attention_cutlass_amd as m
    return m.paged_attn


def make_parts(n, b, rows, h, d, dtype, seed):
    """n parts (o [b, rows, h, d] dtype, lse [b, h, rows] fp32) on the CPU; the pattern of row
    (bi, row, head) is ((bi * rows + row) * h + head) % 6 (see the module docstring)."""
    g = torch.Generator().manual_seed(seed)
    os_ = [(torch.randn(b, rows, h, d, generator=g) * 2).to(dtype) for _ in range(n)]
    ls = [torch.randn(b, h, rows, generator=g) * 3 for _ in range(n)]
    idx = (torch.arange(b).view(b, 1, 1) * rows + torch.arange(rows).view(1, 1, rows)) * h + \
        torch.arange(h).view(1, h, 1)
    pat = idx % NPATTERN                                              # [b, h, rows]
    pat_o = pat.permute(0, 2, 1).unsqueeze(-1)                        # [b, rows, h, 1]
    for i in range(n):
        ls[i] = torch.where(pat == 1, ls[0] + 150.0 * i, ls[i])       # far apart
        ls[i] = torch.where(pat == 2, ls[0], ls[i])                   # equal
    absent = [(3, 0, INF), (4, n - 1, -INF)] + [(5, i, INF if i % 2 == 0 else -INF) for i in range(n)]
    for p, i, val in absent:
        ls[i] = torch.where(pat == p, torch.full_like(ls[i], val), ls[i])
        os_[i] = torch.where(pat_o == p, torch.full_like(os_[i], NAN), os_[i])
    return [o.contiguous() for o in os_], [l.contiguous() for l in ls]


def pack(os_, ls):
    """dense parts -> packed [b * rows, h, d] / [h, b * rows]"""
    return ([o.reshape(-1, *o.shape[2:]) for o in os_],
            [l.permute(1, 0, 2).reshape(l.shape[1], -1).contiguous() for l in ls])


def check(name, o, lse, os_, ls, dtype, report, sink=None):
    ro, rl = mr.merge_ref([x.double() for x in os_], [x.double() for x in ls],
                          None if sink is None else sink.double())
    o, lse = o.double().cpu(), lse.double().cpu()
    amax = max(x[torch.isfinite(x)].abs().max().item() for x in os_)
    assert torch.isfinite(o).all(), f"{name}: O has non-finite values"
    err = (o - ro).abs()
    bound = sr.EPS[dtype] * ro.abs() + 1e-6 * amax
    worst = (err / bound).max().item()
    fin = torch.isfinite(rl)
    dl = (lse[fin] - rl[fin]).abs()
    lse_err = dl.max().item() if dl.numel() else 0.0
    print(f"{name}: o worst err/bound {worst:.3f}; lse err {lse_err:.3e}")
    if report is not None:
        report(dict(case=name, metric="o err/bound", err=worst, bound=1.0))
        report(dict(case=name, metric="lse", err=lse_err, bound=sr.LSE_ATOL))
    assert worst <= 1.0, f"{name}: |o - ref| exceeds eps |ref| + 1e-6 max|o_parts| by x{worst:.2f}"
    assert torch.equal(torch.isinf(lse) & (lse > 0), ~fin), f"{name}: the LSE's +inf rows differ"
    assert lse_err <= sr.LSE_ATOL, f"{name}: LSE off by {lse_err:.3e}"
    dead = ~fin.permute(0, 2, 1) if ro.dim() == 4 else ~fin.permute(1, 0)
    assert (o[dead] == 0).all(), f"{name}: O != 0 on a row with no part present"


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("n", [1, 2, 3, 16])
@pytest.mark.parametrize("d", [8, 40, 128, 256])
def test_merge_matches_ref(pa, parity_report, d, n, dt):
    dtype = DTYPES[dt]
    worst = bu.WorstRows()
    for rows in (1, 67):
        os_, ls = make_parts(n, B, rows, H, d, dtype, 100 * d + n)
        for packed in (False, True):
            po, pl = pack(os_, ls) if packed else (os_, ls)
            o, lse = pa.merge_states([x.to(DEV) for x in po], [x.to(DEV) for x in pl], None, packed)
            assert o.dtype == dtype and lse.dtype == torch.float32 and o.shape == po[0].shape
            check(f"merge d{d} n{n} {dt} rows{rows} {'packed' if packed else 'dense'}", o, lse, po, pl,
                  dtype, worst)
    worst.flush(parity_report)


def test_merge_with_sink(pa, parity_report):
    """sink_values(4): a +20 head and a -inf head; sink = None against sink = -inf bit for bit."""
    h = 4
    for d, n, dtype in ((128, 3, torch.bfloat16), (40, 2, torch.float16)):
        os_, ls = make_parts(n, B, 67, h, d, dtype, 7)
        sink = sr.sink_values(h)
        od, ld = [x.to(DEV) for x in os_], [x.to(DEV) for x in ls]
        o, lse = pa.merge_states(od, ld, sink.to(DEV), False)
        check(f"merge sink d{d} n{n}", o, lse, os_, ls, dtype, parity_report, sink)
        o0, l0 = pa.merge_states(od, ld, None, False)
        o1, l1 = pa.merge_states(od, ld, torch.full((h,), -INF, device=DEV), False)
        assert torch.equal(o0.view(torch.int16), o1.view(torch.int16))
        assert torch.equal(l0.view(torch.int32), l1.view(torch.int32))
        # the -inf head of sink_values is that head of the call without a sink, bit for bit
        assert torch.equal(o[:, :, h - 2].view(torch.int16), o0[:, :, h - 2].view(torch.int16))


def test_views_in_poisoned_arena(pa):
    """Parts and outputs as head-sliced, half-row-range views inside a NaN-poisoned arena: the
    guards and every element outside the output views keep the poison."""
    n, rows, d, dtype = 3, 67, 40, torch.bfloat16
    os_, ls = make_parts(n, B, rows, H, d, dtype, 11)
    specs = {}
    for i in range(n + 1):
        specs[f"o{i}"] = ((B, 2 * rows, H + 2, d), dtype)
        specs[f"l{i}"] = ((B, H + 2, 2 * rows), torch.float32)
    ar = bu.Arena(specs)
    ov = lambda i: ar[f"o{i}"][:, rows:, 1:1 + H]          # noqa: E731
    lv = lambda i: ar[f"l{i}"][:, 1:1 + H, rows:]          # noqa: E731
    for i in range(n):
        ov(i).copy_(os_[i])
        lv(i).copy_(ls[i])
    before = ar.buf.clone()
    o, lse = pa.merge_states([ov(i) for i in range(n)], [lv(i) for i in range(n)], None, False, ov(n), lv(n))
    torch.cuda.synchronize()
    assert o.data_ptr() == ov(n).data_ptr() and lse.data_ptr() == lv(n).data_ptr()
    ar.assert_guards("merge views")
    check("merge arena views", o, lse, os_, ls, dtype, None)
    # outside the two output views nothing changed (the poison included): the arena before the
    # call with the two results pasted in is, byte for byte, the arena after it
    after, ro, rl = ar.buf.clone(), o.clone(), lse.clone()
    ar.buf.copy_(before)
    ov(n).copy_(ro)
    lv(n).copy_(rl)
    assert torch.equal(ar.buf, after), "bytes outside the output views changed"


def test_in_place_and_reproducible(pa):
    """o / lse = part 0's buffers gives the bits of the out-of-place call, which are the same in
    two calls (d = 40: the threads of a row straddle two waves)."""
    for d, n in ((40, 3), (128, 16)):
        os_, ls = make_parts(n, B, 67, H, d, torch.bfloat16, 13)
        od, ld = [x.to(DEV) for x in os_], [x.to(DEV) for x in ls]
        o1, l1 = pa.merge_states(od, ld, None, False)
        o2, l2 = pa.merge_states(od, ld, None, False)
        assert torch.equal(o1.view(torch.int16), o2.view(torch.int16))
        assert torch.equal(l1.view(torch.int32), l2.view(torch.int32))
        o3, l3 = pa.merge_states(od, ld, None, False, od[0], ld[0])
        assert o3.data_ptr() == od[0].data_ptr()
        assert torch.equal(o1.view(torch.int16), o3.view(torch.int16))
        assert torch.equal(l1.view(torch.int32), l3.view(torch.int32))


def test_python_wrapper_no_grad_and_lse_null(pa):
    import xf_flash_attention_cutlass_amd as xfa
    os_, ls = make_parts(2, B, 5, H, 64, torch.bfloat16, 17)
    od = [x.to(DEV).requires_grad_(True) for x in os_]
    ld = [x.to(DEV) for x in ls]
    o, lse = xfa.merge_attn_states(od, ld)
    assert not o.requires_grad and not lse.requires_grad
    check("merge_attn_states", o, lse, os_, ls, torch.bfloat16, None)
    # the C entry with lse = NULL writes O alone
    L = capi.lib()
    out = torch.empty_like(o)
    op = (C.c_void_p * 2)(*[x.data_ptr() for x in od])
    lp = (C.c_void_p * 2)(*[x.data_ptr() for x in ld])
    st = (C.c_int64 * 10)(*od[0].stride()[:3], *out.stride()[:3], *ld[0].stride()[:2], *lse.stride()[:2])
    L.fmha_merge_states(op, lp, 2, out.data_ptr(), None, None, B, 5, H, 64, st, False,
                        capi.stream_handle())
    assert L.fmha_last_status() == 0, L.fmha_last_error()
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int16), o.view(torch.int16))


def test_17_parts_refused_outputs_untouched(pa):
    os_, ls = make_parts(1, B, 5, H, 64, torch.bfloat16, 19)
    od, ld = [os_[0].to(DEV).clone() for _ in range(17)], [ls[0].to(DEV).clone() for _ in range(17)]
    out = torch.full_like(od[0], 7.0)
    lse = torch.full_like(ld[0], 7.0)
    with pytest.raises(RuntimeError, match="1 to 16 parts"):
        pa.merge_states(od, ld, None, False, out, lse)
    L = capi.lib()
    op = (C.c_void_p * 17)(*[x.data_ptr() for x in od])
    lp = (C.c_void_p * 17)(*[x.data_ptr() for x in ld])
    st = (C.c_int64 * 10)(*od[0].stride()[:3], *out.stride()[:3], *ld[0].stride()[:2], *lse.stride()[:2])
    L.fmha_merge_states(op, lp, 17, out.data_ptr(), lse.data_ptr(), None, B, 5, H, 64, st, False,
                        capi.stream_handle())
    assert L.fmha_last_status() != 0 and "num_parts must be in [1, 16]" in L.fmha_last_error().decode()
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (lse == 7.0).all()


def test_graph_capture_and_replay(pa):
    """One merge captured in a graph (the part pointers travel in the kernel arguments: no copy, no
    allocation by the library, no sync) and replayed on new contents of the same buffers."""
    n, d = 3, 128
    a_o, a_l = make_parts(n, B, 67, H, d, torch.bfloat16, 23)
    b_o, b_l = make_parts(n, B, 67, H, d, torch.bfloat16, 29)
    od, ld = [x.to(DEV) for x in a_o], [x.to(DEV) for x in a_l]
    out, lse = torch.zeros_like(od[0]), torch.zeros_like(ld[0])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        pa.merge_states(od, ld, None, False, out, lse)           # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        pa.merge_states(od, ld, None, False, out, lse)
    for x, y in zip(od + ld, b_o + b_l):
        x.copy_(y)
    graph.replay()
    torch.cuda.synchronize()
    eo, el = pa.merge_states(od, ld, None, False)
    assert torch.equal(out.view(torch.int16), eo.view(torch.int16))
    assert torch.equal(lse.view(torch.int32), el.view(torch.int32))
    check("merge graph replay", out, lse, b_o, b_l, torch.bfloat16, None)
