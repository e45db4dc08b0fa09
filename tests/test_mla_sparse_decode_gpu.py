"""GPU: fmha_mla_decode_sparse and fmha_mla_decode_sparse_fp8 (MLA decode over index-selected
tokens) against the CPU oracle per (batch, pos) - tests/mla_sparse_util.py's
flattening under tests/mla_util.py's rule, unchanged - over a 64 x 16 cache whose every slot no
query references is poisoned (NaN rows / 0xFF bytes), into NaN-filled outputs, with an index set
of its own per (batch, pos) and invalid values (-1, num_slots, INT32_MAX, INT32_MIN) sprinkled in.
Every case asserts the kernel, its mapping, its grid and the split count (mla_sparse_util.run).

topk {1, 31, 32, 33, 65, 300, 517} x num_splits {1, 3, 0} x bf16 / fp16 x both caches; the four
shapes with a whole invalid tile, a whole invalid split range, an all-invalid row and duplicates;
page 64; fill independence; bit identity with the dense decode over a sequence's slots in order,
between two calls and between the three surfaces; the wrapper without indices; a non-default
scale; strided views; refusals; graph capture; the merge with a dense partial; caches past 4 GiB.
"""
import ctypes as C

import pytest
import torch

from tests import mla_fp8_util as m8
from tests import mla_sparse_util as su
from tests import mla_util as mu
from xf_flash_attention_cutlass_amd import capi

pytestmark = pytest.mark.gpu

DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
KINDS = ("kv16", "fp8")
TOPKS = (1, 31, 32, 33, 65, 300, 517)
# (heads, seqlen_q): one head tile; a partial head tile per position; 8 head tiles; 3 head tiles a
# position, the last half full
SHAPES = {"h16_sq1": (16, 1), "h8_sq3": (8, 3), "h128_sq1": (128, 1), "h40_sq2": (40, 2)}
_POOL, _PROBLEM = {}, {}


def pool_of(kind, dt, page=16, nblocks=64):
    key = (kind, dt, page * nblocks)
    if key not in _POOL:
        _POOL[key] = su.make_pool(kind, DTYPES[dt], page * nblocks, 11)
    return _POOL[key]


def problem(kind, dt, heads, sq, topk, b=2, specials=("", "duplicates"), page=16, nblocks=64, seed=0):
    """(problem, oracle), computed once and shared among the split counts."""
    key = (kind, dt, heads, sq, topk, b, specials, page, seed)
    if key not in _PROBLEM:
        p = su.make_problem(kind, DTYPES[dt], heads, sq, topk, b=b, seed=seed + topk, page=page, nblocks=nblocks,
                            specials=specials, pool=pool_of(kind, dt, page, nblocks))
        _PROBLEM[key] = (p, su.oracle(p))
    return _PROBLEM[key]


@pytest.mark.parametrize("num_splits", [1, 3, 0])
@pytest.mark.parametrize("topk", TOPKS)
@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("kind", KINDS)
def test_topk(kind, dt, topk, num_splits, parity_report):
    p, ora = problem(kind, dt, 16, 1, topk)
    o, lse, _, _ = su.run(p, num_splits)
    su.assert_case(f"mla-sparse-{kind}-{dt}-topk{topk}-splits{num_splits}", o.cpu(), lse.cpu(), ora, parity_report)


@pytest.mark.parametrize("num_splits", [1, 3, 0])
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("kind", KINDS)
def test_shapes_and_invalid_patterns(kind, dt, shape, num_splits, parity_report):
    """topk 300 (10 tiles), a batch of 4 whose position 0 holds a whole invalid tile in the middle, a
    whole invalid split range (the second of 3), only invalid entries, and duplicates."""
    h, sq = SHAPES[shape]
    p, ora = problem(kind, dt, h, sq, 300, b=4, specials=su.SPECIALS)
    n = su.num_slots(p)
    ind = p.indices.long()
    assert not su.valid_mask(ind[0, 0, 160:192], n).any() and not su.valid_mask(ind[1, 0, 128:256], n).any()
    assert not su.valid_mask(ind[2, 0], n).any() and p.kx[2 * sq].shape[0] == 0
    o, lse, _, splits = su.run(p, num_splits)
    assert num_splits != 3 or splits == 3
    su.assert_case(f"mla-sparse-{kind}-{dt}-{shape}-splits{num_splits}", o.cpu(), lse.cpu(), ora, parity_report)
    # the all-invalid row: O = 0 and LSE = +inf exactly
    assert (o[2, 0] == 0).all() and (lse[2, :, 0] == float("inf")).all()


@pytest.mark.parametrize("kind", KINDS)
def test_page_64(kind, parity_report):
    """The page size only sets num_slots: 16 blocks of 64 rows are the same 1024 slots."""
    p, ora = problem(kind, "bf16", 8, 3, 65, page=64, nblocks=16)
    for ns in (1, 0):
        o, lse, _, _ = su.run(p, ns)
        su.assert_case(f"mla-sparse-{kind}-page64-splits{ns}", o.cpu(), lse.cpu(), ora, parity_report)


@pytest.mark.parametrize("kind", KINDS)
def test_fill_independence(kind):
    """What lies in the slots no query references - slot 0 among them, which a lane with an invalid
    entry loads - does not reach the outputs: zero, NaN and the largest value give the same bits."""
    p, _ = problem(kind, "bf16", 40, 2, 300, b=4, specials=su.SPECIALS)
    ind = p.indices.clone()
    ind[ind == 0] = 1
    p = su.with_indices(p, ind)                            # no query names slot 0: it is poisoned too
    for ns in (1, 3):
        got = []
        for fill in ("zero", "nan", "big"):
            o, lse, _, _ = su.run(p, ns, fill=fill)
            got.append((o.cpu(), lse.cpu()))
            assert not torch.isnan(got[-1][0]).any() and not torch.isnan(got[-1][1]).any()
        for o, lse in got[1:]:
            assert torch.equal(o, got[0][0]) and torch.equal(lse, got[0][1])


# ------------------------------------------------------------------ bit identities -------
def _dense(kind, c, q, num_splits, n):
    """fmha_mla_decode[_fp8] over the one sequence of c with max_seqlen_k = its length."""
    L = capi.lib()
    b, sq, h, _ = q.shape
    qd, kc, tab = q.to(mu.DEV), c.kc.to(mu.DEV), c.table.to(mu.DEV)
    lens = torch.tensor(c.lens, dtype=torch.int32, device=mu.DEV)
    o = torch.full((b, sq, h, mu.DV), float("nan"), dtype=q.dtype, device=mu.DEV)
    lse = torch.full((b, h, sq), float("nan"), dtype=torch.float32, device=mu.DEV)
    st = (C.c_int64 * 6)(qd.stride(0), qd.stride(1), qd.stride(2), o.stride(0), o.stride(1), o.stride(2))
    fn = L.fmha_mla_decode_fp8 if kind == "fp8" else L.fmha_mla_decode
    fn(qd.data_ptr(), kc.data_ptr(), o.data_ptr(), lse.data_ptr(), tab.data_ptr(), tab.stride(0), lens.data_ptr(),
       sq, n, b, h, mu.D, mu.DV, c.page, st, mu.D ** -0.5, -1, -1, num_splits, q.dtype == torch.float16,
       capi.stream_handle())
    capi.check()
    torch.cuda.synchronize()
    return o, lse, kc, L.fmha_last_num_splits()


@pytest.mark.parametrize("n", [517, 65, 32])
@pytest.mark.parametrize("heads", [16, 128])
@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("kind", KINDS)
def test_equals_the_dense_decode_bit_for_bit(kind, dt, heads, n):
    """indices = the physical slots of a dense sequence in order: same tiles, same order, same split
    ranges, same arithmetic - O and LSE equal fmha_mla_decode[_fp8]'s bit for bit."""
    dtype = DTYPES[dt]
    c = (m8.make_cache8 if kind == "fp8" else mu.make_cache)([n], dtype, seed=n)
    q = mu.make_q(1, 1, heads, mu.D, dtype, n)
    r = torch.arange(n)
    slots = (c.table[0, r // c.page].long() * c.page + r % c.page).int()
    assert not torch.equal(slots.long(), r)                # the table is no identity
    for ns in (1, 3):
        o0, l0, kc, splits0 = _dense(kind, c, q, ns, n)
        p = su.Problem(kind, dtype, None, None, slots.view(1, 1, n), q, None, c.page, kc.shape[0])
        o1, l1, _, splits1 = su.run(p, ns, kc=kc)
        assert splits0 == splits1 == min(ns, (n + 31) // 32)
        assert torch.equal(o0, o1) and torch.equal(l0, l1)


@pytest.mark.parametrize("kind", KINDS)
def test_surfaces_bitwise_equal_and_reproducible(kind):
    """The C ABI, the pybind op and the Python wrapper give the same bits, and so do two calls."""
    import xf_flash_attention_cutlass_amd as xfa
    p, _ = problem(kind, "fp16", 40, 2, 300, b=4, specials=su.SPECIALS)
    kc, qd, ind = su.device_cache(p), p.q.to(mu.DEV), p.indices.to(mu.DEV)
    op = xfa.paged_attn.mla_decode_sparse_fp8 if kind == "fp8" else xfa.paged_attn.mla_decode_sparse
    for ns in (1, 0):
        o0, l0, kern, splits = su.run(p, ns, kc=kc)
        o1, l1, _, _ = su.run(p, ns, kc=kc)
        assert torch.equal(o0, o1) and torch.equal(l0, l1)
        o2, l2 = op(qd, kc, ind, 512, mu.D ** -0.5, ns, None)
        assert capi.lib().fmha_last_num_splits() == splits
        assert capi.lib().fmha_last_kernel().decode() == kern
        o3, l3 = xfa.flash_mla_with_kvcache(qd, kc, None, None, num_splits=ns, indices=ind)
        out = torch.full_like(o0, float("nan"))
        kc4 = kc.view(torch.float8_e4m3fn) if kind == "fp8" else kc
        o4, l4 = xfa.flash_mla_with_kvcache(qd, kc4, None, None, num_splits=ns, out=out, indices=ind)
        assert o4 is out
        for o, l in ((o2, l2), (o3, l3), (o4, l4)):
            assert torch.equal(o, o0) and torch.equal(l, l0)
    with pytest.raises(ValueError, match="causal"):
        xfa.flash_mla_with_kvcache(qd, kc, None, None, causal=True, indices=ind)
    with pytest.raises(RuntimeError, match="int32"):
        xfa.flash_mla_with_kvcache(qd, kc, None, None, indices=ind.long())
    with pytest.raises(RuntimeError, match="batch_size and seqlen_q"):
        xfa.flash_mla_with_kvcache(qd, kc, None, None, indices=ind[:, :1])


@pytest.mark.parametrize("kind", KINDS)
def test_wrapper_without_indices_is_the_dense_path(kind):
    """flash_mla_with_kvcache without `indices` runs the dense kernel and gives its bits."""
    import xf_flash_attention_cutlass_amd as xfa
    dtype = torch.bfloat16
    lens = [300, 65, 0]
    c = (m8.make_cache8 if kind == "fp8" else mu.make_cache)(lens, dtype, seed=3)
    q = mu.make_q(len(lens), 2, 16, mu.D, dtype, 3)
    o0, l0, kern, _ = (m8.run8 if kind == "fp8" else mu.run)(c, q, True, 0)
    o1, l1 = xfa.flash_mla_with_kvcache(q.to(mu.DEV), c.kc.to(mu.DEV), c.table.to(mu.DEV),
                                        torch.tensor(lens, dtype=torch.int32, device=mu.DEV), causal=True)
    assert capi.lib().fmha_last_kernel().decode() == kern and "sparse" not in kern
    assert torch.equal(o0, o1) and torch.equal(l0, l1)


# ------------------------------------------------------------------ as the dense tests ---
@pytest.mark.parametrize("kind", KINDS)
def test_scale(kind, parity_report):
    """softmax_scale = 2 x 576^-1/2 against the oracle over 2 q (exact in bf16)."""
    p, _ = problem(kind, "bf16", 16, 1, 65)
    ora = su.oracle(p, q_mul=2.0)
    o, lse, _, _ = su.run(p, 3, scale=2.0 * mu.D ** -0.5)
    su.assert_case(f"mla-sparse-{kind}-scale2", o.cpu(), lse.cpu(), ora, parity_report)


@pytest.mark.parametrize("kind", KINDS)
def test_strided_views(kind, parity_report):
    """q, o and indices as views inside poisoned arenas (the indices arena names a NaN slot, the
    others hold NaN): the o arena is untouched outside o."""
    p, ora = problem(kind, "bf16", 8, 3, 65)
    b, sq, h, _ = p.q.shape
    topk = p.indices.shape[-1]
    qa = torch.full((b, sq + 1, h + 2, mu.D + 64), float("nan"), dtype=p.dtype, device=mu.DEV)
    qv = qa[:, 1:, 1:h + 1, 64:]
    qv.copy_(p.q)
    oa = torch.full((b, sq + 2, h + 1, mu.DV + 128), float("nan"), dtype=p.dtype, device=mu.DEV)
    ov = oa[:, 1:sq + 1, :h, 64:64 + mu.DV]
    used = torch.zeros(su.num_slots(p), dtype=torch.bool)
    flat = p.indices.reshape(-1).long()
    used[flat[su.valid_mask(flat, su.num_slots(p))]] = True
    unused = int((~used).nonzero()[0])                     # a slot device_cache poisons
    ia = torch.full((b, sq + 1, topk + 5), unused, dtype=torch.int32, device=mu.DEV)
    iv = ia[:, 1:, 3:3 + topk]
    iv.copy_(p.indices)
    assert not qv.is_contiguous() and not ov.is_contiguous() and not iv.is_contiguous()
    for ns in (1, 3):
        ov.fill_(float("nan"))
        o, lse, _, _ = su.run(p, ns, o=ov, qd=qv, ind=iv)
        su.assert_case(f"mla-sparse-{kind}-strided-splits{ns}", ov.cpu(), lse.cpu(), ora, parity_report)
        inside = torch.zeros_like(oa, dtype=torch.bool)
        inside[:, 1:sq + 1, :h, 64:64 + mu.DV] = True
        assert torch.isnan(oa[~inside]).all()
    assert torch.isnan(qa[:, 0]).all()


@pytest.mark.parametrize("kind", KINDS)
def test_no_lse_pointer(kind):
    p, _ = problem(kind, "bf16", 16, 1, 65)
    for ns in (1, 3):
        o0, _, _, _ = su.run(p, ns)
        o1, lse, _, _ = su.run(p, ns, want_lse=False)
        assert lse is None and torch.equal(o0, o1)


@pytest.mark.parametrize("kind", KINDS)
def test_refused_calls_leave_outputs_untouched(kind):
    L = capi.lib()
    p, _ = problem(kind, "bf16", 16, 1, 65)
    b, sq, h, _ = p.q.shape
    qd, kc, ind = p.q.to(mu.DEV), su.device_cache(p), p.indices.to(mu.DEV)
    o = torch.full((b, sq, h, mu.DV), float("nan"), dtype=p.dtype, device=mu.DEV)
    lse = torch.full((b, h, sq), float("nan"), dtype=torch.float32, device=mu.DEV)
    dense = [qd.stride(0), qd.stride(1), qd.stride(2), o.stride(0), o.stride(1), o.stride(2)]
    fn = L.fmha_mla_decode_sparse_fp8 if kind == "fp8" else L.fmha_mla_decode_sparse

    def call(d=mu.D, dv=mu.DV, page=p.page, blocks=p.nblocks, splits=0, indices=ind.data_ptr(), strides=dense,
             topk=65, ind_r=ind.stride(1)):
        st = (C.c_int64 * 6)(*strides)
        fn(qd.data_ptr(), kc.data_ptr(), o.data_ptr(), lse.data_ptr(), indices, ind.stride(0), ind_r, topk, sq, b, h,
           d, dv, blocks, page, st, mu.D ** -0.5, splits, False, capi.stream_handle())
        return L.fmha_last_status(), L.fmha_last_error().decode()

    for kw, needle in ((dict(d=512), "(576, 512) only"), (dict(dv=576), "(576, 512) only"),
                       (dict(page=24), "multiple of 16"), (dict(splits=129), "at most 128"),
                       (dict(indices=None), "indices"), (dict(topk=0), "topk"), (dict(blocks=0), "num_blocks"),
                       (dict(ind_r=-65), "non-negative"), (dict(strides=dense[:5] + [516]), "multiples of 8")):
        st, msg = call(**kw)
        torch.cuda.synchronize()
        assert st != 0 and needle in msg, msg
        assert L.fmha_last_kernel() == b"" and L.fmha_last_num_splits() == 0
        assert torch.isnan(o).all() and torch.isnan(lse).all()
    st, msg = call()
    torch.cuda.synchronize()
    assert st == 0 and not torch.isnan(o).any()


@pytest.mark.parametrize("kind", KINDS)
def test_graph_capture_and_replay(kind):
    """A captured call (after a warm-up: the scratch pool is warm, no allocation and no host sync
    inside the capture), replayed on NaN outputs and on new indices, equals the eager results."""
    import xf_flash_attention_cutlass_amd as xfa
    p, _ = problem(kind, "bf16", 128, 1, 300, b=4, specials=su.SPECIALS)
    p2, _ = problem(kind, "bf16", 128, 1, 300, b=4, specials=su.SPECIALS, seed=5)
    kc, qd = su.device_cache(p._replace(indices=torch.cat([p.indices, p2.indices]))), p.q.to(mu.DEV)
    ind = p.indices.to(mu.DEV)
    out = torch.full((4, 1, 128, mu.DV), float("nan"), dtype=p.dtype, device=mu.DEV)

    def step():
        return xfa.flash_mla_with_kvcache(qd, kc, None, None, out=out, indices=ind)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        o0, l0 = step()
        want = [(o0.clone(), l0.clone())]
        splits = capi.lib().fmha_last_num_splits()
        ind.copy_(p2.indices.to(mu.DEV))
        o0, l0 = step()
        want.append((o0.clone(), l0.clone()))
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert splits > 1 and not torch.equal(want[0][0], want[1][0])
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        _, l1 = step()
    for pi, (wo, wl) in zip((p, p2), want):
        ind.copy_(pi.indices.to(mu.DEV))
        out.fill_(float("nan"))
        l1.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, wo) and torch.equal(l1, wl)


@pytest.mark.parametrize("kind", KINDS)
def test_merge_with_a_dense_partial(kind, parity_report):
    """A sparse partial over selected slots and a dense partial over other keys (a 16-bit cache of its
    own), merged by merge_attn_states as two 256-column halves, against the oracle over the union."""
    import xf_flash_attention_cutlass_amd as xfa
    dt = torch.bfloat16
    p, _ = problem(kind, "bf16", 16, 1, 65)
    lens = [77, 33]
    dense = mu.make_cache(lens, dt, seed=9)
    o_s, l_s, _, _ = su.run(p, 3)
    o_d, l_d, _, _ = mu.run(dense, p.q, False, 3)
    out = torch.full_like(o_s, float("nan"))
    lse_out = None
    for lo in (0, 256):
        _, lse_out = xfa.merge_attn_states([o_s[..., lo:lo + 256], o_d[..., lo:lo + 256]], [l_s, l_d],
                                           out=out[..., lo:lo + 256])
    union = su.Keys([torch.cat([p.kx[i], dense.kx[i]]) for i in range(len(lens))])
    ora = mu.oracle(union, su.flat_q(p.q), False)
    su.assert_case(f"mla-sparse-{kind}-merge-dense", out.cpu(), lse_out.cpu(), ora, parity_report)


@pytest.mark.parametrize("kind", KINDS)
def test_cache_beyond_4_gib(kind, parity_report):
    """A cache of just over 4 GiB, only the referenced rows written: indices in its first and in its
    last page (slot-to-byte arithmetic in 64 bits).  Skips below 8 GiB of free device memory."""
    free = torch.cuda.mem_get_info()[0]
    if free < 8 << 30:
        print(f"test_cache_beyond_4_gib: skipped, {free >> 20} MiB of device memory free (needs 8192)")
        pytest.skip("less than 8 GiB of device memory free")
    dtype = torch.bfloat16
    row = 656 if kind == "fp8" else 576 * 2
    page = 16
    nblocks = (1 << 32) // (page * row) + 2
    nslots = nblocks * page
    assert nslots * row > (1 << 32) and (nslots - 1) * row > (1 << 32)
    rows, kx_pool = su.make_pool(kind, dtype, 32, 77)      # the 32 referenced rows
    where = torch.cat([torch.arange(16), torch.arange(nslots - 16, nslots)])
    gen = torch.Generator().manual_seed(4)
    pick = torch.cat([torch.randperm(32, generator=gen), torch.tensor([31])])      # 33 entries, one twice
    ind = where[pick].clone()
    ind[5], ind[20] = -1, nslots                           # two invalid places
    kc = torch.empty((nblocks, page, 1, rows.shape[-1]), dtype=rows.dtype, device=mu.DEV)
    kc.view(nslots, -1)[where.to(mu.DEV)] = rows.to(mu.DEV)
    ok = su.valid_mask(ind, nslots)
    q = mu.make_q(1, 1, 16, mu.D, dtype, 77)
    p = su.Problem(kind, dtype, None, None, ind.int().view(1, 1, 33), q, [kx_pool[pick[ok]][:, None]], page, nblocks)
    ora = su.oracle(p)
    for ns in (1, 2):
        o, lse, _, _ = su.run(p, ns, kc=kc)
        su.assert_case(f"mla-sparse-{kind}-4gib-splits{ns}", o.cpu(), lse.cpu(), ora, parity_report)
    del kc
    torch.cuda.empty_cache()
