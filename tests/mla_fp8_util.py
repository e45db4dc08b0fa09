"""Shared helpers of the fp8 MLA cache tests (not a conftest: imported explicitly).

The fp8 latent cache (include/paged_attn.h, 2.10) stores a token in 656 bytes: 512 e4m3fn latent
features, four fp32 descales (one per 128 features), the 64 rotary features in q's dtype.

* `quantize_ref`, `pack_rows`, `unpack_rows`: a torch restatement of the append's quantiser and of
  the row.
* `operand`: the rows the decode is defined over - feature i < 512 is T(float(e4m3[i]) *
  descale[i / 128]), one fp32 product rounded once to q's dtype T; the rest as stored - with the
  defects of DEFECTS plantable (what a wrong kernel would make of the same bytes).
* `make_rows`: inputs whose 128-feature groups differ (with unit-randn rows all four descales of a
  row are nearly equal and a kernel that swaps them would pass).
* `build_cache8`: per-sequence rows -> a paged byte cache behind a random, non-identity block table
  (the layout of `decode_util.build_cache`: a poison page behind every table entry past a
  sequence's end, two pages no entry names), every byte outside the sequences a chosen fill.  Its
  `kx` are the operand rows, so `mla_util.oracle`, `judge_each` and `assert_case` apply unchanged.
* `as_cache16`: the operand (or a defective one) as a 16-bit `decode_util` cache, for
  `mla_util.emulate`.
* `run8`: fmha_mla_decode_fp8 through the C ABI into NaN-filled outputs; asserts kernel and mapping.
"""
from __future__ import annotations

import ctypes as C
from collections import namedtuple

import torch

from tests import mla_util as mu
from tests.decode_util import DEV, build_cache

ROW = 656
GROUPS, GROUP = 4, 128
F8 = torch.float8_e4m3fn
DEFECTS = ("descale_swap_1_2", "descale_ignored", "descale_prev_row", "descale_0_for_all", "rope_shift_16B")
FILL_BYTES = {"zero": 0x00, "nan": 0xFF, "big": 0x7E}      # 0xFF is NaN as e4m3fn, bf16, fp16 and fp32

Cache8 = namedtuple("Cache8", "kc table lens page width dtype kx rows poison")


# ---------------------------------------------------------------- quantiser and row ------
def quantize_ref(latent):
    """latent [n, 512] (bf16 / fp16) -> (bytes uint8 [n, 512], descale fp32 [n, 4]) as the header
    states the append: per 128-feature group amax = max |float(x)|, descale = amax / 448 in fp32
    (1.0 where amax == 0), byte = e4m3fn(clamp(float(x) * (1 / descale), -448, 448))."""
    x = latent.float().reshape(-1, GROUPS, GROUP)
    amax = x.abs().amax(-1)
    ds = torch.where(amax == 0, torch.ones_like(amax), amax / 448.0)
    b8 = (x * (1 / ds)[..., None]).clamp(-448.0, 448.0).to(F8)
    return b8.view(torch.uint8).reshape(-1, GROUPS * GROUP), ds


def pack_rows(b8, ds, rope):
    """(uint8 [n, 512], fp32 [n, 4], bf16 / fp16 [n, 64]) -> uint8 [n, 656]."""
    n = b8.shape[0]
    rows = torch.empty(n, ROW, dtype=torch.uint8)
    rows[:, :512] = b8
    rows[:, 512:528] = ds.contiguous().view(torch.uint8).reshape(n, 16)
    rows[:, 528:] = rope.contiguous().view(torch.uint8).reshape(n, 128)
    return rows


def unpack_rows(rows, dtype):
    """uint8 [n, 656] -> (uint8 [n, 512], fp32 [n, 4], dtype [n, 64])."""
    rows = rows.contiguous()
    n = rows.shape[0]
    return (rows[:, :512].clone(), rows[:, 512:528].contiguous().view(torch.float32).reshape(n, 4).clone(),
            rows[:, 528:].contiguous().view(dtype).reshape(n, 64).clone())


def rows_of(x, dtype):
    """float [n, 576] -> the packed rows of x rounded to dtype (what the append writes)."""
    xt = x.to(dtype)
    b8, ds = quantize_ref(xt[:, :512])
    return pack_rows(b8, ds, xt[:, 512:])


def operand(rows, dtype, defect=None):
    """uint8 [n, 656] -> float32 [n, 576], every value exact in dtype: the rows the decode attends
    over, or what one of DEFECTS makes of the same bytes."""
    assert defect is None or defect in DEFECTS
    b8, ds, rope = unpack_rows(rows, dtype)
    if defect == "descale_swap_1_2":
        ds = ds[:, [0, 2, 1, 3]]
    elif defect == "descale_ignored":
        ds = torch.ones_like(ds)
    elif defect == "descale_prev_row":
        ds = ds.roll(1, 0)
    elif defect == "descale_0_for_all":
        ds = ds[:, [0, 0, 0, 0]]
    elif defect == "rope_shift_16B":
        rope = rope.roll(8, 1)
    lat = (b8.view(F8).float().reshape(-1, GROUPS, GROUP) * ds[..., None]).to(dtype)
    return torch.cat([lat.reshape(-1, 512).float(), rope.float()], -1)


def make_rows(n, gen):
    """float [n, 576]: unit randn with features 128-255 x 1/16, 256-383 x 8 and, in the second half
    of the rows, the first group x 4 - the four descales of a row differ, and so do the rows'."""
    x = torch.randn(n, mu.D, generator=gen)
    x[:, 128:256] *= 1 / 16
    x[:, 256:384] *= 8
    x[n // 2:, :128] *= 4
    return x


# ---------------------------------------------------------------- the cache --------------
def build_cache8(seqs, page, width, dtype, fill="nan", seed=0) -> Cache8:
    """seqs: per-sequence float [n_b, 576] (n_b may be 0)."""
    assert page % 16 == 0
    lens = [s.shape[0] for s in seqs]
    used = [(n + page - 1) // page for n in lens]
    assert max(used) <= width
    npages = sum(used) + 3
    perm = torch.randperm(npages, generator=torch.Generator().manual_seed(1000 + seed))
    if torch.equal(perm, torch.arange(npages)):
        perm = perm.roll(1)
    poison = int(perm[sum(used)])
    table = torch.full((len(seqs), width), poison, dtype=torch.int32)
    kc = torch.full((npages, page, 1, ROW), FILL_BYTES[fill], dtype=torch.uint8)
    kx, rows, nxt = [], [], 0
    for i, s in enumerate(seqs):
        table[i, :used[i]] = perm[nxt:nxt + used[i]].int()
        nxt += used[i]
        rw = rows_of(s, dtype)
        r = torch.arange(lens[i])
        kc[table[i, r // page].long(), r % page, 0] = rw
        rows.append(rw)
        kx.append(operand(rw, dtype)[:, None])
    return Cache8(kc, table, lens, page, width, dtype, kx, rows, poison)


def make_cache8(lens, dtype, fill="nan", seed=0, page=mu.PAGE, width=None):
    gen = torch.Generator().manual_seed(500 + seed)
    return build_cache8([make_rows(n, gen) for n in lens], page, width or 1024 // page, dtype, fill, seed)


def as_cache16(c: Cache8, defect=None):
    """The operand of c (or what `defect` makes of its bytes) as a 16-bit decode_util cache."""
    ks = [operand(rw, c.dtype, defect)[:, None] for rw in c.rows]
    return build_cache(ks, ks, c.page, c.width, False, c.dtype, "nan", seed=1)


# ---------------------------------------------------------------- the launch -------------
def run8(c: Cache8, q, causal=False, num_splits=0, scale=None, o=None, lse=None, qd=None, want_lse=True, kc=None):
    """One fmha_mla_decode_fp8 call on a device copy of the cache (or on `kc`, a device cache).
    Returns (o, lse, kernel, splits); asserts the kernel, its mapping, its grid and the splits."""
    from xf_flash_attention_cutlass_amd import capi
    L = capi.lib()
    b, sq, h, d = q.shape
    qd = q.to(DEV) if qd is None else qd
    kc = c.kc.to(DEV) if kc is None else kc
    tab = c.table.to(DEV)
    lens = torch.tensor(c.lens, dtype=torch.int32).to(DEV)
    if o is None:
        o = torch.full((b, sq, h, mu.DV), float("nan"), dtype=q.dtype, device=DEV)
    if lse is None and want_lse:
        lse = torch.full((b, h, sq), float("nan"), dtype=torch.float32, device=DEV)
    st = (C.c_int64 * 6)(qd.stride(0), qd.stride(1), qd.stride(2), o.stride(0), o.stride(1), o.stride(2))
    L.fmha_mla_decode_fp8(qd.data_ptr(), kc.data_ptr(), o.data_ptr(), capi.ptr(lse), tab.data_ptr(),
                          tab.stride(0), lens.data_ptr(), sq, c.width * c.page, b, h, mu.D, mu.DV, c.page, st,
                          mu.D ** -0.5 if scale is None else scale, -1, 0 if causal else -1, num_splits,
                          q.dtype == torch.float16, capi.stream_handle())
    capi.check()
    torch.cuda.synchronize()
    kern, splits = L.fmha_last_kernel().decode(), L.fmha_last_num_splits()
    tiles = (sq * h + 15) // 16
    want = "fmha_mla_decode_fp8_kernel<%s>" % ("tiles" if tiles > 1 else "splits")
    assert kern.startswith(want), f"ran {kern!r}, wanted {want!r}"
    assert "grid=%dx1x1 block=256" % ((b * splits * tiles + 3) // 4) in kern, kern
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert splits == mu.expected_splits(num_splits, b, tiles, c.width * c.page, cus), (splits, num_splits)
    return o, lse, kern, splits
