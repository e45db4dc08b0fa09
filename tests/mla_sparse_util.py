"""Shared helpers of the sparse MLA decode tests (not a conftest: imported explicitly).

The sparse decode (include/paged_attn.h, 2.11) attends, for query (batch, pos), over the cache rows
at the valid entries of indices[batch, pos, :] - physical slots, valid iff 0 <= entry < num_slots.
Each (batch, pos) is therefore its own one-position sequence whose keys are those rows, and
`mla_util.oracle` / `judge_each` / `assert_case` and the fp8 operand of `mla_fp8_util` apply
unchanged to the flattened problem.

* `make_pool`: the cache as [num_slots] rows - randn in q's dtype ("kv16") or 2.10's group-scaled
  inputs packed into 656-byte rows ("fp8") - with the exact operand rows the decode is defined over.
* `make_indices`: a random index set per (batch, pos), with invalid values sprinkled in, and the
  special rows of SPECIALS.
* `Problem` / `make_problem`: pool + indices + q + the flattened pseudo-sequences (`kx`); `device_cache`
  poisons every slot no query references.
* `flat` / `flat_q`: [b, sq, h, x] and [b, h, sq] outputs as b * sq one-position sequences.
* `emulate`: a correct sparse split decode on the CPU (32-entry tiles, equal split ranges, fp32
  accumulation, P rounded to q's dtype, invalid rows zeroed and scored -inf, the combine), with the
  defects of DEFECTS plantable.
* `run`: fmha_mla_decode_sparse[_fp8] through the C ABI into NaN-filled outputs; asserts the kernel,
  its mapping, its grid and the split count.
"""
from __future__ import annotations

import ctypes as C
from collections import namedtuple

import torch

from tests import mla_fp8_util as m8
from tests import mla_util as mu
from tests.decode_util import DEV

D, DV = mu.D, mu.DV
TILE = 32
INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31
DEFECTS = ("prev_pos", "invalid_as_slot0", "dup_once", "logical_slots", "tail_next_row", "reset_max")
# rows of the batch with a structure of their own (make_indices): a whole tile invalid in the middle,
# a whole split range invalid (of 3), every entry invalid, and duplicates
SPECIALS = ("tile_invalid", "split_invalid", "all_invalid", "duplicates")

Problem = namedtuple("Problem", "kind dtype rows kx_pool indices q kx page nblocks")
Keys = namedtuple("Keys", "kx")


def num_slots(p):
    return p.nblocks * p.page


# ---------------------------------------------------------------- the cache --------------
def make_pool(kind, dtype, nslots, seed):
    """(stored rows, operand rows float32 [nslots, 576]): "kv16" - randn rounded to dtype, stored as
    such; "fp8" - `mla_fp8_util.make_rows` packed into uint8 [nslots, 656], the operand its
    dequantised rows rounded to dtype."""
    gen = torch.Generator().manual_seed(900 + seed)
    if kind == "fp8":
        rows = m8.rows_of(m8.make_rows(nslots, gen), dtype)
        return rows, m8.operand(rows, dtype)
    st = torch.randn(nslots, D, generator=gen).to(dtype)
    return st, st.float()


def valid_mask(idx, nslots):
    return (idx >= 0) & (idx < nslots)


def make_indices(b, sq, topk, nslots, seed, invalid=0.1, specials=()):
    """int32 [b, sq, topk]: every (batch, pos) draws its own random slots (with repeats possible
    only through `duplicates`), a fraction `invalid` of the places replaced by -1, nslots, INT32_MAX
    or INT32_MIN.  specials[i] shapes (batch i, pos 0)."""
    gen = torch.Generator().manual_seed(1300 + seed)
    idx = torch.empty(b, sq, topk, dtype=torch.int64)
    for i in range(b):
        for s in range(sq):
            if topk <= nslots:
                idx[i, s] = torch.randperm(nslots, generator=gen)[:topk]
            else:
                idx[i, s] = torch.randint(0, nslots, (topk,), generator=gen)
    bad = torch.tensor([-1, nslots, INT_MAX, INT_MIN])
    hit = torch.rand(b, sq, topk, generator=gen) < invalid
    idx = torch.where(hit, bad[torch.randint(0, 4, (b, sq, topk), generator=gen)], idx)
    tiles = (topk + TILE - 1) // TILE
    for i, kind in enumerate(specials):
        if kind == "tile_invalid" and tiles >= 3:
            t = tiles // 2
            idx[i, 0, t * TILE:(t + 1) * TILE] = -1
        elif kind == "split_invalid" and tiles >= 3:
            per = (tiles + 2) // 3
            idx[i, 0, per * TILE:2 * per * TILE] = bad[torch.arange(min(topk, 2 * per * TILE) - per * TILE) % 4]
        elif kind == "all_invalid":
            idx[i, 0] = bad[torch.arange(topk) % 4]
        elif kind == "duplicates" and topk >= 4:
            src = torch.randint(0, topk, (topk // 3,), generator=gen)
            dst = torch.randint(0, topk, (topk // 3,), generator=gen)
            idx[i, 0, dst] = idx[i, 0, src]
    return idx.to(torch.int32)


def keys_of(kx_pool, indices, nslots):
    """The pseudo-sequences: for each flattened (batch, pos) the operand rows at its valid entries,
    in order, as [n, 1, 576]."""
    flat = indices.reshape(-1, indices.shape[-1]).long()
    return [kx_pool[r[valid_mask(r, nslots)]][:, None] for r in flat]


def make_problem(kind, dtype, heads, sq, topk, b=2, seed=0, page=16, nblocks=64, invalid=0.1, specials=(),
                 pool=None) -> Problem:
    nslots = page * nblocks
    rows, kx_pool = pool if pool is not None else make_pool(kind, dtype, nslots, seed)
    indices = make_indices(b, sq, topk, nslots, seed, invalid, specials)
    q = mu.make_q(b, sq, heads, D, dtype, 40 + seed)
    return Problem(kind, dtype, rows, kx_pool, indices, q, keys_of(kx_pool, indices, nslots), page, nblocks)


def with_indices(p: Problem, indices) -> Problem:
    return p._replace(indices=indices, kx=keys_of(p.kx_pool, indices, num_slots(p)))


def flat_q(q):
    b, sq, h, d = q.shape
    return q.reshape(b * sq, 1, h, d)


def flat(o, lse):
    """Outputs [b, sq, h, 512] and [b, h, sq] as b * sq one-position sequences."""
    b, sq, h, d = o.shape
    return o.reshape(b * sq, 1, h, d), lse.permute(0, 2, 1).reshape(b * sq, h, 1)


def oracle(p: Problem, q_mul=1.0):
    return mu.oracle(Keys(p.kx), flat_q(p.q), False, q_mul)


def judge_each(o, lse, ora):
    return mu.judge_each(*flat(o, lse), ora)


def assert_case(name, o, lse, ora, report=None):
    return mu.assert_case(name, *flat(o, lse), ora, report)


FILLS16 = {"zero": 0.0, "nan": float("nan"), "big": None}


def device_cache(p: Problem, fill="nan", indices=None):
    """The cache [nblocks, page, 1, 576 | 656] on the device, every slot that no query references set
    to `fill` (16-bit: 0 / NaN / the dtype's maximum; fp8: the bytes 0x00 / 0xFF / 0x7E)."""
    idx = (p.indices if indices is None else indices).reshape(-1).long()
    used = torch.zeros(num_slots(p), dtype=torch.bool)
    used[idx[valid_mask(idx, num_slots(p))]] = True
    rows = p.rows.clone()
    if p.kind == "fp8":
        rows[~used] = m8.FILL_BYTES[fill]
    else:
        rows[~used] = torch.finfo(p.dtype).max if fill == "big" else FILLS16[fill]
    return rows.reshape(p.nblocks, p.page, 1, rows.shape[-1]).to(DEV)


# ---------------------------------------------------------------- the CPU model ----------
def emulate(p: Problem, splits, defect=None, table=None):
    """A correct sparse split decode on the CPU, or one with a planted defect:
    prev_pos: the previous position's indices (of the flattened batch) used; invalid_as_slot0: an
    invalid entry read as slot 0 instead of being dropped; dup_once: a slot counted once however often
    it occurs; logical_slots: entries taken as logical positions through the block table `table`
    (slot = table[entry / page] * page + entry % page); tail_next_row: places at or beyond topk in the
    last tile taken from the next row of `indices`; reset_max: a tile without a valid entry resets
    the running maximum.  Returns (o [b, sq, h, 512], lse [b, h, sq])."""
    assert defect is None or defect in DEFECTS
    b, sq, h, _ = p.q.shape
    topk, nslots = p.indices.shape[-1], num_slots(p)
    rowsf = p.indices.reshape(b * sq, topk).long()
    tiles = (topk + TILE - 1) // TILE
    pad = tiles * TILE - topk
    scale = D ** -0.5
    o = torch.zeros(b * sq, h, DV, dtype=p.dtype)
    lse = torch.full((b * sq, h), float("inf"), dtype=torch.float32)
    for r in range(b * sq):
        src = rowsf[(r - 1) % (b * sq)] if defect == "prev_pos" else rowsf[r]
        ext = rowsf[(r + 1) % (b * sq)][:pad] if defect == "tail_next_row" else torch.full((pad,), -1)
        ent = torch.cat([src, ext])
        if defect == "logical_slots":
            okl = valid_mask(ent, nslots)
            e = ent.clamp(0, nslots - 1)
            ent = torch.where(okl, table[e // p.page].long() * p.page + e % p.page, ent)
        ok = valid_mask(ent, nslots)
        if defect == "invalid_as_slot0":
            ok = ok | (torch.arange(len(ent)) < topk)
        slot = torch.where(valid_mask(ent, nslots), ent, torch.zeros_like(ent))
        if defect == "dup_once":
            seen = set()
            for j in range(len(ent)):
                if ok[j]:
                    if int(slot[j]) in seen:
                        ok[j] = False
                    seen.add(int(slot[j]))
        qf = p.q.reshape(b * sq, h, D)[r].float()                      # [h, 576]
        per = (tiles + splits - 1) // splits
        parts_o, parts_l = [], []
        for s in range(splits):
            t_lo = min(tiles, s * per)
            t_hi = min(tiles, t_lo + per)
            m_run = torch.full((h,), float("-inf"))
            l_run = torch.zeros(h)
            acc = torch.zeros(h, DV)
            for t in range(t_lo, t_hi):
                sl = slice(t * TILE, (t + 1) * TILE)
                okt = ok[sl]
                kt = torch.where(okt[:, None], p.kx_pool[slot[sl]], torch.tensor(0.0))     # [32, 576]
                st = (qf @ kt.T) * scale
                st = torch.where(okt[None], st, torch.tensor(float("-inf")))
                if defect == "reset_max" and not okt.any():
                    m_run = torch.full((h,), float("-inf"))
                    continue
                m_new = torch.maximum(m_run, st.amax(-1))
                mref = torch.where(torch.isneginf(m_new), torch.zeros_like(m_new), m_new)
                alpha = torch.exp(m_run - mref)
                pr = torch.exp(st - mref[:, None])
                l_run = l_run * alpha + pr.sum(-1)
                acc = acc * alpha[:, None] + pr.to(p.dtype).float() @ kt[:, :DV]
                m_run = m_new
            empty = (l_run == 0) | torch.isnan(l_run)
            inv = torch.where(empty, torch.zeros_like(l_run), 1.0 / l_run)
            parts_o.append(acc * inv[:, None])
            parts_l.append(torch.where(empty, torch.tensor(float("-inf")), m_run + torch.log(l_run)))
        po, pl = torch.stack(parts_o), torch.stack(parts_l)
        mx = pl.amax(0)
        mx0 = torch.where(torch.isneginf(mx), torch.zeros_like(mx), mx)
        sm = torch.where(torch.isneginf(mx), torch.zeros_like(mx), torch.exp(pl - mx0).sum(0))
        rempty = torch.isneginf(mx) | (sm == 0)
        ls = torch.where(rempty, torch.tensor(float("inf")), torch.log(sm) + mx0)
        w = torch.where(rempty[None], torch.zeros_like(pl), torch.exp(pl - ls[None]))
        o[r] = (w[..., None] * po).sum(0).to(p.dtype)
        lse[r] = ls
    return o.reshape(b, sq, h, DV), lse.reshape(b, sq, h).permute(0, 2, 1).contiguous()


# ---------------------------------------------------------------- the launch -------------
def row_tiles(sq, h):
    return sq * ((h + 15) // 16)


def expected_splits(num_splits, batch, tiles, topk, num_cus):
    """The host's split count: fmha_mla_decode's rule with the index tiles for the key tiles."""
    return mu.expected_splits(num_splits, batch, tiles, topk, num_cus)


def run(p: Problem, num_splits=0, scale=None, o=None, lse=None, qd=None, ind=None, kc=None, fill="nan",
        want_lse=True):
    """One fmha_mla_decode_sparse[_fp8] call on `device_cache(p, fill)` (or `kc`).  o / lse / qd /
    ind: device tensors to use (views are fine); else NaN-filled outputs are made.  Returns
    (o, lse, kernel, splits)."""
    from xf_flash_attention_cutlass_amd import capi
    L = capi.lib()
    b, sq, h, _ = p.q.shape
    qd = p.q.to(DEV) if qd is None else qd
    kc = device_cache(p, fill) if kc is None else kc
    ind = p.indices.to(DEV) if ind is None else ind
    topk = ind.shape[-1]
    if o is None:
        o = torch.full((b, sq, h, DV), float("nan"), dtype=p.dtype, device=DEV)
    if lse is None and want_lse:
        lse = torch.full((b, h, sq), float("nan"), dtype=torch.float32, device=DEV)
    st = (C.c_int64 * 6)(qd.stride(0), qd.stride(1), qd.stride(2), o.stride(0), o.stride(1), o.stride(2))
    fn = L.fmha_mla_decode_sparse_fp8 if p.kind == "fp8" else L.fmha_mla_decode_sparse
    fn(qd.data_ptr(), kc.data_ptr(), o.data_ptr(), capi.ptr(lse), ind.data_ptr(), ind.stride(0), ind.stride(1),
       topk, sq, b, h, D, DV, kc.shape[0], kc.shape[1], st, D ** -0.5 if scale is None else scale, num_splits,
       p.dtype == torch.float16, capi.stream_handle())
    capi.check()
    torch.cuda.synchronize()
    kern, splits = L.fmha_last_kernel().decode(), L.fmha_last_num_splits()
    tiles = row_tiles(sq, h)
    want = "fmha_mla_decode_sparse_%skernel<%s>" % ("fp8_" if p.kind == "fp8" else "", "tiles" if tiles > 1 else "splits")
    assert kern.startswith(want), f"ran {kern!r}, wanted {want!r}"
    assert "grid=%dx1x1 block=256" % ((b * splits * tiles + 3) // 4) in kern, kern
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert splits == expected_splits(num_splits, b, tiles, topk, cus), (splits, num_splits)
    return o, lse, kern, splits
