"""Multi-GPU sharding of the attention hot path (one process per GPU, torch.distributed).

The reference has no distributed code (no NCCL/RCCL call sites).  Attention has
no reduction across (batch, head) units in the forward, so the units are partitioned across
ranks and every rank runs the single-GPU kernels on its shard with NO collective in the data
path; the only exchange is an optional all-gather (RCCL over xGMI on MI355X, `nccl` backend =
RCCL) that assembles the sharded outputs on every rank:

  * dense fwd/bwd (C2/C3)  : shard heads in contiguous, GQA-aligned ranges (a K/V head and all
                             query heads that read it stay on one rank, so dK/dV need no
                             cross-rank reduction); batch shards when there are fewer kv heads
                             than ranks (then every rank needs at least one batch element);
  * varlen (C4)            : shard whole sequences, greedy-balanced on sum(s_q * s_k);
  * paged decode (C5)      : shard the batch; every rank owns its sequences' pages, no KV moves.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, List, Sequence, Tuple

import torch


@dataclass(frozen=True)
class Shard:
    start: int
    stop: int

    @property
    def size(self) -> int:
        return self.stop - self.start


def even_ranges(n: int, world: int) -> List[Shard]:
    """Split range(n) into `world` contiguous chunks whose sizes differ by at most one."""
    base, rem = divmod(n, world)
    out, s = [], 0
    for r in range(world):
        e = s + base + (1 if r < rem else 0)
        out.append(Shard(s, e))
        s = e
    return out


def head_shards(num_heads: int, num_heads_k: int, world: int) -> List[Tuple[Shard, Shard]]:
    """GQA-aligned head ranges: rank r gets kv heads [a, b) and query heads [a*G, b*G)."""
    if num_heads % num_heads_k:
        raise ValueError("num_heads must be a multiple of num_heads_k")
    if num_heads_k < world:
        raise ValueError(f"cannot shard {num_heads_k} kv heads over {world} ranks; use batch shards")
    g = num_heads // num_heads_k
    return [(Shard(s.start * g, s.stop * g), s) for s in even_ranges(num_heads_k, world)]


def balanced_sequences(seqlens_q: Sequence[int], seqlens_k: Sequence[int], world: int) -> List[List[int]]:
    """Greedy longest-processing-time assignment of whole sequences on cost s_q * s_k."""
    cost = [int(a) * int(b) for a, b in zip(seqlens_q, seqlens_k)]
    order = sorted(range(len(cost)), key=lambda i: -cost[i])
    load = [0] * world
    parts: List[List[int]] = [[] for _ in range(world)]
    for i in order:
        r = min(range(world), key=lambda j: (load[j], j))
        parts[r].append(i)
        load[r] += cost[i]
    return [sorted(p) for p in parts]


def _world():
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        return dist, dist.get_rank(), dist.get_world_size()
    return None, 0, 1


def all_gather_heads(local: torch.Tensor, shards: List[Tuple[Shard, Shard]], head_dim: int = 2):
    """Assemble [b, s, H, d] from per-rank head shards [b, s, H_r, d] (all ranks get the full
    tensor)."""
    return all_gather_dim(local, [q.size for q, _ in shards], head_dim)


def _slice_alibi(alibi, heads: Shard | None = None, batch: Shard | None = None):
    """ALiBi slopes ([H] or [b, H]) restricted to a rank's query heads / batch rows."""
    if alibi is None:
        return None
    if heads is not None:
        alibi = alibi[..., heads.start:heads.stop]
    if batch is not None and alibi.dim() == 2:
        alibi = alibi[batch.start:batch.stop]
    return alibi.contiguous()


def _gather_dim_impl(local: torch.Tensor, sizes: Sequence[int], dim: int, dist, world: int):
    """The collective itself (world > 1).  Even shards: along dim 0 one all_gather_into_tensor
    whose rank-major buffer IS the result; along another dim (head shards) the rank-major
    buffer is moved to `dim` with one copy.  Uneven shards pad to the largest piece along `dim`
    and drop the padding afterwards."""
    local = local.contiguous()
    nmax = max(sizes)
    shape = list(local.shape)
    if min(sizes) == nmax:
        gathered = local.new_empty([world * shape[0]] + shape[1:])   # rank-major along dim 0
        dist.all_gather_into_tensor(gathered, local)
        if dim == 0:
            return gathered
        # [world, *shape] -> pieces side by side along dim
        g = gathered.view([world] + shape).movedim(0, dim)
        return g.reshape(shape[:dim] + [world * nmax] + shape[dim + 1:])
    shape[dim] = nmax
    buf = local.new_zeros(shape)
    buf.narrow(dim, 0, local.shape[dim]).copy_(local)
    gathered = local.new_empty([world * shape[0]] + shape[1:])
    dist.all_gather_into_tensor(gathered, buf)
    gathered = gathered.view([world] + shape)
    return torch.cat([gathered[r].narrow(dim, 0, sizes[r]) for r in range(world)], dim=dim)


class _AllGatherDim(torch.autograd.Function):
    """All-gather along `dim` whose backward hands each rank the gradient of its own piece.

    Every rank holds the whole gathered output and (data-parallel replicas of one step) computes
    the same loss from it, so d loss / d (my piece) is the slice of d loss / d out at my offset:
    the backward is a narrow, with no communication."""

    @staticmethod
    def forward(ctx, local, sizes, dim, rank):
        dist, _, world = _world()
        ctx.dim, ctx.start, ctx.size = dim, sum(sizes[:rank]), sizes[rank]
        return _gather_dim_impl(local, sizes, dim, dist, world)

    @staticmethod
    def backward(ctx, grad):
        return grad.narrow(ctx.dim, ctx.start, ctx.size), None, None, None


def all_gather_dim(local: torch.Tensor, sizes: Sequence[int], dim: int):
    """Concatenate per-rank pieces along `dim` (rank r holds sizes[r] entries) on every rank.
    Differentiable (`_AllGatherDim`): the backward narrows the output gradient to this rank's
    piece.  World size 1 runs no collective: the local piece is the result.

    That backward assumes every rank computes the same loss from the gathered tensor, so the
    gradient a rank gets for anything upstream of `local` covers its own piece only: gradients of
    replicated inputs and parameters need a SUM all-reduce over the ranks (not DDP's average, and
    not nothing) before they are used."""
    dist, rank, world = _world()
    if world == 1:
        return local
    return _AllGatherDim.apply(local, list(sizes), dim, rank)


def sharded_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                      local_fn: Callable | None = None, gather: bool = True,
                      prefer: str = "heads", **kw):
    """Dense attention sharded over ranks: every rank holds the full (replicated) q/k/v views,
    computes its GQA-aligned query-head range with `local_fn` (default: the gfx950 kernels)
    and, if `gather`, all-gathers the outputs.  With fewer kv heads than ranks, or with
    prefer="batch" and a batch the world divides (whose gather along dim 0 needs no copy), the
    batch is sharded instead.  ALiBi slopes in `kw` are sliced to the rank's heads / batch rows.
    Returns (out, my shard): a query-head range or a batch range (see `attention_shards`).

    Gradients: the gather's backward hands each rank the gradient of its own shard, so what a
    rank gets for the replicated q / k / v (and for the parameters behind them) is its shard's
    part only and needs a SUM all-reduce over the ranks (see `all_gather_dim`)."""
    dist, rank, world = _world()
    if local_fn is None:
        from . import flash_attn_func as local_fn
    kind, shards = attention_shards(q.shape[0], q.shape[2], k.shape[2], world, prefer)
    alibi = kw.pop("alibi_slopes", None)
    if kind == "heads":
        qs, ks = shards[rank]
        if alibi is not None:
            kw["alibi_slopes"] = _slice_alibi(alibi, heads=qs)
        # head-sliced views go to the kernels as they are (fmha_fwd_strided): no copies
        out_local = local_fn(q[:, :, qs.start:qs.stop], k[:, :, ks.start:ks.stop],
                             v[:, :, ks.start:ks.stop], **kw)
        if not gather:
            return out_local, qs
        return all_gather_dim(out_local, [a.size for a, _ in shards], 2), qs
    bs = shards[rank]
    if alibi is not None:
        kw["alibi_slopes"] = _slice_alibi(alibi, batch=bs)
    out_local = local_fn(q[bs.start:bs.stop], k[bs.start:bs.stop], v[bs.start:bs.stop], **kw)
    if not gather:
        return out_local, bs
    return all_gather_dim(out_local, [s.size for s in shards], 0), bs


def attention_shards(batch: int, num_heads: int, num_heads_k: int, world: int,
                     prefer: str = "heads"):
    """("heads", [(q heads, kv heads)] per rank) when every rank gets at least one kv head
    (unless prefer="batch" and world divides the batch), else ("batch", [batch range] per
    rank)."""
    if prefer not in ("heads", "batch"):
        raise ValueError(f"prefer must be 'heads' or 'batch' (got {prefer!r})")
    if prefer == "batch" and batch % world == 0:
        return "batch", batch_shards(batch, world)
    if num_heads_k >= world:
        return "heads", head_shards(num_heads, num_heads_k, world)
    if batch < world:
        raise ValueError(f"cannot shard {num_heads_k} kv heads or {batch} batch rows over {world} ranks")
    return "batch", batch_shards(batch, world)


@dataclass(frozen=True)
class VarlenPlan:
    """Sequence shards of one packed varlen batch, built once from HOST-side lengths (no device
    sync when it is reused): every rank can compute every rank's part, so the per-rank token
    counts need no exchange.

    mine_q / mine_k : packed positions of this rank's query / key tokens (device, int64)
    cu_q / cu_k     : this rank's local cumulative lengths (device, int32)
    max_q / max_k   : this rank's longest sequences (0 if it has none)
    counts          : query tokens per rank;  inv: for each packed query position, its row in the
                      rank-major gathered [world * max(counts)] buffer (device, int64)"""
    parts: tuple
    mine_q: torch.Tensor
    mine_k: torch.Tensor
    cu_q: torch.Tensor
    cu_k: torch.Tensor
    max_q: int
    max_k: int
    counts: tuple
    inv: torch.Tensor


def varlen_plan(seqlens_q: Sequence[int], seqlens_k: Sequence[int], world: int, rank: int,
                device) -> VarlenPlan:
    """Plan for `sharded_varlen` from host lengths (lists of ints), balanced on s_q * s_k."""
    lq = [int(x) for x in seqlens_q]
    lk = [int(x) for x in seqlens_k]
    parts = balanced_sequences(lq, lk, world)
    cq = [0]
    ck = [0]
    for a, b in zip(lq, lk):
        cq.append(cq[-1] + a)
        ck.append(ck[-1] + b)

    def positions(seqs, cu):
        return [t for i in seqs for t in range(cu[i], cu[i + 1])]
    counts = [sum(lq[i] for i in p) for p in parts]
    nmax = max(counts) if counts else 0
    inv = [0] * cq[-1]
    for r, p in enumerate(parts):
        for j, t in enumerate(positions(p, cq)):
            inv[t] = r * nmax + j
    mine = parts[rank]

    def cum(lens):
        out = [0]
        for x in lens:
            out.append(out[-1] + x)
        return out
    L = lambda xs: torch.tensor(xs, dtype=torch.long, device=device)  # noqa: E731
    return VarlenPlan(
        parts=tuple(tuple(p) for p in parts),
        mine_q=L(positions(mine, cq)), mine_k=L(positions(mine, ck)),
        cu_q=torch.tensor(cum([lq[i] for i in mine]), dtype=torch.int32, device=device),
        cu_k=torch.tensor(cum([lk[i] for i in mine]), dtype=torch.int32, device=device),
        max_q=max([lq[i] for i in mine], default=0), max_k=max([lk[i] for i in mine], default=0),
        counts=tuple(counts), inv=L(inv))


class _GatherPacked(torch.autograd.Function):
    """All-gather of per-rank packed outputs back into the global packed order (rank-major
    buffer padded to the largest count, then one index_select).  Backward: this rank's rows of
    the output gradient, no communication (as `_AllGatherDim`)."""

    @staticmethod
    def forward(ctx, local, plan):
        dist, rank, world = _world()
        ctx.mine = plan.mine_q
        nmax = max(plan.counts)
        buf = local.new_zeros((nmax,) + tuple(local.shape[1:]))
        buf[: local.shape[0]] = local
        gathered = local.new_empty((world * nmax,) + tuple(local.shape[1:]))
        dist.all_gather_into_tensor(gathered, buf)
        return gathered.index_select(0, plan.inv)

    @staticmethod
    def backward(ctx, grad):
        return grad.index_select(0, ctx.mine), None


def sharded_varlen(q, k, v, cu_seqlens_q=None, cu_seqlens_k=None, local_fn: Callable | None = None,
                   gather: bool = True, plan: VarlenPlan | None = None, **kw):
    """Sequence-sharded varlen attention (C4): ranks take whole sequences, balanced on
    s_q*s_k; outputs are all-gathered back into the packed [total_q, H, d] order.  Pass a
    `plan` (`varlen_plan`, from host-side lengths) to run without any device sync; without
    one it is built from `cu_seqlens_*` (one host copy of each).  Differentiable: gradients
    flow to this rank's tokens of q / k / v.  Returns (out, packed positions of my tokens).

    Those gradients cover this rank's sequences only: the gradients of the replicated q / k / v
    and of the parameters behind them need a SUM all-reduce over the ranks (see
    `all_gather_dim`)."""
    dist, rank, world = _world()
    if local_fn is None:
        from . import flash_attn_varlen_func as local_fn
    if plan is None:
        cq = [int(x) for x in cu_seqlens_q.tolist()]
        ck = [int(x) for x in cu_seqlens_k.tolist()]
        plan = varlen_plan([b - a for a, b in zip(cq[:-1], cq[1:])],
                           [b - a for a, b in zip(ck[:-1], ck[1:])], world, rank, q.device)
    if plan.mine_q.numel():
        out_local = local_fn(q.index_select(0, plan.mine_q), k.index_select(0, plan.mine_k),
                             v.index_select(0, plan.mine_k), plan.cu_q, plan.cu_k, plan.max_q,
                             plan.max_k, **kw)
    else:
        # no sequences on this rank: a zero-row output still tied to q for autograd
        out_local = q.narrow(0, 0, 0) * 0
    if not gather or world == 1:
        return out_local, plan.mine_q
    return _GatherPacked.apply(out_local, plan), plan.mine_q


def batch_shards(batch: int, world: int) -> List[Shard]:
    """Paged decode (C5): contiguous batch ranges; each rank owns its sequences' KV pages."""
    return even_ranges(batch, world)


def sharded_decode(q: torch.Tensor, kcache: torch.Tensor, vcache: torch.Tensor,
                   cache_seqlens: torch.Tensor, block_table: torch.Tensor,
                   local_fn: Callable | None = None, gather: bool = True, **kw):
    """Batch-sharded paged decode (C5): rank r takes batch rows `batch_shards(b, world)[r]` of
    q / cache_seqlens / block_table; the page pools stay where they are (a rank only reads the
    pages its own rows point to, so in a deployment each rank holds just its sequences'
    pages).  Outputs [b, sq, H, d] are all-gathered in batch order.  Returns (out, my rows)."""
    dist, rank, world = _world()
    if local_fn is None:
        from . import flash_attn_with_kvcache

        def local_fn(qq, kc, vc, sl, bt, **kk):
            return flash_attn_with_kvcache(qq, kc, vc, cache_seqlens=sl, block_table=bt, **kk)
    shards = batch_shards(q.shape[0], world)
    bs = shards[rank]
    alibi = kw.pop("alibi_slopes", None)
    if alibi is not None:
        kw["alibi_slopes"] = _slice_alibi(alibi, batch=bs)
    out_local = local_fn(q[bs.start:bs.stop].contiguous(), kcache, vcache,
                         cache_seqlens[bs.start:bs.stop].contiguous(),
                         block_table[bs.start:bs.stop].contiguous(), **kw)
    if not gather:
        return out_local, bs
    return all_gather_dim(out_local, [s.size for s in shards], 0), bs


# ------------------------------------------------------------------ ring attention ------------
# Context parallelism: one SEQUENCE sharded over the ranks.  Every rank keeps its queries; the
# K/V shards travel round the ring, each step is one forward of the unchanged kernels on one
# (queries, K/V shard) pair, and the per-step (O_t, LSE_t) are joined once by `merge_states`
# (DESIGN.md §3.9, §6).

RING_MAX_WORLD = 16      # one merge call takes this many parts (FMHA_MERGE_MAX_PARTS)


def zigzag_split(x: torch.Tensor, world: int, rank: int, dim: int = 1) -> torch.Tensor:
    """This rank's shard of `x` in the zigzag layout of causal ring attention: `dim` is cut into
    2 * world chunks and rank r holds chunks r and 2 * world - 1 - r (an early and a late one, so
    that every rank has the same causal work)."""
    n = x.shape[dim]
    if n % (2 * world):
        raise ValueError(f"zigzag_split: length {n} is not a multiple of 2 * world = {2 * world}")
    c = n // (2 * world)
    return torch.cat([x.narrow(dim, rank * c, c), x.narrow(dim, (2 * world - 1 - rank) * c, c)], dim=dim)


def zigzag_gather(shards: Sequence[torch.Tensor], dim: int = 1) -> torch.Tensor:
    """Inverse of `zigzag_split`: the whole tensor from the shards of ranks 0 .. world - 1."""
    world = len(shards)
    if shards[0].shape[dim] % 2:
        raise ValueError("zigzag_gather: a zigzag shard has an even length")
    c = shards[0].shape[dim] // 2
    chunks = [None] * (2 * world)
    for r, s in enumerate(shards):
        chunks[r], chunks[2 * world - 1 - r] = s.narrow(dim, 0, c), s.narrow(dim, c, c)
    return torch.cat(chunks, dim=dim)


class KernelOps:
    """The `ops` of `ring_attention` on the gfx950 kernels (the default).  A replacement supplies
    the same four callables:

      fwd(q, k, v, scale, causal, softcap, out=None) -> (out [b, sq, h, d], lse [b, h, sq])
      bwd(dout, q, k, v, out, lse, scale, causal, softcap, deterministic)
                                                     -> (dq, dk, dv, softmax_d [b, h, sq])
      merge(outs, lses, sink, out, lse_out)          -> (out, lse_out), written in place
      sink_bwd(lse, softmax_d, sink)                 -> dsink [h]

    `causal` is bottom-right aligned and only ever passed with sq == sk; `bwd` takes the MERGED
    out and lse of its query rows (it then yields exact dk / dv of its K/V chunk and that chunk's
    additive share of dq); tensors may be strided views."""

    @staticmethod
    def fwd(q, k, v, scale, causal, softcap, out=None):
        from . import paged_attn
        r = paged_attn.fwd(q, k, v, out, None, 0.0, scale, causal, -1, -1, softcap, False, None)
        return r[0], r[5]

    @staticmethod
    def bwd(dout, q, k, v, out, lse, scale, causal, softcap, deterministic):
        from . import paged_attn
        return tuple(paged_attn.bwd(dout, q, k, v, out, lse, None, None, None, None, 0.0, scale,
                                    causal, -1, -1, softcap, deterministic, None, None))

    @staticmethod
    def merge(outs, lses, sink, out, lse_out):
        from . import paged_attn
        return tuple(paged_attn.merge_states(outs, lses, sink, False, out, lse_out))

    @staticmethod
    def sink_bwd(lse, softmax_d, sink):
        from . import paged_attn
        return paged_attn.sink_bwd(lse.contiguous(), softmax_d.contiguous(), sink, False)


class DistRing:
    """The `ring` of `ring_attention` over a torch.distributed group (the default): `shift` posts
    one batch of isend / irecv (to the next rank, from the previous one) and returns at once;
    `wait` completes it and returns the received tensors.  A replacement needs `rank`, `world`
    and `shift(tensors) -> tensors from the previous rank`; if it has no `wait`, what `shift`
    returns is used as it is."""

    def __init__(self, group=None):
        import torch.distributed as dist
        self.dist, self.group = dist, group
        self.rank, self.world = dist.get_rank(group), dist.get_world_size(group)
        peer = (lambda i: dist.get_global_rank(group, i)) if group is not None else (lambda i: i)
        self.next, self.prev = peer((self.rank + 1) % self.world), peer((self.rank - 1) % self.world)

    def shift(self, tensors):
        dist = self.dist
        send = [t.contiguous() for t in tensors]
        recv = [torch.empty_like(t) for t in send]
        ops = [dist.P2POp(dist.isend, t, self.next, self.group) for t in send]
        ops += [dist.P2POp(dist.irecv, t, self.prev, self.group) for t in recv]
        return recv, send, dist.batch_isend_irecv(ops)

    def wait(self, pending):
        recv, _send, works = pending
        for w in works:
            w.wait()
        return recv


def _ring_wait(ring, pending):
    wait = getattr(ring, "wait", None)
    return pending if wait is None else wait(pending)


def _ring_steps(world: int, rank: int, causal: bool, c: int):
    """Step t of rank `rank`: the K/V of rank s = (rank - t) mod world and the sub-problem
    (query rows, key rows, causal flag) the kernels run on it.  Non-causal: everything.  Causal
    (zigzag shards of 2c rows): s == rank the local causal problem; s < rank all queries against
    the FIRST half of the keys (the late half lies in every local query's future); s > rank the
    SECOND half of the queries against all keys (the early half sees none of them)."""
    everything = slice(None)
    for t in range(world):
        s = (rank - t) % world
        if not causal or s == rank:
            yield t, everything, everything, causal
        elif s < rank:
            yield t, everything, slice(0, c), False
        else:
            yield t, slice(c, 2 * c), everything, False


def ring_forward(q, k, v, *, causal, softmax_scale, softcap, sink, ops, ring):
    """The forward of `ring_attention` on this rank's shards: (out [b, s_local, h, d] in q's
    dtype, lse [b, h, s_local] fp32 of the WHOLE sequence's softmax).  sink: what `ops.merge`
    takes (fp32 [h]) or None.  No autograd; `ring_attention` wraps it."""
    world, rank = ring.world, ring.rank
    b, sl, h, _ = q.shape
    c = sl // 2
    kv = (k, v)
    outs, lses, full = [], [], []
    for t, rows, keys, cz in _ring_steps(world, rank, causal, c):
        nxt = ring.shift(kv) if t + 1 < world else None      # posted before this step's compute
        kt, vt = kv
        if rows == slice(None):
            o, l = ops.fwd(q, kt[:, keys], vt[:, keys], softmax_scale, cz, softcap)
        else:
            # rows [:c] of this part are never read: the second-half merge takes rows [c:] only
            o = torch.empty_like(q)
            o2, l2 = ops.fwd(q[:, rows], kt, vt, softmax_scale, cz, softcap, o[:, rows])
            if o2.data_ptr() != o[:, rows].data_ptr():
                o[:, rows].copy_(o2)
            l = l2.new_empty((b, h, sl))
            l[:, :, rows].copy_(l2)
        outs.append(o)
        lses.append(l)
        full.append(rows == slice(None))
        if nxt is not None:
            kv = _ring_wait(ring, nxt)
    if all(full):
        out, lse = ops.merge(outs, lses, sink, None, None)
        return out, lse
    out, lse = torch.empty_like(outs[0]), torch.empty_like(lses[0])
    lo, hi = slice(0, c), slice(c, sl)
    ops.merge([o[:, lo] for o, f in zip(outs, full) if f], [l[:, :, lo] for l, f in zip(lses, full) if f],
              sink, out[:, lo], lse[:, :, lo])
    ops.merge([o[:, hi] for o in outs], [l[:, :, hi] for l in lses], sink, out[:, hi], lse[:, :, hi])
    return out, lse


def ring_backward(dout, q, k, v, out, lse, *, causal, softmax_scale, softcap, deterministic, sink,
                  ops, ring):
    """The backward of `ring_attention`: (dq, dk, dv, dsink or None) for this rank's shards from
    the merged `out` / `lse` of `ring_forward`.  The same ring: every step runs the unchanged
    `bwd` on the forward step's sub-problem; dq partials are summed in fp32 and rounded once;
    the dk / dv accumulators (fp32) travel with their K/V shard and are home after `world`
    steps.  dsink is THIS RANK'S share (its rows only)."""
    world, rank = ring.world, ring.rank
    c = q.shape[1] // 2
    acc_t = torch.float64 if q.dtype == torch.float64 else torch.float32
    dq = torch.zeros(q.shape, dtype=acc_t, device=q.device)
    kv = (k, v)
    acc = (torch.zeros(k.shape, dtype=acc_t, device=k.device), torch.zeros(v.shape, dtype=acc_t, device=v.device))
    softmax_d = None
    for t, rows, keys, cz in _ring_steps(world, rank, causal, c):
        nxt = ring.shift(kv) if t + 1 < world else None
        kt, vt = kv
        g = ops.bwd(dout[:, rows], q[:, rows], kt[:, keys], vt[:, keys], out[:, rows], lse[:, :, rows],
                    softmax_scale, cz, softcap, deterministic)
        dq[:, rows] += g[0]
        acc[0][:, keys] += g[1]
        acc[1][:, keys] += g[2]
        if t == 0:
            softmax_d = g[3]          # step 0 is the local problem: all of this rank's rows
        acc = _ring_wait(ring, ring.shift(acc)) if world > 1 else acc
        if nxt is not None:
            kv = _ring_wait(ring, nxt)
    dsink = None if sink is None else ops.sink_bwd(lse, softmax_d, sink)
    return dq.to(q.dtype), acc[0].to(k.dtype), acc[1].to(v.dtype), dsink


class _RingAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, sink, causal, softmax_scale, softcap, deterministic, ops, ring):
        s32 = None
        if sink is not None:
            s32 = sink.detach().to(device=q.device, dtype=torch.float64 if q.dtype == torch.float64
                                   else torch.float32).contiguous()
        out, lse = ring_forward(q, k, v, causal=causal, softmax_scale=softmax_scale, softcap=softcap,
                                sink=s32, ops=ops, ring=ring)
        ctx.save_for_backward(q, k, v, out, lse, *(() if s32 is None else (s32,)))
        ctx.args = (causal, softmax_scale, softcap, deterministic, ops, ring)
        ctx.sink_dtype = None if sink is None else sink.dtype
        return out

    @staticmethod
    def backward(ctx, dout):
        q, k, v, out, lse, *s32 = ctx.saved_tensors
        causal, scale, softcap, deterministic, ops, ring = ctx.args
        dq, dk, dv, dsink = ring_backward(dout, q, k, v, out, lse, causal=causal, softmax_scale=scale,
                                          softcap=softcap, deterministic=deterministic,
                                          sink=s32[0] if s32 and ctx.needs_input_grad[3] else None,
                                          ops=ops, ring=ring)
        if dsink is not None:
            dsink = dsink.to(ctx.sink_dtype)
        return (dq, dk, dv, dsink) + (None,) * 6


def ring_attention(q, k, v, *, causal=False, softmax_scale=None, softcap=0.0, deterministic=False,
                   sink=None, group=None, ops=None, ring=None, window_size=(-1, -1),
                   alibi_slopes=None, dropout_p=0.0):
    """Ring (context-parallel) attention: q, k, v are THIS RANK'S shard [b, s_local, h(k), d] of
    one long sequence; returns this rank's rows of the attention over the whole sequence.
    Differentiable in q, k, v and sink.

    Layout.  Non-causal: contiguous shards (rank r holds rows [r * s_local, (r + 1) * s_local)).
    Causal: the zigzag layout of `zigzag_split` (rank r holds chunks r and 2W - 1 - r of 2W), so
    s_local is even and every rank does the same work.

    Forward: W steps; at step t the rank holds the K/V of rank (r - t) mod W and runs one forward
    of the unchanged kernels on it (for causal: the local causal problem, all queries against
    the early key half, or the late query half against all keys, passed as strided views); the
    exchange for step t + 1 is posted before the compute of step t.  The per-step (O_t, LSE_t)
    stay in the input dtype and are merged once per query half by `merge_states`, which rounds
    once; the sink joins there and only there.  Backward: the same ring with fp32 dk / dv
    accumulators travelling alongside K/V; each step calls the unchanged backward with the
    merged out and LSE, which makes it exact for its chunk.

    sink: a per-head logit [h] as in `flash_attn_func`.  Its gradient is THIS RANK'S share (the
    sum over this rank's rows): like the gradient of any replicated parameter it needs a
    SUM all-reduce over the group by the caller (the q / k / v gradients need no reduction).

    ops: the forward / backward / merge / sink-backward callables (`KernelOps`, the gfx950
    kernels, by default); ring: the exchange (`DistRing` over `group` by default).  world == 1
    with the default ops runs `flash_attn_func` itself, bit for bit.

    Refused: sliding windows, ALiBi, dropout, fp8 inputs, more than 16 ranks (the part limit of
    one merge), an odd s_local with causal, and with the default ops a head size that is not a
    multiple of 8."""
    if tuple(int(w) for w in window_size) != (-1, -1):
        raise NotImplementedError("ring_attention does not support sliding windows")
    if alibi_slopes is not None:
        raise NotImplementedError("ring_attention does not support ALiBi")
    if dropout_p != 0.0:
        raise NotImplementedError("ring_attention does not support dropout")
    if q.dtype == torch.float8_e4m3fn or k.dtype == torch.float8_e4m3fn or v.dtype == torch.float8_e4m3fn:
        raise NotImplementedError("ring_attention does not support fp8 inputs")
    if ring is None:
        ring = DistRing(group)
    if ring.world > RING_MAX_WORLD:
        raise NotImplementedError(f"ring_attention supports at most {RING_MAX_WORLD} ranks "
                                  f"(got {ring.world}): one merge takes that many parts")
    if causal and q.shape[1] % 2:
        raise ValueError(f"ring_attention: causal needs an even s_local (zigzag halves), got {q.shape[1]}")
    if q.dim() != 4 or k.shape != v.shape or k.shape[1] != q.shape[1]:
        raise ValueError("ring_attention: q [b, s_local, h, d] and k, v [b, s_local, hk, d] shards "
                         "of one length are required")
    if sink is not None and (sink.dim() != 1 or sink.shape[0] != q.shape[2]):
        raise ValueError(f"sink must have shape (num_heads,) = ({q.shape[2]},), got {tuple(sink.shape)}")
    if softmax_scale is None:
        softmax_scale = q.shape[-1] ** (-0.5)
    if ops is None:
        if ring.world == 1:
            from . import flash_attn_func
            return flash_attn_func(q, k, v, causal=causal, softcap=softcap, deterministic=deterministic,
                                   softmax_scale=softmax_scale, sink=sink)
        if q.shape[-1] % 8:
            raise NotImplementedError("ring_attention: head size must be a multiple of 8")
        ops = KernelOps
    return _RingAttention.apply(q, k, v, sink, causal, float(softmax_scale), float(softcap),
                                bool(deterministic), ops, ring)
