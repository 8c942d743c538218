"""Data-parallel utterance sharding: one process per GPU, weights replicated, utterance i -> rank
i mod world, no collective on the data path.  The only collective is the optional gather of the finished code
tensors (ragged in time: padded to the longest, lengths travel alongside) — RCCL all_gather on GPUs, gloo on CPU."""
from __future__ import annotations

import torch
import torch.distributed as dist


def shard_indices(n_utterances: int, rank: int, world: int) -> list[int]:
    """Round-robin assignment: utterance i runs on rank i % world."""
    return list(range(rank, n_utterances, world))


def gather_codes(local_codes: list[torch.Tensor], n_utterances: int, pad_value: int = 0, group=None) -> list[torch.Tensor] | None:
    """local_codes[j] = int64 [n_q, T_j] of the j-th utterance of this rank (shard_indices order).  Returns, on every
    rank, the list of all n_utterances code tensors in utterance order.  Works for world == 1 without a process group."""
    if not dist.is_available() or not dist.is_initialized():
        assert len(local_codes) == n_utterances
        return list(local_codes)
    world, rank = dist.get_world_size(group), dist.get_rank(group)
    dev = local_codes[0].device if local_codes else torch.device("cpu")
    n_q = local_codes[0].shape[0] if local_codes else 0
    meta = torch.tensor([len(local_codes), n_q, max([c.shape[1] for c in local_codes], default=0)], dtype=torch.int64, device=dev)
    metas = [torch.empty_like(meta) for _ in range(world)]
    dist.all_gather(metas, meta, group=group)
    per_rank = max(int(m[0]) for m in metas)
    n_q = max(int(m[1]) for m in metas)
    t_max = max(int(m[2]) for m in metas)
    buf = torch.full((per_rank, n_q, t_max), pad_value, dtype=torch.int64, device=dev)
    lens = torch.zeros(per_rank, dtype=torch.int64, device=dev)
    for j, c in enumerate(local_codes):
        buf[j, :, : c.shape[1]] = c
        lens[j] = c.shape[1]
    bufs = [torch.empty_like(buf) for _ in range(world)]
    lenss = [torch.empty_like(lens) for _ in range(world)]
    dist.all_gather(bufs, buf, group=group)
    dist.all_gather(lenss, lens, group=group)
    out: list[torch.Tensor | None] = [None] * n_utterances
    for r in range(world):
        for j, i in enumerate(shard_indices(n_utterances, r, world)):
            out[i] = bufs[r][j, :, : int(lenss[r][j])].clone()
    assert all(o is not None for o in out)
    return out  # type: ignore[return-value]


def generate_sharded(generate_fn, conditionings: list[torch.Tensor], gather: bool = True, group=None, batch_size: int = 1):
    """Run `generate_fn` on this rank's share of `conditionings` (each [2, L_c, d] = [cond ‖ uncond] of one utterance);
    optionally gather.  batch_size == 1: `generate_fn(cond) -> int64 [1, n_q, T]` per utterance.  batch_size > 1: the
    share runs in groups of up to `batch_size` utterances, `generate_fn(cond [2b, L_c, d], b) -> int64 [b, n_q, T]`
    with rows [cond_0..cond_{b-1}, uncond_0..uncond_{b-1}] (Zonos.generate's batch layout).  A group whose conditionings differ in
    length is right-padded (conditioning.pad_conditionings) and goes out as `generate_fn(cond [2b, L_max, d], b, lengths)`, lengths =
    the b valid lengths (Zonos.generate's `conditioning_lengths`); groups of one length keep the two-argument call."""
    world = dist.get_world_size(group) if dist.is_available() and dist.is_initialized() else 1
    rank = dist.get_rank(group) if world > 1 else 0
    share = shard_indices(len(conditionings), rank, world)
    if batch_size <= 1:
        mine = [generate_fn(conditionings[i])[0] for i in share]
    else:
        mine = []
        for j in range(0, len(share), batch_size):
            grp = [conditionings[i] for i in share[j:j + batch_size]]
            if len({c.shape[1] for c in grp}) > 1:
                from .conditioning import pad_conditionings
                cond, lengths = pad_conditionings(grp, cfg_scale=2.0)
                codes = generate_fn(cond, len(grp), lengths)
            else:
                cond = torch.cat([c[0:1] for c in grp] + [c[1:2] for c in grp], dim=0)
                codes = generate_fn(cond, len(grp))
            mine.extend(codes[b] for b in range(len(grp)))
    return gather_codes(mine, len(conditionings), group=group) if gather else mine


MIXED_CALL_ROWS = 64          # rows of one generate_batch(mixed_guidance=True) call (model.MAX_BATCH_REQUESTS)


def request_groups(requests, share: list[int], batch_size: int, ragged_prefix: bool = False, mixed_guidance: bool = False) -> list[list[int]]:
    """This rank's requests (indices `share`) as the calls it makes: requests that may share a `Zonos.generate_batch` call - all guided or
    all at cfg_scale == 1, one audio prefix length (any, with `ragged_prefix`) - in groups of up to `batch_size`, each in request order.
    With `mixed_guidance` the groups no longer split by guidance; a group then also ends before its rows (one per cfg_scale == 1 request,
    two per guided one) would exceed MIXED_CALL_ROWS."""
    buckets: dict[tuple[bool, int], list[int]] = {}
    for i in share:
        r = requests[i]
        key = (False if mixed_guidance else float(r.cfg_scale) != 1.0,
               0 if ragged_prefix or r.audio_prefix_codes is None else int(r.audio_prefix_codes.shape[-1]))
        buckets.setdefault(key, []).append(i)
    step = max(1, int(batch_size))
    if not mixed_guidance:
        return [idx[j:j + step] for idx in buckets.values() for j in range(0, len(idx), step)]
    groups = []
    for idx in buckets.values():
        cur, rows = [], 0
        for i in idx:
            need = 2 if float(requests[i].cfg_scale) != 1.0 else 1
            if cur and (len(cur) == step or rows + need > MIXED_CALL_ROWS):
                groups.append(cur)
                cur, rows = [], 0
            cur.append(i)
            rows += need
        if cur:
            groups.append(cur)
    return groups


def generate_sharded_requests(generate_batch_fn, requests, gather: bool = True, group=None, batch_size: int = 8, ragged_prefix: bool = False,
                              mixed_guidance: bool = False):
    """`generate_sharded` for `model.GenRequest`s, each with its own sampling parameters, seed, cfg_scale and length: request i runs on rank
    i mod world, and a rank's share goes out in `request_groups` as `generate_batch_fn(list of requests) -> list of int64 [1, n_q, T]`
    (`Zonos.generate_batch`).  Returns the code tensors [n_q, T_i] in request order: of every request on every rank with `gather`, of this
    rank's share (`shard_indices` order) without.  `ragged_prefix`: requests with audio prefixes of different lengths share a call, made as
    `generate_batch_fn(list of requests, ragged_prefix=True)`.  `mixed_guidance`: guided and cfg_scale == 1 requests share a call as well, made
    with `mixed_guidance=True`."""
    world = dist.get_world_size(group) if dist.is_available() and dist.is_initialized() else 1
    rank = dist.get_rank(group) if world > 1 else 0
    share = shard_indices(len(requests), rank, world)
    done: dict[int, torch.Tensor] = {}
    for idx in request_groups(requests, share, batch_size, ragged_prefix, mixed_guidance):
        batch = [requests[i] for i in idx]
        kw = {**({"ragged_prefix": True} if ragged_prefix else {}), **({"mixed_guidance": True} if mixed_guidance else {})}
        outs = generate_batch_fn(batch, **kw)
        if len(outs) != len(idx):
            raise ValueError(f"generate_batch_fn returned {len(outs)} results for {len(idx)} requests")
        for i, o in zip(idx, outs):
            done[i] = o[0]
    mine = [done[i] for i in share]
    return gather_codes(mine, len(requests), group=group) if gather else mine
