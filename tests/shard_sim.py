"""R sharded ranks simulated in one process on one GPU: one HipShardEngine per rank, the three
all-to-alls of the ShardedTrainer protocol done by tensor slicing (tests/test_gpu_shard.py,
tools/shard_sim_bench.py)."""

import numpy as np


def split_pairs(buf, counts, kp):
    """A pair buffer in the wire layout ([P][kp] vectors, then [P][2] scalars) cut per peer."""
    import torch

    counts = [int(c) for c in counts]
    P = sum(counts)
    vec = torch.split(buf[: P * kp], [c * kp for c in counts])
    sc = torch.split(buf[P * kp:], [c * 2 for c in counts])
    return list(zip(vec, sc))


def cat_pairs(parts):
    """Concatenate per-peer pieces back into the wire layout (what an all-to-all delivers)."""
    import torch

    return torch.cat([v for v, _ in parts] + [s for _, s in parts])


def simulated_step(engines, batches, t, step_size, reg):
    """One iteration of the ShardedTrainer protocol with the all-to-alls done by slicing; returns
    pair_cnt[src][owner], the (sample, owner) pairs every rank sent."""
    import torch

    R = len(engines)
    kp = engines[0].kp
    routed = [e.route(b) for e, b in zip(engines, batches)]
    ent_cnt = [c[:R] for _, _, c in routed]   # [src][owner]
    pair_cnt = [c[R:] for _, _, c in routed]
    keep = []
    torch.cuda.synchronize()  # the slicing below runs on the main stream, owner_prepare on the side streams
    for o in range(R):
        slots = torch.cat([torch.split(routed[r][0], ent_cnt[r].tolist())[o] for r in range(R)])
        ents = torch.cat([torch.split(routed[r][1], (2 * ent_cnt[r]).tolist())[o] for r in range(R)])
        src_e = np.array([ent_cnt[r][o] for r in range(R)])
        src_p = np.array([pair_cnt[r][o] for r in range(R)])
        torch.cuda.synchronize()
        engines[o].owner_prepare(batches[o], slots, ents, src_e, src_p)
        keep.append((slots, ents, src_p))
    torch.cuda.synchronize()  # route / prepare ran on the engines' side streams
    partials = []
    for o in range(R):
        out = engines[o].owner_forward(batches[o], int(keep[o][2].sum()))
        partials.append(split_pairs(out, keep[o][2], kp))
    s_rows = []
    for r in range(R):
        pin = cat_pairs([partials[o][r] for o in range(R)])
        s = engines[r].combine(batches[r], pin, int(pair_cnt[r].sum()))
        s_rows.append(split_pairs(s, pair_cnt[r], kp))
    gm = sum(int(b.n_rows) for b in batches)
    for o in range(R):
        engines[o].owner_update(batches[o], cat_pairs([s_rows[r][o] for r in range(R)]), t, step_size, reg, gm)
    torch.cuda.synchronize()
    return pair_cnt
