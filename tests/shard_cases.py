"""The cases of tests/test_gpu_shard_phases.py, built without a GPU: the batches a route is checked on, the
received buffers an owner is checked on and the hand-made partials a combine is checked on, each with the
conditions that show it crosses the edge it is named for.  tests/test_shard_phases_cpu.py runs every
builder and its conditions on the CPU; the GPU tests assert the same conditions before they run.

Sizes come from the library's geometry (tests/shard_probe.py) as a Geometry g; nothing here copies a
constant of fm_shard.hip.
"""

from __future__ import annotations

from collections import namedtuple

import numpy as np

from oracle import fm_ref as R_
from problems import f32, make_rows
from shard_ref_engine import NpBatch, NumpyShardEngine

RouteCase = namedtuple("RouteCase", "name R F csr edges")  # edges: [(what, condition that proves it)]
OwnerCase = namedtuple("OwnerCase", "name R owner F k sources ids w V edges")

K_ROUTE = 4  # the route does not read the table: any k

ROUTE_R = [1, 2, 3, 4, 7, 8, 9, 16, 17, 31, 32, 33, 63, 64]
# every small case by name ("max": the most ranks the library takes; W: the wave, T: the pair tile), so a test
# can be parametrised before the geometry is read
_SIZES = ["1", "W-1", "W", "W+1", "T-1", "T", "T+1", "2T+1"]
ROUTE_NAMES = ([f"rows_{z}_R{r}" for r in ("3", "max") for z in _SIZES] + [f"rows_T+1_R{r}" for r in ROUTE_R if r not in (3, 64)]
               + ["lengths_R3", "lengths_Rmax", "owners_Rmax", "coprime7_Rmax", "coprime5_R3", "topslot_R2", "topslot_R4",
                  "topslot_R3", "topslot_Rmax", "F40_Rmax", "F2_R3"])
OWNER_NAMES = (["random_R1_k3", "random_R2_k8", "random_R3_k8", "random_R3_k3", "random_Rmax_k8"]
               + [f"{h}_R{r}" for r in ("3", "max") for h in ("empty_first", "empty_middle", "empty_last", "all_but_one")]
               + ["empty_run_R3", "one_each_R2", "one_each_R3", "one_each_Rmax", "pairs_1_and_300", "n0_R3"])


def csr_of(lengths, col, seed, labels=None):
    """A batch from per-row lengths and ids; values fp32-representable, with zeros and ones among them."""
    rng = np.random.default_rng(seed)
    lengths = np.asarray(lengths, dtype=np.int64)
    n = int(lengths.sum())
    x = f32(rng.normal(0.0, 1.0, n))
    u = rng.random(n)
    x[u < 0.05] = 0.0
    x[u > 0.7] = 1.0
    y = f32(rng.normal(0.0, 1.0, len(lengths))) if labels is None else labels
    return R_.CSR(np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64), np.asarray(col, dtype=np.int32), x, y)


def by_owner(seed, has, R, slots=64, F=None):
    """Rows from has [B][R] (entries of row i at owner r; ids r modulo R): F = R * slots + 1 unless given."""
    has = np.asarray(has, dtype=np.int64).reshape(-1, R)
    F = R * slots + 1 if F is None else F
    return make_rows(seed, has, F, K_ROUTE, pool=R * slots, labels="real")[0], F


def random_has(seed, B, R, p=None):
    rng = np.random.default_rng(seed)
    p = min(0.5, 4.0 / R) if p is None else p
    return (rng.random((B, R)) < p) * rng.integers(1, 3, (B, R))


def masks(csr, R, F):
    """has [B][R] of a batch, straight from the ids."""
    sample = np.repeat(np.arange(csr.n_rows), np.diff(csr.row_ptr))
    ids = csr.col.astype(np.int64)
    m = np.zeros((csr.n_rows, R), dtype=bool)
    m[sample[ids < F], ids[ids < F] % R] = True
    return m


# ------------------------------------------------------------------------------------------ route
def route_cases(g):
    """name -> builder() of every small route case."""
    T, W, team = g.pair_tile, 64, g.route_team
    out = {}

    sizes = {"1": 1, "W-1": W - 1, "W": W, "W+1": W + 1, "T-1": T - 1, "T": T, "T+1": T + 1, "2T+1": 2 * T + 1}

    def size_case(sym, R, rname):
        def build():
            B = sizes[sym]
            csr, F = by_owner(1000 + B + R, random_has(B * 131 + R, B, R), R)
            edges = [("the rows are the named size", csr.n_rows == B),
                     ("a partial last wave", B % W != 0) if sym not in ("W", "T") else ("whole waves", B % W == 0),
                     ("more than one tile", B > T) if sym in ("T+1", "2T+1") else ("one tile", B <= T)]
            return RouteCase(f"rows_{sym}_R{rname}", R, F, csr, edges)
        return build

    for R, rname in ((3, "3"), (g.max_r, "max")):
        for sym in sizes:
            out[f"rows_{sym}_R{rname}"] = size_case(sym, R, rname)
    for R in ROUTE_R:
        if R not in (3, g.max_r):
            out[f"rows_T+1_R{R}"] = size_case("T+1", R, str(R))

    def lengths_case(R, rname):
        def build():
            # the route team's trips: a row of 0, 1, team - 1, team, team + 1 and 2 team + 1 entries
            want = np.array([0, 1, team - 1, team, team + 1, 2 * team + 1])
            rng = np.random.default_rng(5 + R)
            B = 6 * 11 + 1
            F = R * 64 + 1
            lens = want[np.arange(B) % 6]
            col = np.concatenate([rng.choice(F, size=n, replace=False) for n in lens]) if lens.sum() else []
            csr = csr_of(lens, col, 6 + R)
            edges = [("every trip edge of a team is a row length", set(want.tolist()) <= set(np.diff(csr.row_ptr).tolist())),
                     ("a row takes a third trip", np.diff(csr.row_ptr).max() > 2 * team)]
            return RouteCase(f"lengths_R{rname}", R, F, csr, edges)
        return build

    for R, rname in ((3, "3"), (g.max_r, "max")):
        out[f"lengths_R{rname}"] = lengths_case(R, rname)

    def owners_case():
        R = g.max_r
        B = T + 1
        has = np.zeros((B, R), dtype=np.int64)
        kind = np.arange(B) % 5
        has[kind == 0] = 1  # every owner: the mask is all ones
        has[kind == 1, R - 1] = 2  # only the last owner
        has[kind == 2, 32] = 1  # only the first owner of the mask's high half
        has[kind == 3, 31] = 3  # only the last of its low half
        csr, F = by_owner(77, has, R)
        m = masks(csr, R, F)
        edges = [("a sample with every owner", m.all(axis=1).any()),
                 ("a sample with owner R - 1 alone", (m[:, R - 1] & (m.sum(axis=1) == 1)).any()),
                 ("with owner 32 alone", (m[:, 32] & (m.sum(axis=1) == 1)).any()),
                 ("with owner 31 alone", (m[:, 31] & (m.sum(axis=1) == 1)).any()),
                 ("with none", (~m.any(axis=1)).any()), ("R is the most ranks", R == g.max_r and R > 32)]
        return RouteCase("owners_Rmax", R, F, csr, edges)

    out["owners_Rmax"] = owners_case

    def coprime_case(R, period, rname):
        def build():
            B = 2 * T + 1
            i, o = np.arange(B)[:, None], np.arange(R)[None, :]
            has = ((i + 3 * o) % period == 0).astype(np.int64)
            csr, F = by_owner(90 + R, has, R)
            m = masks(csr, R, F)
            edges = [("the period is coprime to the wave", np.gcd(period, W) == 1),
                     ("neighbouring waves see different ballots", all((m[a:a + W] != m[a + W:a + 2 * W]).any()
                                                                     for a in range(0, B - 2 * W, W)))]
            return RouteCase(f"coprime{period}_R{rname}", R, F, csr, edges)
        return build

    out["coprime7_Rmax"] = coprime_case(g.max_r, 7, "max")
    out["coprime5_R3"] = coprime_case(3, 5, "3")

    def top_slot_case(R, s, rname):
        def build():
            # F = R 2^s + 1: owner 0's last slot (id F - 1, in every other row) needs one more key bit than
            # any other owner's
            F = R * (1 << s) + 1
            csr, _ = by_owner(40 + R, random_has(41 + R, T + 1, R), R, slots=1 << s)
            col = csr.col.copy()
            first = csr.row_ptr[:-1][np.diff(csr.row_ptr) > 0][::2]
            col[first] = F - 1
            csr = R_.CSR(csr.row_ptr, col, csr.val, csr.label)
            edges = [("F = R 2^s + 1", F == R * 2 ** s + 1), ("the top slot is routed", (csr.col == F - 1).any()),
                     ("it needs its own bit", ((F - 1) // R).bit_length() > ((F - 2) // R).bit_length())]
            return RouteCase(f"topslot_R{rname}", R, F, csr, edges)
        return build

    for R, s, rname in ((2, 8, "2"), (4, 7, "4"), (3, 6, "3"), (g.max_r, 4, "max")):
        out[f"topslot_R{rname}"] = top_slot_case(R, s, rname)

    def few_features_case(R, F, rname):
        def build():
            rng = np.random.default_rng(R + F)
            B = T + 1
            lens = rng.integers(0, F + 1, B)
            col = np.concatenate([rng.choice(F, size=n, replace=False) for n in lens])
            csr = csr_of(lens, col, 3 * R + F)
            edges = [("fewer features than ranks", F < R), ("the owners from F on get nothing", not masks(csr, R, F)[:, F:].any())]
            return RouteCase(f"F{F}_R{rname}", R, F, csr, edges)
        return build

    out["F40_Rmax"] = few_features_case(g.max_r, 40, "max")
    out["F2_R3"] = few_features_case(3, 2, "3")
    return out


def large_route_case(g, R):
    """More rows than one k_sample_mask sweep and one k_rows_scan trip take, more entries than one
    k_route_keys sweep: rows of 0..34 entries."""
    B = int(g.mask_sweep) + g.pair_tile + 1
    rng = np.random.default_rng(11)
    csr = make_rows(7, rng.integers(0, 35, B), 30011, K_ROUTE, labels="real")[0]
    ntiles = -(-B // g.pair_tile)
    edges = [("a second k_sample_mask sweep", B > g.mask_sweep), ("a second k_rows_scan trip", ntiles > g.scan_trip),
             ("k_route_keys' unrolled entries", g.route_unroll > 1 and csr.nnz > g.route_sweep),
             ("the last tile is partial", B % g.pair_tile != 0)]
    return RouteCase(f"large_R{R}", R, 30011, csr, edges)


def outside_ids(seed, csr, F, frac=0.3, whole_rows=3):
    """csr with a share of its ids moved to [F, F + 50) and a few rows wholly outside the model."""
    rng = np.random.default_rng(seed)
    col = csr.col.copy()
    out = rng.random(len(col)) < frac
    rows = np.nonzero(np.diff(csr.row_ptr) > 0)[0][:: max(1, csr.n_rows // whole_rows)]
    for r in rows:
        out[csr.row_ptr[r]:csr.row_ptr[r + 1]] = True
    col[out] = F + rng.integers(0, 50, int(out.sum()))
    return R_.CSR(csr.row_ptr, col, csr.val, csr.label), out


def drop_entries(csr, out):
    """csr without the flagged entries (its rows kept)."""
    sample = np.repeat(np.arange(csr.n_rows), np.diff(csr.row_ptr))
    lens = np.bincount(sample[~out], minlength=csr.n_rows)
    return R_.CSR(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), csr.col[~out], csr.val[~out], csr.label)


# ------------------------------------------------------------------------------------------ owner
def received(case):
    """What owner case.owner receives when source r routes case.sources[r]: the reference's route of
    every source, its block for that owner, source after source.  -> slots int32 [n], ents uint32 [n][2],
    src_entries [R], src_pairs [R]."""
    R, o = case.R, case.owner
    slots, ents, se, sp = [], [], [], []
    for r, csr in enumerate(case.sources):
        eng = NumpyShardEngine(case.F, case.k, r, R)
        s, e, counts = eng.route(NpBatch(csr))
        off = int(counts[:o].sum())
        n = int(counts[o])
        slots.append(s.numpy()[off:off + n])
        ents.append(e.numpy().view(np.uint32).reshape(-1, 2)[off:off + n])
        se.append(n)
        sp.append(int(counts[R + o]))
    return (np.concatenate(slots).astype(np.int32), np.concatenate(ents).reshape(-1, 2), np.asarray(se, dtype=np.int64),
            np.asarray(sp, dtype=np.int64))


def _empty_csr():
    return R_.CSR(np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0), np.zeros(0))


def _table(seed, F, k, absent_fifth=True):
    rng = np.random.default_rng(seed)
    ids = np.arange(F, dtype=np.int32)
    if absent_fifth:
        ids = np.sort(rng.permutation(F)[F // 5:]).astype(np.int32)
    return ids, f32(rng.normal(0.0, 0.1, len(ids))), f32(rng.normal(0.0, 0.1, (len(ids), k)))


def owner_cases(g):
    out = {}

    def finish(name, R, owner, F, k, sources, extra=()):
        ids, w, V = _table(len(name) + R, F, k)
        c = OwnerCase(name, R, owner, F, k, sources, ids, w, V, None)
        slots, ents, se, sp = received(c)
        edges = list(extra(slots, ents, se, sp)) if extra else []
        mine = np.arange(owner, F, R)
        edges.append(("a fifth of the table is absent, rows of this owner among them",
                      len(ids) == F - F // 5 and not np.isin(mine, ids).all() and np.isin(mine, ids).any()))
        return c._replace(edges=edges)

    def random_case(R, k, rname):
        def build():
            srcs = [by_owner(300 + 7 * r + R, random_has(301 + r + R, 37 + 3 * (r % 5), R, p=max(0.3, 2.0 / R)), R)[0]
                    for r in range(R)]
            return finish(f"random_R{rname}_k{k}", R, R - 1, R * 64 + 1, k, srcs,
                          lambda s, e, se, sp: [("every source sends", (se > 0).all()), ("pairs of several entries", (se > sp).any())])
        return build

    for R, k, rname in ((1, 3, "1"), (2, 8, "2"), (3, 8, "3"), (3, 3, "3"), (g.max_r, 8, "max")):
        out[f"random_R{rname}_k{k}"] = random_case(R, k, rname)

    def holes_case(R, holes, name, rname):
        def build():
            srcs = []
            for r in range(R):
                has = random_has(500 + r, 41, R, p=0.5)
                if r in holes:
                    has[:, 0] = 0  # the source holds rows, none with an entry of owner 0
                srcs.append(by_owner(501 + r, has, R)[0])

            def extra(s, e, se, sp):
                full = [r for r in range(R) if r not in holes]
                return [("the named sources send nothing", all(se[r] == 0 and sp[r] == 0 for r in holes)),
                        ("the others send", all(se[r] > 0 for r in full))]
            return finish(f"{name}_R{rname}", R, 0, R * 64 + 1, 8, srcs, extra)
        return build

    for R, rname in ((3, "3"), (g.max_r, "max")):
        out[f"empty_first_R{rname}"] = holes_case(R, {0}, "empty_first", rname)
        out[f"empty_middle_R{rname}"] = holes_case(R, {R // 2}, "empty_middle", rname)
        out[f"empty_last_R{rname}"] = holes_case(R, {R - 1}, "empty_last", rname)
        out[f"all_but_one_R{rname}"] = holes_case(R, set(range(R)) - {R // 2}, "all_but_one", rname)
    out["empty_run_R3"] = holes_case(3, {0, 1}, "empty_run", "3")

    def one_each_case(R, rname):
        def build():
            rng = np.random.default_rng(R)
            srcs = [csr_of([0, 1, 0], [R * int(rng.integers(0, 64))], 600 + r) for r in range(R)]

            def extra(s, e, se, sp):
                return [("every source sends one pair of one entry", (se == 1).all() and (sp == 1).all()),
                        ("local index 0 follows local index 0 at every source boundary", (e[:, 0] == 0).all() and len(e) == R)]
            return finish(f"one_each_R{rname}", R, 0, R * 64 + 1, 8, srcs, extra)
        return build

    for R, rname in ((2, "2"), (3, "3"), (g.max_r, "max")):
        out[f"one_each_R{rname}"] = one_each_case(R, rname)

    def long_pairs_case():
        R = 3
        has = np.zeros((40, R), dtype=np.int64)
        has[:, 1] = np.where(np.arange(40) % 2 == 0, 1, 300)
        srcs = [by_owner(700 + r, has, R, slots=512)[0] for r in range(R)]
        return finish("pairs_1_and_300", R, 1, R * 512 + 1, 8, srcs,
                      lambda s, e, se, sp: [("pairs of 1 and of 300 entries alternate",
                                             set(np.diff(np.nonzero(np.diff(e[: se[0], 0], prepend=-1))[0]).tolist()) == {1, 300})])

    out["pairs_1_and_300"] = long_pairs_case

    def nothing_case():
        return finish("n0_R3", 3, 0, 3 * 64 + 1, 8, [_empty_csr()] * 3, lambda s, e, se, sp: [("n = 0", len(s) == 0 and se.sum() == 0)])

    out["n0_R3"] = nothing_case
    return out


def large_owner_case(g):
    """More received entries than one k_pair_table sweep takes (its unrolled entries), three sources."""
    R, per = 3, 12
    rows = int(g.table_sweep) // (R * per) + 1000
    has = np.zeros((rows, R), dtype=np.int64)
    has[:, 0] = per
    srcs = [by_owner(800 + r, has, R, slots=10003)[0] for r in range(R)]
    ids, w, V = _table(9, R * 10003 + 1, 3)
    c = OwnerCase("large_R3", R, 0, R * 10003 + 1, 3, srcs, ids, w, V, None)
    return c._replace(edges=[("k_pair_table's unrolled entries", g.table_unroll > 1 and R * rows * per > g.table_sweep)])


# ------------------------------------------------------------------------------------------ combine
COMBINE_K = [3, 8, 13, 29, 33, 70]
COMBINE_R = [3, 8, 9, 64]
COMBINE_B = 257


def combine_batch(R, seed=0):
    """The batch a combine is checked on: rows of no pair, of every owner and of the last owner alone among
    random ones.  -> (csr, F)"""
    has = random_has(900 + R + seed, COMBINE_B, R)
    has[0::7] = 0
    has[1::7] = 1
    has[2::7] = 0
    has[2::7, R - 1] = 2
    return by_owner(901 + R + seed, has, R, slots=16)


def tagged_partials(pairs_out, kp, wide):
    """Partial rows whose words name their (owner, pair, column): both signs, exponents over 2^-12 .. 2^11,
    ten mantissa bits (fp32 words), or those and one more at 2^-40 (fp64 words: not fp32-representable).
    -> vec [Ps][kp], sc [Ps][2] in the wire's word type."""
    o = np.repeat(np.arange(len(pairs_out)), pairs_out)[:, None]
    p = np.concatenate([np.arange(n) for n in pairs_out] + [np.zeros(0, dtype=np.int64)])[:, None].astype(np.int64)
    c = np.arange(kp + 2)[None, :]
    sign = np.where((o + p + c) % 2 == 0, 1.0, -1.0)
    v = sign * (1.0 + ((o * 131 + p * 17 + c * 7) % 1024) / 1024.0) * 2.0 ** ((o * 5 + p * 3 + c) % 24 - 12)
    if wide:
        v = v * (1.0 + 2.0 ** -40)
    v = v.astype(np.float64 if wide else np.float32)
    return np.ascontiguousarray(v[:, :kp]), np.ascontiguousarray(v[:, kp:])


def near_labels(yhat, seed):
    """fp64 labels that are not fp32-representable; every other one within 2^-10 of its sample's yhat, so
    an r formed from fp32 operands would be off by far more than r's own rounding."""
    rng = np.random.default_rng(seed)
    y = rng.normal(0.0, 1.0, len(yhat)) + np.pi * 1e-9
    near = np.arange(len(yhat)) % 2 == 0
    y[near] = (yhat.astype(np.float64) * (1.0 + 2.0 ** -10) + 2.0 ** -30)[near]
    return y
