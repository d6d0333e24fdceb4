"""TEST INFRASTRUCTURE: a NumPy implementation of the sharded phase functions (route /
owner_forward / combine / owner_update, include/fm_hip.h fm_shard_*) with the oracle's fp64
math and the same fp32 wire formats, so the exchange protocol of
fm_spark_amd.distributed.ShardedTrainer can run on CPU under gloo."""

import math
from collections import namedtuple

import numpy as np
import torch

# NumpyShardEngine.combine_exact's result, per sample (pair_sample: per pair)
CombineRef = namedtuple("CombineRef", "S yhat r sum_a2 abs_vv abs_wx pair_sample has_pair")


def rows_to_soa(rows, kp):
    """[P][kp + 2] rows -> the fp32 wire layout: [P][kp] vectors, then [P][2] scalars (flat)."""
    rows = np.asarray(rows, dtype=np.float32)
    return np.ascontiguousarray(np.concatenate([rows[:, :kp].reshape(-1), rows[:, kp:kp + 2].reshape(-1)]))


def soa_to_rows(flat, kp):
    P = len(flat) // (kp + 2)
    return np.concatenate([flat[: P * kp].reshape(P, kp), flat[P * kp:].reshape(P, 2)], axis=1).astype(np.float64)


class NpBatch:
    def __init__(self, csr):
        self.csr = csr
        self.n_rows = csr.n_rows
        self.nnz = csr.nnz


class NumpyShardEngine:
    def __init__(self, num_features, k, rank, world, w0=0.0):
        self.device = torch.device("cpu")
        self.F, self.k, self.R, self.rank, self.w0 = num_features, k, world, rank, w0
        self.kp = (k + 3) // 4 * 4
        self.width = self.kp + 2  # wire: [P][kp] vectors, then [P][2] scalars
        self.rows = (num_features - rank + world - 1) // world
        self.w = np.zeros(self.rows)
        self.V = np.zeros((self.rows, k))
        self.present = np.zeros(self.rows, dtype=bool)
        self.stats = (0.0, 0, 0)

    def batch(self, csr):
        return NpBatch(csr)

    def load_tables(self, ids, w, V):
        ids = np.asarray(ids, dtype=np.int64)
        mine = ids % self.R == self.rank
        slots = ids[mine] // self.R
        self.w[slots] = np.asarray(w)[mine]
        self.V[slots] = np.asarray(V).reshape(len(ids), self.k)[mine]
        self.present[slots] = True

    def export_tables(self):
        slots = np.nonzero(self.present)[0]
        return (slots * self.R + self.rank).astype(np.int32), self.w[slots], self.V[slots]

    # requester -------------------------------------------------------------------
    def route(self, b):
        """Ids >= F (a predict batch's ids outside the model) belong to no owner: they are absent from
        the masks, counts and send buffers, and a row holding only such ids has no pair."""
        csr = b.csr
        ids = csr.col.astype(np.int64)
        sample = np.repeat(np.arange(csr.n_rows), np.diff(csr.row_ptr))
        val = csr.val
        inside = ids < self.F
        if not inside.all():
            ids, sample, val = ids[inside], sample[inside], val[inside]
        owner = ids % self.R
        order = np.argsort(owner, kind="stable")
        send_slot = (ids[order] // self.R).astype(np.int32)
        ents = np.bincount(owner, minlength=self.R)
        has = np.zeros((csr.n_rows, self.R), dtype=bool)
        has[sample, owner] = True
        pairs = has.sum(axis=0)
        b.pairidx = np.where(has, np.cumsum(has, axis=0) - 1, -1)  # [B][R]
        b.pairs_out = pairs
        # wire entry = {index of its (sample, owner) pair within this rank's pairs to the owner, x}
        local = b.pairidx[sample[order], owner[order]].astype(np.uint32)
        ent = np.stack([local, val[order].astype(np.float32).view(np.uint32)], axis=1)
        counts = np.concatenate([ents, pairs]).astype(np.int64)
        return torch.from_numpy(send_slot), torch.from_numpy(ent.view(np.int32).reshape(-1).copy()), counts

    def combine(self, b, partials_in, n_pairs_out):
        csr = b.csr
        kp = self.kp
        part = soa_to_rows(partials_in.numpy(), kp).astype(np.float64)
        poff = np.concatenate([[0], np.cumsum(b.pairs_out)])
        B = csr.n_rows
        S = np.zeros((B, kp))
        vv = np.zeros(B)
        wx = np.zeros(B)
        for o in range(self.R):  # owner order
            ix = b.pairidx[:, o]
            m = ix >= 0
            rows = part[poff[o] + ix[m]]
            S[m] += rows[:, :kp]
            vv[m] += rows[:, kp]
            wx[m] += rows[:, kp + 1]
        yhat = 0.5 * (np.sum(S * S, axis=1) - vv) + wx + self.w0
        has = (b.pairidx >= 0).any(axis=1)  # a row with a pair (every entry outside the model: none)
        d = (yhat - csr.label)[has]
        b.loss = (float(np.sum(d * d)), int(has.sum()))
        out = np.zeros((int(n_pairs_out), kp + 2), dtype=np.float64)
        for o in range(self.R):
            ix = b.pairidx[:, o]
            m = ix >= 0
            out[poff[o] + ix[m], :kp] = S[m]
            out[poff[o] + ix[m], kp] = yhat[m] - csr.label[m]  # r, formed in fp64
            out[poff[o] + ix[m], kp + 1] = yhat[m]
        return torch.from_numpy(rows_to_soa(out, kp))

    def combine_exact(self, b, vec, sc, label=None):
        """The combine of arbitrary given partials, for a check of the kernel word by word: vec [Ps][kp]
        and sc [Ps][2] (fp32 or fp64 words, the pairs in owner blocks as route numbered them).
        Returns a CombineRef over the batch's samples: S, the fp64 sum in owner order rounded once to fp32
        (what every pair of the sample must get, bit for bit); yhat and r = yhat - label as np.longdouble
        (the squares and the sums carried in it, nothing rounded to fp32); and the magnitudes an error bound
        needs: sum_a2 = sum of the squared S columns, abs_vv = sum over owners of |sum v^2 x^2|, abs_wx
        likewise; pair_sample [Ps]: the sample of every pair."""
        kp, B, L = self.kp, b.csr.n_rows, np.longdouble
        vec = np.asarray(vec).reshape(-1, kp).astype(np.float64)
        sc = np.asarray(sc).reshape(-1, 2).astype(np.float64)
        label = b.csr.label if label is None else np.asarray(label, dtype=np.float64)
        poff = np.concatenate([[0], np.cumsum(b.pairs_out)])
        assert len(vec) == len(sc) == poff[-1]
        S = np.zeros((B, kp))
        vv, wx, avv, awx = (np.zeros(B, dtype=L) for _ in range(4))
        pair_sample = np.full(int(poff[-1]), -1, dtype=np.int64)
        for o in range(self.R):  # owner order, fp64 adds: nothing is reassociated
            ix = b.pairidx[:, o]
            m = ix >= 0
            p = poff[o] + ix[m]
            S[m] += vec[p]
            vv[m] += sc[p, 0]
            wx[m] += sc[p, 1]
            avv[m] += np.abs(sc[p, 0])
            awx[m] += np.abs(sc[p, 1])
            pair_sample[p] = np.nonzero(m)[0]
        assert (pair_sample >= 0).all()
        a2 = (S.astype(L) ** 2).sum(axis=1)
        yhat = L(0.5) * (a2 - vv) + wx + L(self.w0)
        return CombineRef(S.astype(np.float32), yhat, yhat - label.astype(L), a2, avv, awx, pair_sample,
                          (b.pairidx >= 0).any(axis=1))

    # owner -----------------------------------------------------------------------
    def owner_forward_exact(self, recv_slot, recv_ent, src_entries, src_pairs):
        """The owner's partial sums of received entries, for a check of the kernel word by word.  The
        pair of an entry is its source's pair offset plus the local index it carries (the wire's rule,
        not a guess from where the index changes).  Returns (vec [P][kp], sc [P][2], abs_vec, abs_sc,
        n [P]) as np.longdouble: the three sums {sum v x | sum v^2 x^2, sum w x} per pair, the sums of
        their terms' absolute values, and the pair's entries.  Table rows absent from the model
        contribute nothing."""
        L = np.longdouble
        slots = np.asarray(recv_slot).astype(np.int64).reshape(-1)
        ent = np.ascontiguousarray(np.asarray(recv_ent)).view(np.uint32).reshape(-1, 2)
        src_entries, src_pairs = np.asarray(src_entries, dtype=np.int64), np.asarray(src_pairs, dtype=np.int64)
        n, P = len(slots), int(src_pairs.sum())
        assert n == int(src_entries.sum()) == len(ent)
        vec, avec = np.zeros((P, self.kp), dtype=L), np.zeros((P, self.kp), dtype=L)
        sc, asc = np.zeros((P, 2), dtype=L), np.zeros((P, 2), dtype=L)
        cnt = np.zeros(P, dtype=np.int64)
        if n == 0:
            return vec, sc, avec, asc, cnt
        pbase = np.concatenate([[0], np.cumsum(src_pairs)])
        pair = pbase[np.repeat(np.arange(self.R), src_entries)] + ent[:, 0].astype(np.int64)
        x = ent[:, 1].view(np.float32).astype(L)
        assert (np.diff(pair) >= 0).all() and pair[0] == 0 and pair[-1] == P - 1 and (np.diff(pair) <= 1).all()
        start = np.nonzero(np.diff(pair, prepend=-1))[0]  # every pair's first entry
        here = self.present[slots]
        V = np.where(here[:, None], self.V[slots], 0.0).astype(L)
        w = np.where(here, self.w[slots], 0.0).astype(L)
        tv = V * x[:, None]
        tq = (V * V).sum(axis=1) * x * x
        tw = w * x
        vec[:, : self.k] = np.add.reduceat(tv, start, axis=0)
        avec[:, : self.k] = np.add.reduceat(np.abs(tv), start, axis=0)
        sc[:, 0], sc[:, 1] = np.add.reduceat(tq, start), np.add.reduceat(tw, start)
        asc[:, 0], asc[:, 1] = np.add.reduceat(np.abs(tq), start), np.add.reduceat(np.abs(tw), start)
        cnt[:] = np.diff(start, append=n)
        return vec, sc, avec, asc, cnt

    def owner_prepare(self, b, recv_slot, recv_ent, src_entries, src_pairs):
        b.recv_in = (recv_slot.clone(), recv_ent.clone(), np.asarray(src_entries), np.asarray(src_pairs))

    def owner_forward(self, b, n_pairs_in):
        recv_slot, recv_ent, src_entries, src_pairs = b.recv_in
        slots = recv_slot.numpy().astype(np.int64)
        ent = recv_ent.numpy().view(np.uint32).reshape(-1, 2)
        s, x = ent[:, 0].astype(np.int64), ent[:, 1].view(np.float32).astype(np.float64)
        n = len(slots)
        src = np.repeat(np.arange(self.R), src_entries)
        head = np.ones(n, dtype=bool)
        head[1:] = (s[1:] != s[:-1]) | (src[1:] != src[:-1])
        pair = np.cumsum(head) - 1
        P = int(head.sum())
        assert P == int(np.sum(src_pairs)) == n_pairs_in
        V, w = self.V[slots], self.w[slots]
        part = np.zeros((P, self.kp + 2))
        np.add.at(part[:, : self.k], pair, V * x[:, None])
        np.add.at(part[:, self.kp], pair, np.sum(V * V, axis=1) * x * x)
        np.add.at(part[:, self.kp + 1], pair, w * x)
        b.recv = (slots, x, pair)
        return torch.from_numpy(rows_to_soa(part, self.kp))

    def owner_update(self, b, s_recv, t, step_size, reg_param, global_rows):
        if global_rows == 0:
            return 1
        slots, x, pair = b.recv
        Srow = soa_to_rows(s_recv.numpy(), self.kp).astype(np.float64)
        S, r, yhat = Srow[pair, : self.k], Srow[pair, self.kp], Srow[pair, self.kp + 1]
        eta = step_size / math.sqrt(t)
        lam = eta * reg_param
        V = self.V[slots]
        gw = (x - 1.0) * yhat + r  # x * yhat - y with y = yhat - r (SGD.scala:145)
        gv = (S * x[:, None] - V * x[:, None] * x[:, None]) * r[:, None]
        GW = np.zeros(self.rows)
        GV = np.zeros((self.rows, self.k))
        np.add.at(GW, slots, gw)
        np.add.at(GV, slots, gv)
        touched = np.unique(slots)
        w_new, V_new = self.w.copy(), self.V.copy()
        w_new[touched] = self.w[touched] - (GW[touched] / global_rows) * eta
        V_new[touched] = self.V[touched] - GV[touched] * (eta / global_rows)
        pres = self.present.copy()
        pres[touched] = True
        self.w[pres] = np.sign(w_new[pres]) * np.maximum(0.0, np.abs(w_new[pres]) - lam)
        self.V[pres] = np.sign(V_new[pres]) * np.maximum(0.0, np.abs(V_new[pres]) - lam)
        self.present = pres
        self.stats = (b.loss[0], b.loss[1], len(touched))
        return 0

    def last_stats(self):
        return self.stats


class NumpyReplEngine:
    """TEST INFRASTRUCTURE: the replicated phase functions (fm_repl_grad / fm_repl_apply) in
    NumPy with the same fp32 gradient buffer layout [F][kp + 4]."""

    def __init__(self, num_features, k, w0=0.0):
        self.device = torch.device("cpu")
        self.F, self.k, self.w0 = num_features, k, w0
        self.kp = (k + 3) // 4 * 4
        self.width = self.kp + 4
        self.w = np.zeros(num_features)
        self.V = np.zeros((num_features, k))
        self.present = np.zeros(num_features, dtype=bool)
        self.stats = (0.0, 0, 0)

    def batch(self, csr):
        return NpBatch(csr)

    def load_tables(self, ids, w, V):
        ids = np.asarray(ids, dtype=np.int64)
        self.w[ids] = w
        self.V[ids] = np.asarray(V).reshape(len(ids), self.k)
        self.present[ids] = True

    def export_tables(self):
        ids = np.nonzero(self.present)[0]
        return ids.astype(np.int32), self.w[ids], self.V[ids]

    def grad_phase(self, b):
        csr = b.csr
        g = np.zeros((self.F, self.width))
        self.loss = (0.0, 0)
        if csr.n_rows:
            ids = csr.col.astype(np.int64)
            x = csr.val
            srow = np.repeat(np.arange(csr.n_rows), np.diff(csr.row_ptr))
            V, w = self.V[ids], self.w[ids]
            S = np.zeros((csr.n_rows, self.k))
            np.add.at(S, srow, V * x[:, None])
            vv = np.zeros(csr.n_rows)
            np.add.at(vv, srow, np.sum(V * V, axis=1) * x * x)
            wx = np.zeros(csr.n_rows)
            np.add.at(wx, srow, w * x)
            yhat = 0.5 * (np.sum(S * S, axis=1) - vv) + wx + self.w0
            has = np.diff(csr.row_ptr) > 0
            d = (yhat - csr.label)[has]
            self.loss = (float(np.sum(d * d)), int(has.sum()))
            r = (yhat - csr.label)[srow]
            np.add.at(g[:, : self.k], ids, (S[srow] * x[:, None] - V * x[:, None] * x[:, None]) * r[:, None])
            np.add.at(g[:, self.kp], ids, x * yhat[srow] - csr.label[srow])
            g[ids, self.kp + 1] = 1.0
        self.grad = torch.from_numpy(g.astype(np.float32).reshape(-1))
        return self.grad

    def apply(self, grad, t, step_size, reg_param, global_rows):
        if global_rows == 0:
            return 1
        G = grad.numpy().reshape(self.F, self.width).astype(np.float64)
        touched = np.nonzero(G[:, self.kp + 1] > 0)[0]
        eta = step_size / math.sqrt(t)
        lam = eta * reg_param
        w_new, V_new = self.w.copy(), self.V.copy()
        w_new[touched] -= (G[touched, self.kp] / global_rows) * eta
        V_new[touched] -= G[touched, : self.k] * (eta / global_rows)
        pres = self.present.copy()
        pres[touched] = True
        self.w[pres] = np.sign(w_new[pres]) * np.maximum(0.0, np.abs(w_new[pres]) - lam)
        self.V[pres] = np.sign(V_new[pres]) * np.maximum(0.0, np.abs(V_new[pres]) - lam)
        self.present = pres
        self.stats = (self.loss[0], self.loss[1], len(touched))
        return 0

    def last_stats(self):
        return self.stats
