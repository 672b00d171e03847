"""numpy statement of khop_temporal (include/ggms.h, GGMS_KHOP_TEMPORAL): the eligible prefix, the two picks, one layer,
and the batch chain with its cut-off rule (a node's cut is the minimum of the times of the seeds that reach it) on top
of khop_labor_ref's numbering."""
import numpy as np

import khop_labor_ref as labor

INF = 0xFFFFFFFF  # "no cut": every edge with a time below 2^32 - 1 is eligible
UNIFORM, RECENT = 0, 1


def eligible(times, cut):
    """e = the number of entries of a (non-decreasing) list of times that lie strictly before `cut`."""
    return int(np.searchsorted(np.asarray(times, dtype=np.uint32), np.uint32(cut), side="left"))


def select_positions(ids, times, cut, fanout, salt, pick):
    """The selected positions of one seed's list, ascending: among the first e (time < cut), khop_labor's bottom-k
    (UNIFORM) or the last min(fanout, e) (RECENT)."""
    e = eligible(times, cut)
    if pick == RECENT:
        return np.arange(e - min(fanout, e), e)
    return labor.select_positions(ids[:e], fanout, salt)


def sample_layer(ip, ix, et, seeds, cuts, fanout, salt, pick=UNIFORM):
    """(seed position, out_src, out_dst, out_pos) of every sampled edge: seeds in input order, positions ascending in a
    seed; out_pos = the edge's position in ix."""
    where, src, dst, pos = [], [], [], []
    for j, (s, c) in enumerate(zip(np.asarray(seeds, dtype=np.int64), np.asarray(cuts, dtype=np.int64))):
        b, e = int(ip[s]), int(ip[s + 1])
        p = select_positions(ix[b:e], et[b:e], c, fanout, salt, pick)
        where.append(np.full(p.size, j, np.int64))
        src.append(np.full(p.size, s, np.uint32))
        dst.append(ix[b:e][p].astype(np.uint32))
        pos.append((b + p).astype(np.uint32))
    if not where:
        z = np.zeros(0, np.uint32)
        return np.zeros(0, np.int64), z, z, z
    return np.concatenate(where), np.concatenate(src), np.concatenate(dst), np.concatenate(pos)


def sample_batch(ip, ix, et, seeds, seed_time, fanouts, salt, pick=UNIFORM):
    """ggms_sample_batch_temporal: dict(layers=[{row, col, eid, num_src, num_dst, cut_at_start}] by layer id,
    input_nodes, node_cut, seed_local).  Numbering as khop_labor_ref.sample_batch; cut_at_start[local id] = the cut of
    every frontier node as the layer found it (the snapshot it sampled with), node_cut the final cuts."""
    seeds = np.asarray(seeds, dtype=np.uint32)
    seed_time = np.asarray(seed_time, dtype=np.uint32)
    local, n2o, cut = {}, [], {}

    def enter(ids):
        out = np.empty(len(ids), np.uint32)
        for e, v in enumerate(ids.tolist()):
            if v not in local:
                local[v] = len(n2o)
                n2o.append(v)
            out[e] = local[v]
        return out

    for v, t in zip(seeds.tolist(), seed_time.tolist()):
        cut[v] = min(cut.get(v, INF), t)
    seed_local = enter(seeds)
    L = len(fanouts)
    layers = [None] * L
    frontier, col_of = seeds, seed_local
    for i in range(L - 1, -1, -1):
        c_f = np.array([cut[v] for v in frontier.tolist()], dtype=np.uint32)  # the snapshot
        start = np.full(len(n2o), INF, np.uint32)  # by local id (repeated raw seeds share their cut)
        start[col_of] = c_f
        where, _, dst, pos = sample_layer(ip, ix, et, frontier, c_f, fanouts[i], labor.layer_salt(salt, i), pick)
        for t, c in zip(dst.tolist(), c_f[where].tolist()):
            cut[t] = min(cut.get(t, INF), c)
        col = col_of[where].astype(np.uint32) if where.size else np.zeros(0, np.uint32)
        row = enter(dst)
        layers[i] = dict(row=row, col=col, eid=pos, num_src=len(n2o), num_dst=len(frontier), cut_at_start=start)
        frontier = np.array(n2o, dtype=np.uint32)
        col_of = np.arange(len(n2o), dtype=np.uint32)
    return dict(layers=layers, input_nodes=np.array(n2o, dtype=np.uint32), seed_local=seed_local,
                node_cut=np.array([cut[v] for v in n2o], dtype=np.uint32))


def filtered_csr(ip, ix, et, T):
    """The CSR of the edges with time < T, and for each of its positions the position in the original."""
    keep = np.asarray(et) < T
    kept_before = np.concatenate([[0], np.cumsum(keep)])
    fip = kept_before[np.asarray(ip, dtype=np.int64)].astype(np.uint32)
    return fip, np.asarray(ix)[keep], np.flatnonzero(keep).astype(np.uint32)


def sorted_times(ip, rng, lo=1, hi=1000):
    """Random times, non-decreasing inside every list (with repeats)."""
    ip = np.asarray(ip, dtype=np.int64)
    E = int(ip[-1])
    t = rng.randint(lo, hi, E).astype(np.uint32)
    owner = np.repeat(np.arange(ip.size - 1), np.diff(ip))
    return t[np.lexsort((t, owner))]
