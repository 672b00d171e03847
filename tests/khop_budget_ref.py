"""numpy statement of khop_budget (include/ggms.h, GGMS_KHOP_BUDGET): the candidates' weights and keys, the chosen set,
one layer, and the batch chain with khop_labor's dedup and numbering."""
import numpy as np

import khop_labor_ref as labor
import khop_labor_weighted_ref as lw

U = np.uint64
UNIFORM, LADIES = 0, 1


def contribution(deg, mode):
    """c_i of a seed of degree deg: 1, or LADIES' max(1, floor(2^40 / deg^2)) for deg < 2^20."""
    if mode == UNIFORM or deg == 0 or deg >= 1 << 20:
        return 1
    return max(1, (1 << 40) // (deg * deg))


def candidates(ip, ix, seeds, mode, salt):
    """(ids ascending, W, key32) of the M distinct neighbours of the frontier."""
    W = {}
    for s in np.asarray(seeds, dtype=np.int64).tolist():
        b, e = int(ip[s]), int(ip[s + 1])
        c = contribution(e - b, mode)
        for t in ix[b:e].tolist():
            W[t] = W.get(t, 0) + c
    t = np.array(sorted(W), dtype=U)
    w = np.array([W[v] for v in t.tolist()], dtype=U)
    E = lw.variate(labor.fmix32(t ^ U(salt)))
    return t, w, (E.astype(np.float32) / w.astype(np.float32)).astype(np.float32).view(np.uint32)


def sample_layer(ip, ix, seeds, budget, fanout, mode, salt):
    """(seed position, out_src, out_dst, out_pos, M, chosen) of one layer."""
    t, _, k32 = candidates(ip, ix, seeds, mode, salt)
    keep = np.argsort((k32.astype(U) << U(32)) | t)[:budget]  # every candidate if M <= budget
    key_of = dict(zip(t[keep].tolist(), k32[keep].tolist()))
    where, src, dst, pos = [np.zeros(0, np.int64)], [np.zeros(0, np.uint32)], [np.zeros(0, np.uint32)], [np.zeros(0, np.uint32)]
    for j, s in enumerate(np.asarray(seeds, dtype=np.int64).tolist()):
        b, e = int(ip[s]), int(ip[s + 1])
        ids = ix[b:e]
        p = np.array([q for q, v in enumerate(ids.tolist()) if v in key_of], dtype=np.int64)
        if p.size > fanout:
            k = np.array([key_of[v] for v in ids[p].tolist()], dtype=U)
            p = np.sort(p[np.argsort((k << U(32)) | p.astype(U))[:fanout]])
        where.append(np.full(p.size, j, np.int64))
        src.append(np.full(p.size, s, np.uint32))
        dst.append(ids[p].astype(np.uint32))
        pos.append((b + p).astype(np.uint32))
    return tuple(np.concatenate(x) for x in (where, src, dst, pos)) + (t.size, keep.size)


def sample_batch(ip, ix, seeds, fanouts, layer_nodes, mode, salt):
    """ggms_sample_batch_budget: khop_labor_ref.sample_batch's chain (first-occurrence numbering, layer L-1 from the raw
    seeds, every later one from all nodes seen so far, khop_labor's layer salts) with this sampler and `eid`."""
    seeds = np.asarray(seeds, dtype=np.uint32)
    local, n2o = {}, []

    def enter(ids):
        for v in ids.tolist():
            if v not in local:
                local[v] = len(n2o)
                n2o.append(v)
        return np.array([local[v] for v in ids.tolist()], np.uint32)

    col_of, frontier = enter(seeds), seeds
    layers = [None] * len(fanouts)
    for i in range(len(fanouts) - 1, -1, -1):
        where, _, dst, pos, _, _ = sample_layer(ip, ix, frontier, layer_nodes[i], fanouts[i], mode, labor.layer_salt(salt, i))
        layers[i] = dict(row=enter(dst), col=col_of[where].astype(np.uint32), eid=pos, num_src=len(n2o),
                         num_dst=len(frontier))
        frontier = np.array(n2o, dtype=np.uint32)
        col_of = np.arange(len(n2o), dtype=np.uint32)
    return dict(layers=layers, input_nodes=np.array(n2o, dtype=np.uint32))
