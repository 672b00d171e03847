"""numpy statement of khop_typed_temporal (include/ggms.h, GGMS_KHOP_TYPED_TEMPORAL): khop_typed_ref's segments with
khop_temporal_ref's selection on each, one layer, and khop_temporal_ref's batch chain with a fanout row per layer."""
import numpy as np

import khop_labor_ref as labor
import khop_temporal_ref as temporal
import khop_typed_ref as typed

INF, UNIFORM, RECENT = temporal.INF, temporal.UNIFORM, temporal.RECENT


def select_positions(ids, types, times, cut, type_fanout, salt, pick):
    """(positions, types) of one seed's selection: from every segment, among its entries with time < cut, khop_labor's
    bottom-k_r under the one salt (UNIFORM) or the last min(k_r, e_r) (RECENT)."""
    b = typed.boundaries(types, len(type_fanout))
    pos, typ = [np.zeros(0, np.int64)], [np.zeros(0, np.uint8)]
    for r, k in enumerate(type_fanout):
        if int(k) and b[r + 1] > b[r]:
            p = b[r] + temporal.select_positions(ids[b[r]:b[r + 1]], times[b[r]:b[r + 1]], cut, int(k), salt, pick)
            pos.append(p.astype(np.int64))
            typ.append(np.full(p.size, r, np.uint8))
    return np.concatenate(pos), np.concatenate(typ)


def sample_layer(ip, ix, et, tm, seeds, cuts, type_fanout, salt, pick=UNIFORM):
    """(seed position, out_src, out_dst, out_pos, out_type) of every sampled edge, as khop_typed_ref.sample_layer."""
    where, src, dst, pos, typ = ([np.zeros(0, dt)] for dt in (np.int64, np.uint32, np.uint32, np.uint32, np.uint8))
    for j, (s, c) in enumerate(zip(np.asarray(seeds, dtype=np.int64), np.asarray(cuts, dtype=np.int64))):
        b, e = int(ip[s]), int(ip[s + 1])
        p, t = select_positions(ix[b:e], et[b:e], tm[b:e], c, type_fanout, salt, pick)
        where.append(np.full(p.size, j, np.int64))
        src.append(np.full(p.size, s, np.uint32))
        dst.append(ix[b:e][p].astype(np.uint32))
        pos.append((b + p).astype(np.uint32))
        typ.append(t)
    return tuple(np.concatenate(a) for a in (where, src, dst, pos, typ))


def sample_batch(ip, ix, et, tm, seeds, seed_time, type_fanouts, salt, pick=UNIFORM):
    """ggms_sample_batch_typed_temporal: khop_temporal_ref.sample_batch's dict, every layer with its `etype`."""
    seeds, seed_time = np.asarray(seeds, dtype=np.uint32), np.asarray(seed_time, dtype=np.uint32)
    local, n2o, cut = {}, [], {}

    def enter(ids):
        for v in ids.tolist():
            if v not in local:
                local[v] = len(n2o)
                n2o.append(v)
        return np.array([local[v] for v in ids.tolist()], dtype=np.uint32)

    for v, t in zip(seeds.tolist(), seed_time.tolist()):
        cut[v] = min(cut.get(v, INF), t)
    seed_local = enter(seeds)
    layers = [None] * len(type_fanouts)
    frontier, col_of = seeds, seed_local
    for i in range(len(type_fanouts) - 1, -1, -1):
        c_f = np.array([cut[v] for v in frontier.tolist()], dtype=np.uint32)  # the layer's snapshot
        where, _, dst, pos, typ = sample_layer(ip, ix, et, tm, frontier, c_f, type_fanouts[i], labor.layer_salt(salt, i), pick)
        for t, c in zip(dst.tolist(), c_f[where].tolist()):
            cut[t] = min(cut.get(t, INF), c)
        col = col_of[where].astype(np.uint32)
        layers[i] = dict(row=enter(dst), col=col, eid=pos, etype=typ, num_src=len(n2o), num_dst=len(frontier), cut_at_start=c_f)
        frontier = np.array(n2o, dtype=np.uint32)
        col_of = np.arange(len(n2o), dtype=np.uint32)
    return dict(layers=layers, input_nodes=np.array(n2o, dtype=np.uint32), seed_local=seed_local,
                node_cut=np.array([cut[v] for v in n2o], dtype=np.uint32))


def sorted_times(ip, et, rng, lo=1, hi=1000):
    """Random times (with repeats), non-decreasing inside every (node, type) segment of a type-sorted CSR."""
    t = rng.randint(lo, hi, int(ip[-1])).astype(np.uint32)
    owner = np.repeat(np.arange(len(ip) - 1), np.diff(np.asarray(ip, dtype=np.int64)))
    return t[np.lexsort((t, et, owner))]
