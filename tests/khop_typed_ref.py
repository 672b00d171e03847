"""numpy statement of khop_typed (include/ggms.h, GGMS_KHOP_TYPED): the segments of a type-sorted list, khop_labor's
selection per segment under one salt, one layer, and the batch chain on top of khop_labor_ref's numbering."""
import numpy as np

import khop_labor_ref as labor


def boundaries(types, R):
    """b_0 .. b_R of a (non-decreasing) list of types: b_r = the number of entries with type < r."""
    return np.searchsorted(np.asarray(types, dtype=np.int64), np.arange(R + 1), side="left")


def select_positions(ids, types, type_fanout, salt):
    """(positions, types) of one seed's selection, ascending position: from every segment [b_r, b_{r+1}) khop_labor's
    bottom-k with fanout k_r, all segments under the same salt."""
    R = len(type_fanout)
    b = boundaries(types, R)
    pos, typ = [], []
    for r in range(R):
        k = int(type_fanout[r])
        if k == 0 or b[r + 1] == b[r]:
            continue
        p = b[r] + labor.select_positions(ids[b[r]:b[r + 1]], k, salt)
        pos.append(p)
        typ.append(np.full(p.size, r, np.uint8))
    if not pos:
        return np.zeros(0, np.int64), np.zeros(0, np.uint8)
    return np.concatenate(pos).astype(np.int64), np.concatenate(typ)


def sample_layer(ip, ix, et, seeds, type_fanout, salt):
    """(seed position, out_src, out_dst, out_pos, out_type) of every sampled edge: seeds in input order, positions
    ascending in a seed; out_pos = the edge's position in ix."""
    where, src, dst, pos, typ = [], [], [], [], []
    for j, s in enumerate(np.asarray(seeds, dtype=np.int64)):
        b, e = int(ip[s]), int(ip[s + 1])
        p, t = select_positions(ix[b:e], et[b:e], type_fanout, salt)
        where.append(np.full(p.size, j, np.int64))
        src.append(np.full(p.size, s, np.uint32))
        dst.append(ix[b:e][p].astype(np.uint32))
        pos.append((b + p).astype(np.uint32))
        typ.append(t)
    if not where:
        z = np.zeros(0, np.uint32)
        return np.zeros(0, np.int64), z, z, z, np.zeros(0, np.uint8)
    return np.concatenate(where), np.concatenate(src), np.concatenate(dst), np.concatenate(pos), np.concatenate(typ)


def sample_batch(ip, ix, et, seeds, type_fanouts, salt):
    """ggms_sample_batch_typed: dict(layers=[{row, col, eid, etype, num_src, num_dst}] by layer id, input_nodes,
    seed_local).  type_fanouts[i] = the fanouts of layer i.  Numbering as khop_labor_ref.sample_batch."""
    seeds = np.asarray(seeds, dtype=np.uint32)
    local, n2o = {}, []

    def enter(ids):
        out = np.empty(len(ids), np.uint32)
        for e, v in enumerate(ids.tolist()):
            if v not in local:
                local[v] = len(n2o)
                n2o.append(v)
            out[e] = local[v]
        return out

    seed_local = enter(seeds)
    L = len(type_fanouts)
    layers = [None] * L
    frontier, col_of = seeds, seed_local
    for i in range(L - 1, -1, -1):
        where, _, dst, pos, typ = sample_layer(ip, ix, et, frontier, type_fanouts[i], labor.layer_salt(salt, i))
        col = col_of[where].astype(np.uint32) if where.size else np.zeros(0, np.uint32)
        row = enter(dst)
        layers[i] = dict(row=row, col=col, eid=pos, etype=typ, num_src=len(n2o), num_dst=len(frontier))
        frontier = np.array(n2o, dtype=np.uint32)
        col_of = np.arange(len(n2o), dtype=np.uint32)
    return dict(layers=layers, input_nodes=np.array(n2o, dtype=np.uint32), seed_local=seed_local)


def filtered_csr(ip, ix, et, r):
    """The CSR of the edges of type r, and for each of its positions the position in the original."""
    keep = np.asarray(et) == r
    kept_before = np.concatenate([[0], np.cumsum(keep)])
    fip = kept_before[np.asarray(ip, dtype=np.int64)].astype(np.uint32)
    return fip, np.asarray(ix)[keep], np.flatnonzero(keep).astype(np.uint32)


def sorted_types(ip, rng, R, weights=None):
    """Random types below R (drawn with `weights`), non-decreasing inside every list."""
    ip = np.asarray(ip, dtype=np.int64)
    E = int(ip[-1])
    t = rng.choice(R, size=E, p=weights).astype(np.uint8)
    owner = np.repeat(np.arange(ip.size - 1), np.diff(ip))
    return t[np.lexsort((t, owner))]


def segment_graph(lists):
    """A CSR from explicit lists: lists[v] = the segment lengths of node v by type.  Neighbour ids are an aperiodic
    function of the position (with repeats across nodes, so seeds share picks).  -> (indptr, indices, edge_type)."""
    deg = np.array([int(sum(seg)) for seg in lists], dtype=np.int64)
    ip = np.zeros(len(lists) + 1, np.uint32)
    ip[1:] = np.cumsum(deg)
    E = int(ip[-1])
    ix = ((np.arange(E, dtype=np.uint64) * np.uint64(2654435761)) % np.uint64(100003)).astype(np.uint32)
    et = np.concatenate([np.repeat(np.arange(len(seg)), seg) for seg in lists] + [np.zeros(0, np.int64)]).astype(np.uint8)
    return ip, ix, et
