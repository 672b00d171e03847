"""ggms_hetero_nodes / ggms_hetero_edges (include/ggms.h) restated in plain numpy: the statement the GPU tests compare with,
bit for bit.  Shares no code with xgnn_amd/csrc/hetero.hip."""
import numpy as np

EMPTY = 0xFFFFFFFF
NO_TYPE = 0xFF


def hetero_nodes(node_type, num_type, nodes, cuts=()):
    """nodes: the n entries that count.  -> dict(ntype, local, slot, typed_nodes, base, cut_counts); typed_nodes holds
    base[T] entries, cut_counts has shape (len(cuts), T)."""
    node_type = np.asarray(node_type, np.uint8)
    nodes = np.asarray(nodes, np.uint32)
    T, n = int(num_type), nodes.size
    ntype = np.full(n, NO_TYPE, np.uint8)
    ok = nodes < node_type.size
    ntype[ok] = node_type[nodes[ok]]
    ntype[ntype >= T] = NO_TYPE
    valid = ntype != NO_TYPE
    local = np.full(n, EMPTY, np.uint32)
    base = np.zeros(T + 1, np.uint32)
    for t in range(T):
        at = np.flatnonzero(ntype == t)
        local[at] = np.arange(at.size, dtype=np.uint32)
        base[t + 1] = base[t] + at.size
    slot = np.full(n, EMPTY, np.uint32)
    slot[valid] = base[ntype[valid]] + local[valid]
    typed = np.zeros(int(base[T]), np.uint32)
    typed[slot[valid]] = nodes[valid]
    cut_counts = np.zeros((len(cuts), T), np.uint32)
    for k, c in enumerate(cuts):
        head = ntype[:min(int(c), n)]
        cut_counts[k] = np.bincount(head[head != NO_TYPE], minlength=T)[:T]
    return dict(ntype=ntype, local=local, slot=slot, typed_nodes=typed, base=base, cut_counts=cut_counts)


def hetero_edges(rows, cols, eids, etypes, num_rel, local):
    """Per layer the E entries that count (eids: None, or a list).  -> (out_rows, out_cols, out_eids or None, offsets):
    the outputs hold offsets[i][R] entries each, offsets has shape (L, R + 1)."""
    R = int(num_rel)
    local = np.asarray(local, np.uint32)

    def look(ids):
        out = np.full(ids.size, EMPTY, np.uint32)
        ok = ids < local.size
        out[ok] = local[ids[ok]]
        return out

    out_rows, out_cols, out_eids = [], [], []
    offsets = np.zeros((len(rows), R + 1), np.uint32)
    for i, (row, col, et) in enumerate(zip(rows, cols, etypes)):
        et = np.asarray(et, np.uint8)
        kept = np.flatnonzero(et < R)
        order = kept[np.argsort(et[kept], kind="stable")]
        offsets[i, 1:] = np.cumsum(np.bincount(et[kept], minlength=R)[:R])
        out_rows.append(look(np.asarray(row, np.uint32)[order]))
        out_cols.append(look(np.asarray(col, np.uint32)[order]))
        if eids is not None:
            out_eids.append(np.asarray(eids[i], np.uint32)[order])
    return out_rows, out_cols, (out_eids if eids is not None else None), offsets


# ---- the same statements as double loops (tests/test_hetero_host.py holds the two equal) -------------------------------
def hetero_nodes_loops(node_type, num_type, nodes, cuts=()):
    T, n = int(num_type), len(nodes)
    ntype = [NO_TYPE] * n
    for i, v in enumerate(nodes):
        if int(v) < len(node_type) and int(node_type[int(v)]) < T:
            ntype[i] = int(node_type[int(v)])
    local = [EMPTY] * n
    for i in range(n):
        if ntype[i] != NO_TYPE:
            local[i] = sum(1 for j in range(i) if ntype[j] == ntype[i])
    base = [sum(1 for i in range(n) if ntype[i] < t) for t in range(T + 1)]
    slot = [EMPTY if ntype[i] == NO_TYPE else base[ntype[i]] + local[i] for i in range(n)]
    typed = [0] * base[T]
    for i in range(n):
        if slot[i] != EMPTY:
            typed[slot[i]] = int(nodes[i])
    cut_counts = [[sum(1 for i in range(min(int(c), n)) if ntype[i] == t) for t in range(T)] for c in cuts]
    return dict(ntype=np.array(ntype, np.uint8), local=np.array(local, np.uint32), slot=np.array(slot, np.uint32),
                typed_nodes=np.array(typed, np.uint32), base=np.array(base, np.uint32),
                cut_counts=np.array(cut_counts, np.uint32).reshape(len(cuts), T))


def hetero_edges_loops(rows, cols, eids, etypes, num_rel, local):
    R = int(num_rel)
    out_rows, out_cols, out_eids, offsets = [], [], [], []
    for i in range(len(rows)):
        et = [int(x) for x in etypes[i]]
        E = len(et)
        off = [sum(1 for e in range(E) if et[e] < r) for r in range(R + 1)]
        o_r, o_c, o_e = [0] * off[R], [0] * off[R], [0] * off[R]
        for e in range(E):
            if et[e] >= R:
                continue
            q = off[et[e]] + sum(1 for f in range(e) if et[f] == et[e])
            r, c = int(rows[i][e]), int(cols[i][e])
            o_r[q] = int(local[r]) if r < len(local) else EMPTY
            o_c[q] = int(local[c]) if c < len(local) else EMPTY
            if eids is not None:
                o_e[q] = int(eids[i][e])
        out_rows.append(np.array(o_r, np.uint32))
        out_cols.append(np.array(o_c, np.uint32))
        out_eids.append(np.array(o_e, np.uint32))
        offsets.append(off)
    return out_rows, out_cols, (out_eids if eids is not None else None), np.array(offsets, np.uint32).reshape(len(rows), R + 1)
