"""ggms_gather_typed (include/ggms.h) restated: once in numpy, once as plain loops (tests/test_typed_feat_host.py holds the
two equal).  The statement the GPU tests compare with, bit for bit.  Shares no code with xgnn_amd/csrc/gather_typed.hip;
the conversions are those of tests/feat_formats.py.

A table set is a list with one entry per node type: None (the type has no table, dim == 0) or a dict
    bits        (rows, dim) raw bits of the table (np.uint32 for F32, np.uint16 for F16 / BF16)
    src, out    ggms_dtype codes of the table and of what is delivered
    first_node  the type's first node id, used when there is no rank table
"""
import numpy as np

import feat_formats as ff

ES = {ff.F32: 4, ff.F16: 2, ff.BF16: 2}


def row_bytes(tab):
    """rb_t: the bytes of an output row (0 for a type without a table)."""
    return 0 if tab is None else tab["bits"].shape[1] * ES[tab["out"]]


def out_bytes(tables, max_nodes):
    """ggms_gather_typed_out_bytes"""
    return max_nodes * max([row_bytes(t) for t in tables] + [0]) + 16 * len(tables)


def groups(base, max_nodes):
    """b[t] = max over u <= t of min(base[u], max_nodes) -- nothing behind max_nodes, no group overlaps another."""
    return np.maximum.accumulate(np.minimum(np.asarray(base, np.uint64), max_nodes)).astype(np.int64)


def offsets(tables, base, max_nodes):
    """off[0] = 0, off[t + 1] = round_up(off[t] + cnt_t x rb_t, 16)"""
    b = groups(base, max_nodes)
    off = [0]
    for t, tab in enumerate(tables):
        off.append((off[t] + int(b[t + 1] - b[t]) * row_bytes(tab) + 15) // 16 * 16)
    return np.array(off, np.uint64)


def gather_typed(tables, typed_nodes, base, max_nodes, row_of_node=None, num_node=None):
    """-> (out, off): out holds off[T] bytes (np.uint8), off the T + 1 offsets (np.uint64)."""
    typed_nodes = np.asarray(typed_nodes, np.uint32)
    b = groups(base, max_nodes)
    off = offsets(tables, base, max_nodes)
    if num_node is None:
        num_node = len(row_of_node) if row_of_node is not None else 1 << 40
    out = np.zeros(int(off[-1]), np.uint8)  # pad bytes and zero rows: zero
    for t, tab in enumerate(tables):
        cnt = int(b[t + 1] - b[t])
        if tab is None or cnt == 0:
            continue
        v = typed_nodes[b[t]:b[t] + cnt].astype(np.int64)
        ok = v < num_node
        row = np.zeros(cnt, np.int64)
        if row_of_node is not None:
            row[ok] = np.asarray(row_of_node, np.uint32)[v[ok]]
        else:
            row = v - int(tab["first_node"])
        ok &= (row >= 0) & (row < tab["bits"].shape[0])
        dim = tab["bits"].shape[1]
        block = np.zeros((cnt, dim), ff.BITS[tab["out"]])
        got = tab["bits"][row[ok]]
        block[ok] = got if tab["src"] == tab["out"] else ff.convert_bits(np.ascontiguousarray(got), tab["src"], tab["out"])
        o = int(off[t])
        out[o:o + cnt * row_bytes(tab)] = block.view(np.uint8).reshape(-1)
    return out, off


def gather_typed_loops(tables, typed_nodes, base, max_nodes, row_of_node=None, num_node=None):
    T = len(tables)
    b, run = [], 0
    for u in range(T + 1):
        run = max(run, min(int(base[u]), max_nodes))
        b.append(run)
    if num_node is None:
        num_node = len(row_of_node) if row_of_node is not None else 1 << 40
    off = [0]
    for t in range(T):
        end = off[t] + (b[t + 1] - b[t]) * row_bytes(tables[t])
        off.append(end + (-end) % 16)
    out = [0] * off[T]
    for t, tab in enumerate(tables):
        if tab is None:
            continue
        dim, es = tab["bits"].shape[1], ES[tab["out"]]
        for j in range(b[t + 1] - b[t]):
            v = int(typed_nodes[b[t] + j])
            if v >= num_node:
                continue
            row = int(row_of_node[v]) if row_of_node is not None else v - int(tab["first_node"])
            if row < 0 or row >= tab["bits"].shape[0]:
                continue
            for c in range(dim):
                one = tab["bits"][row:row + 1, c:c + 1]
                if tab["src"] != tab["out"]:
                    one = ff.convert_bits(np.ascontiguousarray(one), tab["src"], tab["out"])
                x = int(one[0, 0])
                at = off[t] + (j * dim + c) * es
                for k in range(es):  # little endian
                    out[at + k] = (x >> (8 * k)) & 0xFF
    return np.array(out, np.uint8), np.array(off, np.uint64)


def hashed_bits(t, rows, dim, dt, first_row=0):
    """An aperiodic table: element (r, c) of type t is a hash of (t, r, c), so a row from the wrong type, rank or column
    shows.  F32 tables keep finite-or-not as it falls; the exponent is left alone."""
    r = (np.arange(first_row, first_row + rows, dtype=np.uint64)[:, None] + 1) * np.uint64(0x9E3779B97F4A7C15)
    c = (np.arange(dim, dtype=np.uint64)[None, :] + 1) * np.uint64(0xC2B2AE3D27D4EB4F)
    with np.errstate(over="ignore"):
        h = (r ^ c) + np.uint64(t + 1) * np.uint64(0x165667B19E3779F9)
        h ^= h >> np.uint64(29)
        h *= np.uint64(0xBF58476D1CE4E5B9)
        h ^= h >> np.uint64(32)
    return (h & np.uint64(0xFFFFFFFF if dt == ff.F32 else 0xFFFF)).astype(ff.BITS[dt])
