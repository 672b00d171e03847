"""ggms_induced_edges (include/ggms.h) restated in numpy: the yardstick of every induced-subgraph test.

  nodes[0, n)      the set, in the batch's order
  loc(v)           = min { j : nodes[j] == v } for ids v < num_node; an entry that is EMPTY or >= num_node owns nothing and
                   is nobody's target
  owner positions  j with loc(nodes[j]) == j (a repeated id: only its first position owns the list)
  edges, in order  for owner j ascending, for p = indptr[u] .. indptr[u + 1] - 1 ascending (u = nodes[j]): if w = indices[p]
                   has a loc, the edge (row = loc(w), col = j, eid = p)

`indices` is only sliced by list (indices[a:b]), so graphgen.SparseIndices serves too."""
import numpy as np

EMPTY = 0xFFFFFFFF


def first_positions(nodes, num_node):
    """(ids, loc): the distinct valid ids of `nodes`, ascending, and the first position of each."""
    nodes = np.asarray(nodes, dtype=np.uint32).astype(np.int64)
    pos = np.flatnonzero(nodes < num_node)
    ids, first = np.unique(nodes[pos], return_index=True)  # return_index: the first occurrence
    return ids, pos[first]


def induced_edges(indptr, indices, nodes, max_edges=None):
    """-> (row, col, eid, M, walked): uint32 arrays of min(M, max_edges) entries (all M without max_edges), M = the number
    of induced edges that exist, walked = the list entries of the owners."""
    num_node = len(indptr) - 1
    ids, loc = first_positions(nodes, num_node)
    rows, cols, eids = [], [], []
    walked = 0
    for k in np.argsort(loc, kind="stable"):  # owners by position
        u, j = int(ids[k]), int(loc[k])
        a, b = int(indptr[u]), int(indptr[u + 1])
        walked += b - a
        if b == a or ids.size == 0:
            continue
        w = np.asarray(indices[a:b]).astype(np.int64)
        at = np.minimum(np.searchsorted(ids, w), ids.size - 1)
        hit = ids[at] == w
        rows.append(loc[at[hit]])
        cols.append(np.full(int(hit.sum()), j, np.int64))
        eids.append(a + np.flatnonzero(hit))
    cat = lambda xs: (np.concatenate(xs) if xs else np.zeros(0, np.int64)).astype(np.uint32)
    row, col, eid = cat(rows), cat(cols), cat(eids)
    M = int(row.size)
    keep = M if max_edges is None else min(M, int(max_edges))
    return row[:keep], col[:keep], eid[:keep], M, walked
