"""ggms_edge_positions (include/ggms.h) in numpy: the definition, with no call into the library."""
import numpy as np

EMPTY = 0xFFFFFFFF


def first_position(indptr, indices, s, t):
    """The smallest p in s's list with indices[p] == t; EMPTY if there is none or s / t is no node.  `indices` needs
    slicing only (graphgen.SparseIndices will do)."""
    num_node = len(indptr) - 1
    s, t = int(s), int(t)
    if s >= num_node or t >= num_node:  # (EMPTY is no node either)
        return EMPTY
    a, b = int(indptr[s]), int(indptr[s + 1])
    hit = np.flatnonzero(np.asarray(indices[a:b]) == t)
    return a + int(hit[0]) if hit.size else EMPTY


def edge_positions(indptr, indices, rows, cols, id_map=None):
    """rows / cols: per layer the layer's edges (exactly n_i entries).  -> per layer the uint32 positions."""
    def glob(x):
        if id_map is None:
            return int(x)
        return int(id_map[x]) if int(x) < len(id_map) else EMPTY
    return [np.array([first_position(indptr, indices, glob(c), glob(r)) for r, c in zip(row, col)], np.uint32)
            for row, col in zip(rows, cols)]
