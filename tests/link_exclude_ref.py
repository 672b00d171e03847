"""numpy statement of ggms_drop_pair_edges (include/ggms.h): a set of (col, row) pairs and a boolean mask per layer.

col is the node whose list was read, row the sampled neighbour.  FORWARD drops (col, row) == (src[i], dst[i]), REVERSE
drops (col, row) == (dst[i], src[i]); a pair holding EMPTY matches nothing; every instance of a matching edge goes, the
kept edges keep their order."""
import numpy as np

FORWARD, REVERSE = 1, 2
EMPTY = 0xFFFFFFFF
WHICH_OF = {"none": 0, "self": FORWARD, "both": FORWARD | REVERSE}  # the engine's exclude_seed_edges values


def pair_set(pair_src, pair_dst, which):
    """The (col, row) pairs an edge must not be."""
    out = set()
    for s, d in zip(np.asarray(pair_src).view(np.uint32).tolist(), np.asarray(pair_dst).view(np.uint32).tolist()):
        if s == EMPTY or d == EMPTY:
            continue
        if which & FORWARD:
            out.add((s, d))
        if which & REVERSE:
            out.add((d, s))
    return out


def keep_mask(row, col, pairs):
    """keep[e] = the edge (col[e], row[e]) is none of `pairs`."""
    row, col = np.asarray(row).view(np.uint32), np.asarray(col).view(np.uint32)
    if not pairs:
        return np.ones(row.size, bool)
    keys = np.array(sorted((c << 32) | r for c, r in pairs), np.uint64)
    edge = (col.astype(np.uint64) << np.uint64(32)) | row.astype(np.uint64)
    return ~np.isin(edge, keys)


def drop_pair_edges(pair_src, pair_dst, which, layers):
    """layers: [(row, col)] holding exactly the layer's edges -> ([(row, col)] of the kept edges, dropped per layer)."""
    pairs = pair_set(pair_src, pair_dst, which)
    out, dropped = [], []
    for row, col in layers:
        keep = keep_mask(row, col, pairs)
        out.append((np.asarray(row).view(np.uint32)[keep], np.asarray(col).view(np.uint32)[keep]))
        dropped.append(int((~keep).sum()))
    return out, dropped
