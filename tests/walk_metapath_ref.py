"""random_walk_metapath (include/ggms.h, ggms_sample_walk_metapath) restated in plain numpy / Python integers.  Shares no
code with the kernel; the GPU result must equal this bit for bit."""
import math

import numpy as np

from khop_labor_ref import layer_salt

EMPTY = 0xFFFFFFFF
M32 = 0xFFFFFFFF


def fmix32(x):
    x &= M32
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & M32
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & M32
    return x ^ (x >> 16)


def seed_visits(ip, ix, et, metapath, s, T, p, W, salt):
    """The visits of seed node s by visit number t * W + w; None where the walk had ended."""
    M = len(metapath)
    thr = min(1 << 32, math.floor(p * 4294967296.0))
    visits = [None] * (T * W)
    base = fmix32(s ^ salt)
    for w in range(W):
        wk = fmix32(base + 0x9E3779B9 * (w + 1))
        u = s
        for t in range(T):
            for j, r in enumerate(metapath):
                types = et[ip[u]:ip[u + 1]]
                b = int(np.searchsorted(types, r, "left"))
                e = int(np.searchsorted(types, r, "right")) - b
                if e == 0:  # no edge of relation r: the walk ends
                    break
                u = int(ix[int(ip[u]) + b + ((fmix32(wk + 0x85EBCA6B * (2 * (t * M + j) + 1)) * e) >> 32)])
            else:  # a full traversal: a visit, then the restart test
                visits[t * W + w] = u
                if fmix32(wk + 0x85EBCA6B * (2 * t + 2)) >= thr:
                    continue
            break  # the walk ended
    return visits


def sample_layer(ip, ix, et, metapath, inp, T, p, W, K, salt):
    """One layer: (where = the seed's position in inp, src, dst, data) of every output edge, seeds in input order, the
    distinct visited nodes by count descending, ties by the smaller first visit number, cut at K."""
    where, src, dst, data, memo = [], [], [], [], {}
    for i, s in enumerate(np.asarray(inp, dtype=np.uint32).tolist()):
        if s == EMPTY:
            continue
        if s not in memo:  # the walks are keyed by node id
            count, first = {}, {}
            for e, v in enumerate(seed_visits(ip, ix, et, metapath, s, T, p, W, salt)):
                if v is not None:
                    count[v] = count.get(v, 0) + 1
                    first.setdefault(v, e)
            memo[s] = sorted(count, key=lambda v: (-count[v], first[v]))[:K], count
        top, count = memo[s]
        for v in top:
            where.append(i), src.append(s), dst.append(v), data.append(count[v])
    return np.array(where, np.int64), np.array(src, np.uint32), np.array(dst, np.uint32), np.array(data, np.uint32)


def sample_batch(ip, ix, et, metapath, seeds, num_layer, T, p, W, K, salt):
    """ggms_sample_batch_walk_metapath: first-occurrence numbering (the seeds, then every layer's new nodes in edge
    order); layer L-1 walks from the raw seeds, every later one from all nodes seen so far, layer i under
    layer_salt(salt, i).  dict(layers=[{row, col, data, num_src, num_dst}] by layer id, input_nodes)."""
    local, n2o = {}, []

    def enter(ids):
        for v in ids.tolist():
            if v not in local:
                local[v] = len(n2o)
                n2o.append(v)
        return np.array([local[v] for v in ids.tolist()], np.uint32)

    frontier = np.asarray(seeds, dtype=np.uint32)
    col_of, layers = enter(frontier), [None] * num_layer
    for i in range(num_layer - 1, -1, -1):
        where, _, dst, data = sample_layer(ip, ix, et, metapath, frontier, T, p, W, K, layer_salt(salt, i))
        layers[i] = dict(row=enter(dst), col=col_of[where].astype(np.uint32), data=data, num_src=len(n2o),
                         num_dst=len(frontier))
        frontier = np.array(n2o, dtype=np.uint32)
        col_of = np.arange(len(n2o), dtype=np.uint32)
    return dict(layers=layers, input_nodes=np.array(n2o, dtype=np.uint32))
