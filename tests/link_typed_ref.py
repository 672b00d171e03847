"""numpy statement of ggms_link_seeds_typed (include/ggms.h), on tests/link_ref.py: the negatives of positive (u, r, v)
are nodes of v's type, drawn through the type lists by link_ref's hash; only u's segment of relation r rejects."""
import numpy as np

import link_ref as ref

TYPED_UNIFORM, TYPED_EXCLUDE = 2, 3


def type_lists(node_type, T):
    """(type_nodes: the node ids grouped by type, ascending inside a type; type_base[T + 1]: the groups' starts)"""
    node_type = np.asarray(node_type)
    base = np.concatenate([[0], np.cumsum(np.bincount(node_type, minlength=T))]).astype(np.uint32)
    return np.argsort(node_type, kind="stable").astype(np.uint32), base


def negatives(ip, ix, et, nt, T, e, K, mode, salt, lists=None):
    """(the K negatives of edge e, how many of them were forced, r); lists: type_lists(nt, T), to build them once"""
    nodes, base = lists or type_lists(nt, T)
    u, v = ref.edge_endpoints(ip, ix, e)
    r, t = int(et[e]), int(nt[v])
    n_t = int(base[t + 1]) - int(base[t])
    c = nodes[int(base[t]) + ref.cand(e, np.arange(K)[:, None], np.arange(ref.ATTEMPTS)[None, :], salt, n_t)]  # (K, 8)
    if mode == TYPED_UNIFORM:
        return c[:, 0].copy(), 0, r
    lo, hi = int(ip[u]), int(ip[u + 1])
    banned = set(ix[lo:hi][np.asarray(et[lo:hi]) == r].tolist()) | {u}
    ok = ~np.isin(c, list(banned))
    first = np.where(ok.any(1), ok.argmax(1), ref.ATTEMPTS - 1)
    return c[np.arange(K), first], int((~ok.any(1)).sum()), r


def link_seeds_typed(ip, ix, et, nt, T, edge_ids, K, mode, salt):
    """(endpoints in link_ref.link_seeds' layout, rel uint8[B], forced count); an edge id >= E: EMPTY and 0xff"""
    edge_ids = np.asarray(edge_ids, dtype=np.int64)
    B, E = edge_ids.size, int(ip[-1])
    out, rel, forced = np.full(B * (2 + K), ref.EMPTY, np.uint32), np.full(B, 0xFF, np.uint8), 0
    lists = type_lists(nt, T)
    for i, e in enumerate(edge_ids.tolist()):
        if e >= E:
            continue
        out[i], out[B + i] = ref.edge_endpoints(ip, ix, e)
        out[2 * B + i * K: 2 * B + (i + 1) * K], f, rel[i] = negatives(ip, ix, et, nt, T, e, K, mode, salt, lists)
        forced += f
    return out, rel, forced


SEG = [1, 63, 64, 65, 512, 513, 2049, 2050]  # segment lengths around the wave, the 512-id group and the 2048-id wide group
T_ALL, N_BASE = 6, 900


def edge_case_graph():
    """The leaf tests' graph, (ip, ix, et, nt, T = 6, cases: name -> edge id).
    Nodes [0, 900): T = 3 types, lists of 0 .. 40 entries, relations 0 .. 8 from datagen.relation_types.  Behind them:
    S, the ONE node of type 3; 32 nodes of type 4; G0 .. G3 of type 5; then owners (type 0) whose lists are built by hand,
    relation 9 + the entry's type (15: a second relation into type 5):
      rows k = 0 .. 7   three segments of SEG[k], SEG[k + 1], SEG[k + 2] entries (types 0, 1, 2): every length at the head, in
                        the middle and at the tail of a list; then lists of 3, 64 and 65 entries in all
      hub               40 000 entries: segments of 3, 30 000 and 9 997
      single, all       S alone under relation 12; all 32 nodes of type 4 under relation 13: every candidate is in the segment
      other             G0 under relation 14, G1 .. G3 under relation 15 only: they do not reject
    and G3 itself owns (14: G1): the source is of the destination's type and is drawn."""
    from xgnn_amd import datagen
    rng = np.random.RandomState(4)
    deg = rng.randint(0, 41, N_BASE)
    ip0 = np.concatenate([[0], np.cumsum(deg)])
    ix0 = rng.randint(0, N_BASE, int(ip0[-1]))
    nt = rng.choice(3, N_BASE, p=[0.5, 0.3, 0.2]).astype(np.uint8)
    of = [np.flatnonzero(nt == t) for t in range(3)]
    S, F, G = N_BASE, np.arange(N_BASE + 1, N_BASE + 33), np.arange(N_BASE + 33, N_BASE + 37)
    seg3 = lambda a, b, c: ([rng.choice(of[0], a), rng.choice(of[1], b), rng.choice(of[2], c)], [9] * a + [10] * b + [11] * c)  # noqa: E731
    rows = [seg3(SEG[k], SEG[(k + 1) % 8], SEG[(k + 2) % 8]) for k in range(8)]
    rows += [seg3(1, 1, 1), seg3(20, 1, 43), seg3(1, 63, 1), seg3(3, 30000, 9997), ([[S]], [12]), ([F], [13] * 32),
             ([G[:1], G[1:]], [14, 15, 15, 15])]
    names = [f"row{k}" for k in range(8)] + ["three", "sixty4", "sixty5", "hub", "single", "all", "other"]
    lists = [ix0[ip0[v]:ip0[v + 1]] for v in range(N_BASE)] + [[] for _ in range(36)] + [[G[1]]]  # ..., S, F, G0 .. G2, G3
    types = [datagen.relation_types(ip0, ix0, nt, 3)[ip0[v]:ip0[v + 1]] for v in range(N_BASE)] + [[] for _ in range(36)] + [[14]]
    for ids, ty in rows:
        lists.append(np.concatenate(ids))
        types.append(ty)
    nt = np.concatenate([nt, [3], [4] * 32, [5] * 4, [0] * len(rows)]).astype(np.uint8)
    ip, ix = ref.graph_of_lists(lists)
    ix, et, _ = datagen.sort_lists_by_type(ip, ix, np.concatenate(types).astype(np.uint8))
    first = N_BASE + 37
    cases = {"g3": int(ip[first - 1])}
    for k, name in enumerate(names):  # the first and last position of every segment of the row
        b, e = int(ip[first + k]), int(ip[first + k + 1])
        cut = [b] + (np.flatnonzero(np.diff(et[b:e])) + b + 1).tolist() + [e]
        for s, (x, y) in enumerate(zip(cut[:-1], cut[1:])):
            cases[f"{name}.{s}a"], cases[f"{name}.{s}z"] = x, y - 1
    return ip, ix, et, nt, T_ALL, cases
