"""numpy statement of ggms_link_seeds (include/ggms.h): edge ids -> endpoints, the candidate hash, both negative modes,
the forced rule, the endpoint layout and the engine's salt rule.  Plus the first-occurrence ranks a batch numbers its
raw seeds by (ggms_sample_batch_seed_ids)."""
import numpy as np

from khop_labor_ref import GOLDEN, M32, batch_salt, fmix32

EMPTY = 0xFFFFFFFF
ATTEMPTS = 8
UNIFORM, EXCLUDE = 0, 1
LINK_TAG = 0x6C696E6B


def engine_salt(seed, epoch, batch_index):
    """The salt of the engine's batch (epoch, global batch index) of a run with config key `seed`."""
    return int(fmix32(batch_salt(seed, epoch, batch_index) ^ LINK_TAG))


def edge_endpoints(ip, ix, e):
    """(u, v) of CSR position e < E: u is the one row with ip[u] <= e < ip[u + 1] (upper bound over ip), v = ix[e]."""
    u = int(np.searchsorted(np.asarray(ip, dtype=np.int64), int(e), side="right")) - 1
    assert ip[u] <= e < ip[u + 1]
    return u, int(ix[e])


def cand(e, j, a, salt, num_node):
    """cand(e, j, a) = mulhi32(fmix32(fmix32(e ^ salt) + 0x9e3779b9 * (8 j + a + 1)), num_node); j, a may be arrays."""
    h0 = int(fmix32((int(e) ^ int(salt)) & M32))
    step = (np.asarray(j, dtype=np.uint64) * np.uint64(ATTEMPTS) + np.asarray(a, dtype=np.uint64) + np.uint64(1))
    h = fmix32((np.uint64(h0) + np.uint64(GOLDEN) * step) & np.uint64(M32))
    return ((h * np.uint64(num_node)) >> np.uint64(32)).astype(np.uint32)


def negatives(ip, ix, e, K, mode, salt):
    """(the K negatives of edge e, how many of them were forced)."""
    num_node = len(ip) - 1
    u, _ = edge_endpoints(ip, ix, e)
    c = cand(e, np.arange(K)[:, None], np.arange(ATTEMPTS)[None, :], salt, num_node)  # (K, 8)
    if mode == UNIFORM:
        return c[:, 0].copy(), 0
    banned = set(ix[int(ip[u]):int(ip[u + 1])].tolist()) | {u}
    out, forced = np.empty(K, np.uint32), 0
    for j in range(K):
        ok = [a for a in range(ATTEMPTS) if int(c[j, a]) not in banned]
        out[j] = c[j, ok[0]] if ok else c[j, ATTEMPTS - 1]
        forced += not ok
    return out, forced


def link_seeds(ip, ix, edge_ids, K, mode, salt):
    """(endpoints uint32[B (2 + K)], forced count): [0, B) sources, [B, 2 B) destinations, [2 B + i K + j] negative j of
    positive i; an edge id >= E leaves GGMS_EMPTY_KEY in its 2 + K positions."""
    edge_ids = np.asarray(edge_ids, dtype=np.int64)
    B, E = edge_ids.size, int(ip[-1])
    out = np.full(B * (2 + K), EMPTY, np.uint32)
    forced = 0
    for i, e in enumerate(edge_ids.tolist()):
        if e >= E:
            continue
        out[i], out[B + i] = edge_endpoints(ip, ix, e)
        out[2 * B + i * K: 2 * B + (i + 1) * K], f = negatives(ip, ix, e, K, mode, salt)
        forced += f
    return out, forced


def split(endpoints, K):
    """(src[B], dst[B], neg[B, K]) views of an endpoint list."""
    B = endpoints.size // (2 + K)
    return endpoints[:B], endpoints[B:2 * B], endpoints[2 * B:].reshape(B, K)


def first_occurrence_ranks(seeds):
    """(local id of every raw seed, the distinct seeds in first-occurrence order): how a batch numbers its seeds."""
    seeds = np.asarray(seeds)
    uniq, first, inv = np.unique(seeds, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")  # unique values by first occurrence
    rank = np.empty(order.size, np.uint32)
    rank[order] = np.arange(order.size, dtype=np.uint32)
    return rank[inv.ravel()], uniq[order].astype(np.uint32)


def graph_of_lists(lists):
    ip = np.zeros(len(lists) + 1, np.uint32)
    ip[1:] = np.cumsum([len(x) for x in lists])
    ix = np.concatenate([np.asarray(x, np.uint32) for x in lists]) if ip[-1] else np.zeros(0, np.uint32)
    return ip, ix


def complete_graph(n):
    """every node adjacent to every OTHER node: with the source itself rejected, no candidate is ever accepted"""
    return graph_of_lists([[w for w in range(n) if w != v] for v in range(n)])
