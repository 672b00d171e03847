"""ppr_topk (include/ggms.h, ggms_sample_ppr) restated in plain numpy / Python integers, and the exact PPR vector by a
dense float64 solve.  Shares no code with the kernel; the GPU result must equal `sample_layer` bit for bit."""
import math

import numpy as np

EMPTY = 0xFFFFFFFF
ONE = 1 << 30


def constants(alpha, eps):
    return math.floor(alpha * 65536 + 0.5), math.floor(eps * ONE)


def push(ip, ix, s, alpha, eps, C, max_rounds):
    """The map node -> [r, p] of seed s after the rounds; (map, rounds performed, truncated)."""
    A, E = constants(alpha, eps)
    deg = lambda u: int(ip[u + 1]) - int(ip[u])
    state, rounds = {s: [ONE, 0]}, 0
    for _ in range(max_rounds):
        act = [u for u, (r, _) in state.items() if (r >= E * deg(u) if deg(u) else r > 0)]
        if not act:
            break
        new = {int(v) for u in act for v in ix[ip[u]:ip[u + 1]].tolist()} - state.keys()
        if len(state) + len(new) > C:
            return state, rounds, True
        adds = []
        for u in act:  # with the values the round began with: all reads before all adds
            r, d = state[u][0], deg(u)
            if d == 0:
                state[u][1] += r
                state[u][0] = 0
                continue
            a = (A * r) >> 16
            q = (r - a) // d
            state[u][1] += a
            state[u][0] -= a + q * d
            adds.append((u, q))
        for u, q in adds:
            for v in ix[ip[u]:ip[u + 1]].tolist():
                state.setdefault(v, [0, 0])[0] += q
        rounds += 1
    return state, rounds, False


def sample_layer(ip, ix, inp, alpha, eps, C, max_rounds, K):
    """One layer: (where = the seed's position in inp, src, dst, data, stat (n, 2)), seeds in input order, the scored
    nodes but the seed by p descending, ties by the smaller id, cut at K."""
    where, src, dst, data, memo = [], [], [], [], {}
    stat = np.zeros((len(inp), 2), np.uint32)
    for i, s in enumerate(np.asarray(inp, dtype=np.uint32).tolist()):
        if s == EMPTY:
            continue
        if s not in memo:
            state, rounds, trunc = push(ip, ix, s, alpha, eps, C, max_rounds)
            top = sorted((u for u, (_, p) in state.items() if u != s and p > 0), key=lambda u: (-state[u][1], u))[:K]
            assert sum(r + p for r, p in state.values()) == ONE
            memo[s] = [(u, state[u][1]) for u in top], (rounds | (trunc << 31), sum(p for _, p in state.values()))
        top, stat[i] = memo[s]
        for u, p in top:
            where.append(i), src.append(s), dst.append(u), data.append(p)
    return np.array(where, np.int64), np.array(src, np.uint32), np.array(dst, np.uint32), np.array(data, np.uint32), stat


def sample_batch(ip, ix, seeds, num_layer, alpha, eps, C, max_rounds, K):
    """ggms_sample_batch_ppr: first-occurrence numbering (the seeds, then every layer's new nodes in edge order); layer
    L-1 pushes from the raw seeds, every later one from all nodes seen so far.
    dict(layers=[{row, col, data, num_src, num_dst}] by layer id, input_nodes)."""
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
        where, _, dst, data, _ = sample_layer(ip, ix, frontier, alpha, eps, C, max_rounds, K)
        layers[i] = dict(row=enter(dst), col=col_of[where].astype(np.uint32), data=data, num_src=len(n2o),
                         num_dst=len(frontier))
        frontier = np.array(n2o, dtype=np.uint32)
        col_of = np.arange(len(n2o), dtype=np.uint32)
    return dict(layers=layers, input_nodes=np.array(n2o, dtype=np.uint32))


def exact_ppr(ip, ix, s, alpha):
    """pi = alpha e_s + (1 - alpha) pi P in float64, alpha = A / 65536, with dangling nodes absorbing (their walk stops:
    all the mass that reaches one stays there)."""
    n = len(ip) - 1
    a = constants(alpha, 1.0)[0] / 65536
    deg = np.diff(ip.astype(np.int64))
    P = np.zeros((n, n))
    np.add.at(P, (np.repeat(np.arange(n), deg), ix.astype(np.int64)), 1.0)
    P[deg > 0] /= deg[deg > 0, None]
    stop = np.where(deg > 0, a, 1.0)  # the share of the mass arriving at u that settles there
    e = np.zeros(n)
    e[s] = 1.0
    # the mass arriving at every node: x = e_s + x diag(1 - stop) P
    x = np.linalg.solve((np.eye(n) - (1.0 - stop)[:, None] * P).T, e)
    return x * stop
