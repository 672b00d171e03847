"""numpy statement of khop_labor (include/ggms.h, GGMS_KHOP_LABOR): the hash, the salt rules, one layer, and the batch
chain with first-occurrence numbering as ggms_sample_batch documents it.  Plus the community graph the sampler's claim
(fewer input nodes than independent sampling) is tested on."""
import numpy as np

M32 = 0xFFFFFFFF
GOLDEN = 0x9E3779B9


def fmix32(x):
    """MurmurHash3's 32-bit finaliser, element-wise, mod 2^32."""
    x = np.asarray(x, dtype=np.uint64) & M32
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x85EBCA6B)) & M32
    x ^= x >> np.uint64(13)
    x = (x * np.uint64(0xC2B2AE35)) & M32
    x ^= x >> np.uint64(16)
    return x


def layer_salt(batch_salt, layer):
    return int(fmix32((int(batch_salt) + GOLDEN * (layer + 1)) & M32))


def batch_salt(seed, epoch, batch_index):
    return int(fmix32(int(fmix32(((int(seed) & M32) + int(epoch)) & M32)) ^ (int(batch_index) & M32)))


def select_positions(ids, fanout, salt):
    """The min(fanout, d) positions of the list with the smallest keys (fmix32(id ^ salt) << 32) | position, ascending."""
    d = len(ids)
    if d <= fanout:
        return np.arange(d)
    keys = (fmix32(np.asarray(ids, dtype=np.uint64) ^ np.uint64(salt)) << np.uint64(32)) | np.arange(d, dtype=np.uint64)
    return np.sort(np.argpartition(keys, fanout - 1)[:fanout])


def sample_layer(ip, ix, seeds, fanout, salt):
    """(seed position, out_src, out_dst) of every sampled edge: seeds in input order, positions ascending in a seed."""
    where, src, dst = [], [], []
    for j, s in enumerate(np.asarray(seeds, dtype=np.int64)):
        ids = ix[int(ip[s]):int(ip[s + 1])]
        pos = select_positions(ids, fanout, salt)
        where.append(np.full(pos.size, j, np.int64))
        src.append(np.full(pos.size, s, np.uint32))
        dst.append(ids[pos].astype(np.uint32))
    if not where:
        return np.zeros(0, np.int64), np.zeros(0, np.uint32), np.zeros(0, np.uint32)
    return np.concatenate(where), np.concatenate(src), np.concatenate(dst)


def sample_batch(ip, ix, seeds, fanouts, salt):
    """ggms_sample_batch(GGMS_KHOP_LABOR): dict(layers=[{row, col, num_src, num_dst}] by layer id, input_nodes).
    Local ids are first-occurrence positions: the seeds, then every layer's new neighbours in edge order; layer
    L-1 samples from the raw seeds (col = the seed's local id), every later one from all nodes seen so far."""
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
    L = len(fanouts)
    layers = [None] * L
    frontier, col_of = seeds, seed_local
    for i in range(L - 1, -1, -1):
        where, _, dst = sample_layer(ip, ix, frontier, fanouts[i], layer_salt(salt, i))
        col = col_of[where].astype(np.uint32) if where.size else np.zeros(0, np.uint32)
        row = enter(dst)
        layers[i] = dict(row=row, col=col, num_src=len(n2o), num_dst=len(frontier))
        frontier = np.array(n2o, dtype=np.uint32)
        col_of = np.arange(len(n2o), dtype=np.uint32)
    return dict(layers=layers, input_nodes=np.array(n2o, dtype=np.uint32))


def community_graph(num_node=20_000, community=500, mean_degree=50, inside=0.9, skew=0.6, max_degree=2000, seed=0):
    """CSR of a clustered graph: degree = clip(int(lognormal(ln mean - 0.5, 1)), 1, max); a neighbour lies inside the
    owner's community with probability `inside`, drawn there with popularity ~ rank^-skew, else uniform over all nodes."""
    rng = np.random.RandomState(seed)
    deg = np.clip(rng.lognormal(np.log(mean_degree) - 0.5, 1.0, num_node).astype(np.int64), 1, max_degree)
    ip = np.zeros(num_node + 1, np.uint32)
    ip[1:] = np.cumsum(deg)
    E = int(ip[-1])
    owner = np.repeat(np.arange(num_node, dtype=np.int64), deg)
    cdf = np.cumsum(np.arange(1, community + 1, dtype=np.float64) ** -skew)
    rank = np.searchsorted(cdf / cdf[-1], rng.random_sample(E))
    local = np.minimum((owner // community) * community + rank, num_node - 1)
    ix = np.where(rng.random_sample(E) < inside, local, rng.randint(0, num_node, E)).astype(np.uint32)
    return ip, ix
