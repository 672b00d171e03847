"""numpy statement of khop_labor_weighted (include/ggms.h, GGMS_KHOP_LABOR_WEIGHTED): the fixed-point exponential
variate of a node, the key of an edge, one layer, and the batch chain with khop_labor's dedup and numbering."""
import numpy as np

import khop_labor_ref as labor

U = np.uint64
W_MIN, W_MAX = np.float32(2.0 ** -40), np.float32(2.0 ** 40)

# T[i] = round(2^32 log2(1 + i / 256)): the same 257 constants as xgnn_amd/csrc/labor_log2_table.h
LOG2_TABLE = np.array([
    0x00000000, 0x01709c47, 0x02dfca17, 0x044d8c46, 0x05b9e5a1, 0x0724d8ef,
    0x088e68eb, 0x09f6984a, 0x0b5d69bb, 0x0cc2dfe2, 0x0e26fd5d, 0x0f89c4c2,
    0x10eb38a0, 0x124b5b7e, 0x13aa2fdd, 0x1507b836, 0x1663f6fb, 0x17beee97,
    0x1918a16e, 0x1a7111df, 0x1bc84241, 0x1d1e34e3, 0x1e72ec11, 0x1fc66a0f,
    0x2118b11a, 0x2269c369, 0x23b9a32f, 0x25085296, 0x2655d3c5, 0x27a228db,
    0x28ed53f3, 0x2a375721, 0x2b803474, 0x2cc7edf6, 0x2e0e85aa, 0x2f53fd90,
    0x309857a0, 0x31db95d0, 0x331dba0f, 0x345ec646, 0x359ebc5b, 0x36dd9e2f,
    0x381b6d9c, 0x39582c79, 0x3a93dc98, 0x3bce7fc7, 0x3d0817cf, 0x3e40a672,
    0x3f782d72, 0x40aeae89, 0x41e42b6f, 0x4318a5d5, 0x444c1f6b, 0x457e99db,
    0x46b016ca, 0x47e097db, 0x49101eac, 0x4a3eacd7, 0x4b6c43f1, 0x4c98e58e,
    0x4dc4933b, 0x4eef4e83, 0x501918ec, 0x5141f3fb, 0x5269e12f, 0x5390e204,
    0x54b6f7f1, 0x55dc246d, 0x570068e8, 0x5823c6d1, 0x59463f92, 0x5a67d492,
    0x5b888736, 0x5ca858df, 0x5dc74aea, 0x5ee55eb1, 0x6002958c, 0x611ef0cf,
    0x623a71cc, 0x635519cf, 0x646eea24, 0x6587e415, 0x66a008e4, 0x67b759d6,
    0x68cdd82a, 0x69e3851c, 0x6af861e6, 0x6c0c6fc0, 0x6d1fafdd, 0x6e322370,
    0x6f43cba8, 0x7054a9b1, 0x7164beb5, 0x72740bdb, 0x73829249, 0x74905320,
    0x759d4f81, 0x76a98888, 0x77b4ff51, 0x78bfb4f4, 0x79c9aa88, 0x7ad2e11f,
    0x7bdb59cd, 0x7ce3159f, 0x7dea15a3, 0x7ef05ae4, 0x7ff5e66a, 0x80fab93c,
    0x81fed45d, 0x830238d0, 0x8404e794, 0x8506e1a8, 0x86082807, 0x8708bbaa,
    0x88089d8b, 0x8907ce9d, 0x8a064fd5, 0x8b042225, 0x8c01467c, 0x8cfdbdc8,
    0x8df988f5, 0x8ef4a8ed, 0x8fef1e98, 0x90e8eade, 0x91e20ea1, 0x92da8ac6,
    0x93d2602c, 0x94c98fb4, 0x95c01a3a, 0x96b6009b, 0x97ab43af, 0x989fe451,
    0x9993e356, 0x9a874193, 0x9b79ffdb, 0x9c6c1f01, 0x9d5d9fd5, 0x9e4e8325,
    0x9f3ec9bd, 0xa02e746a, 0xa11d83f5, 0xa20bf926, 0xa2f9d4c5, 0xa3e71797,
    0xa4d3c25e, 0xa5bfd5df, 0xa6ab52da, 0xa7963a0d, 0xa8808c38, 0xa96a4a17,
    0xaa537465, 0xab3c0bdc, 0xac241135, 0xad0b8526, 0xadf26866, 0xaed8bba8,
    0xafbe7fa1, 0xb0a3b502, 0xb1885c7b, 0xb26c76bc, 0xb3500472, 0xb433064b,
    0xb5157cf3, 0xb5f76913, 0xb6d8cb54, 0xb7b9a45e, 0xb899f4d9, 0xb979bd69,
    0xba58feb2, 0xbb37b959, 0xbc15edff, 0xbcf39d45, 0xbdd0c7ca, 0xbead6e2d,
    0xbf89910c, 0xc0653103, 0xc1404eae, 0xc21aeaa6, 0xc2f50586, 0xc3ce9fe4,
    0xc4a7ba58, 0xc5805579, 0xc65871da, 0xc7301011, 0xc80730b0, 0xc8ddd449,
    0xc9b3fb6d, 0xca89a6ac, 0xcb5ed695, 0xcc338bb7, 0xcd07c69e, 0xcddb87d6,
    0xceaecfeb, 0xcf819f66, 0xd053f6d2, 0xd125d6b7, 0xd1f73f9c, 0xd2c83209,
    0xd398ae81, 0xd468b58c, 0xd53847ac, 0xd6076565, 0xd6d60f39, 0xd7a445a9,
    0xd8720936, 0xd93f5a60, 0xda0c39a5, 0xdad8a784, 0xdba4a47b, 0xdc703104,
    0xdd3b4d9d, 0xde05fac0, 0xded038e6, 0xdf9a088a, 0xe0636a24, 0xe12c5e2b,
    0xe1f4e517, 0xe2bcff5e, 0xe384ad75, 0xe44befd0, 0xe512c6e5, 0xe5d93326,
    0xe69f3506, 0xe764ccf7, 0xe829fb69, 0xe8eec0ce, 0xe9b31d94, 0xea77122b,
    0xeb3a9f02, 0xebfdc485, 0xecc08322, 0xed82db45, 0xee44cd5a, 0xef0659cc,
    0xefc78104, 0xf088436d, 0xf148a170, 0xf2089b75, 0xf2c831e4, 0xf3876524,
    0xf446359b, 0xf504a3af, 0xf5c2afc6, 0xf6805a44, 0xf73da38e, 0xf7fa8c05,
    0xf8b7140f, 0xf9733c0c, 0xfa2f045e, 0xfaea6d67, 0xfba57787, 0xfc60231e,
    0xfd1a708c, 0xfdd4602e, 0xfe8df264, 0xff47278b, 0x100000000,
], dtype=np.uint64)


def variate(h):
    """E of a 32-bit hash: (33 << 32) - the fixed-point log2 of v = 2 h + 1; E / 2^32 * ln 2 ~ Exp(1)."""
    v = U(2) * np.asarray(h, dtype=U) + U(1)
    e = np.zeros(v.shape, U)
    for s in (32, 16, 8, 4, 2, 1):  # e = floor(log2 v), v < 2^33
        big = (v >> (e + U(s))) != 0
        e = np.where(big, e + U(s), e)
    f = ((v << (U(63) - e)) >> U(31)) & U(0xFFFFFFFF)
    i, r = f >> U(24), f & U(0xFFFFFF)
    t0, t1 = LOG2_TABLE[i], LOG2_TABLE[i + U(1)]
    return (U(33) << U(32)) - ((e << U(32)) + t0 + (((t1 - t0) * r) >> U(24)))


def key32(ids, weights, salt):
    """bits(float32(E) / clamp(w)) per list position: positive normal floats, which order like their bit patterns."""
    E = variate(labor.fmix32(np.asarray(ids, dtype=U) ^ U(salt)))
    w = np.fmin(np.fmax(np.asarray(weights, dtype=np.float32), W_MIN), W_MAX)
    return (E.astype(np.float32) / w).astype(np.float32).view(np.uint32)


def select_positions(ids, weights, fanout, salt):
    """The min(fanout, d) positions with the smallest (key32, position), ascending."""
    d = len(ids)
    if d <= fanout:
        return np.arange(d)
    order = np.lexsort((np.arange(d), key32(ids, weights, salt)))
    return np.sort(order[:fanout])


def sample_layer(ip, ix, ew, seeds, fanout, salt):
    """(seed position, out_src, out_dst, out_pos) of every sampled edge: seeds in input order, positions ascending."""
    where, src, dst, pos = [np.zeros(0, np.int64)], [np.zeros(0, np.uint32)], [np.zeros(0, np.uint32)], [np.zeros(0, np.uint32)]
    for j, s in enumerate(np.asarray(seeds, dtype=np.int64)):
        b, e = int(ip[s]), int(ip[s + 1])
        p = select_positions(ix[b:e], ew[b:e], fanout, salt)
        where.append(np.full(p.size, j, np.int64))
        src.append(np.full(p.size, s, np.uint32))
        dst.append(ix[b:e][p].astype(np.uint32))
        pos.append((b + p).astype(np.uint32))
    return tuple(np.concatenate(x) for x in (where, src, dst, pos))


def sample_batch(ip, ix, ew, seeds, fanouts, salt):
    """ggms_sample_batch_labor_weighted: khop_labor_ref.sample_batch's chain -- first-occurrence numbering, layer L-1
    from the raw seeds, every later one from all nodes seen so far, khop_labor's layer salts -- with this sampler;
    every layer also carries `eid`, the CSR positions."""
    seeds = np.asarray(seeds, dtype=np.uint32)
    local, n2o = {}, []

    def enter(ids):
        for v in ids.tolist():
            if v not in local:
                local[v] = len(n2o)
                n2o.append(v)
        return np.array([local[v] for v in ids.tolist()], np.uint32)

    col_of, frontier = enter(seeds), seeds
    layers = [None] * len(fanouts)
    for i in range(len(fanouts) - 1, -1, -1):
        where, _, dst, pos = sample_layer(ip, ix, ew, frontier, fanouts[i], labor.layer_salt(salt, i))
        layers[i] = dict(row=enter(dst), col=col_of[where].astype(np.uint32), eid=pos, num_src=len(n2o),
                         num_dst=len(frontier))
        frontier = np.array(n2o, dtype=np.uint32)
        col_of = np.arange(len(n2o), dtype=np.uint32)
    return dict(layers=layers, input_nodes=np.array(n2o, dtype=np.uint32))
