"""khop_typed without a GPU: the numpy statement (tests/khop_typed_ref.py) against a brute-force loop, the restriction
property (the edges of one type are khop_labor's on the CSR filtered to that type), R = 1 against khop_labor_ref, the
marginals, datagen's type-sorted CSR, and the argument refusals of the C entry points (all before any device call)."""
import ctypes as C

import numpy as np
import pytest

import khop_labor_ref as labor
import khop_typed_ref as ref

INVALID = -1  # GGMS_ERR_INVALID


def multigraph(num_node=200, seed=0, max_deg=60, R=5, num_id=None):
    """Lists of random length with many parallel edges (ids from a small range), types sorted inside every list; the
    last type is rare and type 1 is held by no list."""
    rng = np.random.RandomState(seed)
    deg = rng.randint(0, max_deg, num_node)
    deg[rng.randint(0, num_node, 5)] = 0
    ip = np.zeros(num_node + 1, np.uint32)
    ip[1:] = np.cumsum(deg)
    ix = rng.randint(0, num_id or num_node, int(ip[-1])).astype(np.uint32)
    w = np.ones(R)
    if R > 2:
        w[1], w[-1] = 0.0, 0.05
    return ip, ix, ref.sorted_types(ip, rng, R, w / w.sum())


def brute_edges(ids, types, type_fanout, salt):
    """The definition, entry by entry: per type the k_r smallest (hash, position) pairs; ascending position."""
    out = []
    for r, k in enumerate(type_fanout):
        seg = [p for p in range(len(ids)) if int(types[p]) == r]
        keyed = sorted((int(labor.fmix32(int(ids[p]) ^ salt)), p) for p in seg)
        out += [(p, r) for _, p in keyed[:k]]
    return sorted(out)


def test_reference_equals_the_brute_force_loop():
    ip, ix, et = multigraph()
    seeds = np.random.RandomState(1).randint(0, 200, 300).astype(np.uint32)
    for tf, salt in (([1, 1, 1, 1, 1], 7), ([5, 3, 0, 2, 4], 0x4329F67E), ([127, 0, 127, 1, 127], 3)):
        where, src, dst, pos, typ = ref.sample_layer(ip, ix, et, seeds, tf, salt)
        n = 0
        for j, s in enumerate(seeds.tolist()):
            b, e = int(ip[s]), int(ip[s + 1])
            want = brute_edges(ix[b:e], et[b:e], tf, salt)
            sel = where == j
            assert pos[sel].tolist() == [b + p for p, _ in want], (j, s)
            assert typ[sel].tolist() == [r for _, r in want]
            assert (et[pos[sel]] == typ[sel]).all() and (ix[pos[sel]] == dst[sel]).all() and (src[sel] == s).all()
            n += len(want)
        assert n == pos.size


def test_restriction_property():
    """For every r the typed sample's edges of type r equal khop_labor on the CSR filtered to type r, fanout k_r, the
    same salt."""
    ip, ix, et = multigraph(seed=3)
    seeds = np.random.RandomState(4).randint(0, 200, 250).astype(np.uint32)
    tf, salt = [4, 2, 0, 7, 1], 0x1234567
    where, _, dst, pos, typ = ref.sample_layer(ip, ix, et, seeds, tf, salt)
    for r, k in enumerate(tf):
        fip, fix, orig = ref.filtered_csr(ip, ix, et, r)
        if k == 0:
            assert not (typ == r).any()
            continue
        fwhere, _, fdst = labor.sample_layer(fip, fix, seeds, k, salt)
        # the filtered CSR's selected positions, as positions of the original
        fpos = []
        for s in seeds.astype(np.int64):
            ids = fix[int(fip[s]):int(fip[s + 1])]
            fpos.append(orig[int(fip[s]) + labor.select_positions(ids, k, salt)])
        fpos = np.concatenate(fpos) if fpos else np.zeros(0, np.uint32)
        assert np.array_equal(where[typ == r], fwhere)
        assert np.array_equal(dst[typ == r], fdst)
        assert np.array_equal(pos[typ == r], fpos)


def test_one_type_is_khop_labor_leaf_and_batch():
    ip, ix, _ = multigraph(seed=5)
    et = np.zeros(ix.size, np.uint8)
    seeds = np.random.RandomState(6).randint(0, 200, 120).astype(np.uint32)
    for k, salt in ((1, 1), (10, 99), (127, 5)):
        where, src, dst, pos, typ = ref.sample_layer(ip, ix, et, seeds, [k], salt)
        lw, ls, ld = labor.sample_layer(ip, ix, seeds, k, salt)
        assert np.array_equal(where, lw) and np.array_equal(src, ls) and np.array_equal(dst, ld)
        assert (typ == 0).all() and (ix[pos] == dst).all()
    for fanouts in ([5], [5, 4], [3, 4, 5]):
        got = ref.sample_batch(ip, ix, et, seeds, [[f] for f in fanouts], 31)
        want = labor.sample_batch(ip, ix, seeds, fanouts, 31)
        assert np.array_equal(got["input_nodes"], want["input_nodes"])
        for g, w in zip(got["layers"], want["layers"]):
            assert np.array_equal(g["row"], w["row"]) and np.array_equal(g["col"], w["col"])
            assert (g["num_src"], g["num_dst"]) == (w["num_src"], w["num_dst"])
            assert np.array_equal(got["input_nodes"][g["row"]], ix[g["eid"]])


def test_marginals_of_the_reference():
    """One seed, neighbour ids i * 2654435761 % 100003 for i < 25, segments of 8 / 12 / 5 entries, fanouts 2 / 3 / 0, batch
    salts 0 .. 3999, layer 0: every position of the first two segments is drawn 1000 +- 137 times (5 sigma, sigma =
    sqrt(4000 * 1/4 * 3/4)), no position of the third ever."""
    ids = ((np.arange(25, dtype=np.uint64) * np.uint64(2654435761)) % np.uint64(100003)).astype(np.uint32)
    ip = np.array([0, 25], np.uint32)
    et = np.repeat(np.arange(3), [8, 12, 5]).astype(np.uint8)
    picks = np.zeros(25, np.int64)
    for s in range(4000):
        _, _, _, pos, typ = ref.sample_layer(ip, ids, et, [0], [2, 3, 0], labor.layer_salt(s, 0))
        assert pos.size == 5 and typ.tolist() == [0, 0, 1, 1, 1]
        picks[pos] += 1
    dev = np.abs(picks[:20] - 1000).max()
    print("picks of the sampled segments: min", picks[:20].min(), "max", picks[:20].max(), "largest deviation",
          dev / np.sqrt(4000 * 0.25 * 0.75), "sigma")
    assert (picks[20:] == 0).all()
    assert (np.abs(picks[:20] - 1000) <= 137).all()


def test_sort_lists_by_type_and_the_precondition(tmp_path):
    from xgnn_amd import datagen
    rng = np.random.RandomState(2)
    ip, ix, _ = multigraph(seed=2)
    E = ix.size
    et = rng.randint(0, 4, E).astype(np.uint8)
    feat = np.arange(E, dtype=np.float32)
    nix, net, nfeat, perm = datagen.sort_lists_by_type(ip, ix, et, feat)
    assert datagen.first_unsorted_list(ip, net) is None
    assert np.array_equal(nix, ix[perm]) and np.array_equal(net, et[perm]) and np.array_equal(nfeat, feat[perm])
    assert net.dtype == np.uint8
    for v in range(ip.size - 1):  # a permutation inside every list, stable inside a type
        b, e = int(ip[v]), int(ip[v + 1])
        assert sorted(perm[b:e].tolist()) == list(range(b, e))
        for r in range(4):
            assert (np.diff(perm[b:e][net[b:e] == r]) > 0).all()
    # the same return convention as sort_lists_by_time
    tix, tt, tfeat, tperm = datagen.sort_lists_by_time(ip, ix, et.astype(np.uint32), feat)
    assert np.array_equal(tperm, perm) and np.array_equal(tix, nix) and np.array_equal(tfeat, nfeat)
    g = dict(indptr=ip, indices=nix, train_set=np.arange(10, dtype=np.uint32), meta=dict(feat_dim=4, num_class=2))
    d = datagen.write_dataset(str(tmp_path / "ok"), g, minimal=True, edge_type=net, num_edge_type=4)
    assert np.array_equal(np.fromfile(d + "/edge_type.bin", np.uint8), net)
    assert "NUM_EDGE_TYPE\t4\n" in open(d + "/meta.txt").read()
    # an unsorted list, a type >= R, a bad R, a bad length: refused, the first two with the offending node
    v = next(v for v in range(ip.size - 1) if net[int(ip[v])] != net[int(ip[v + 1]) - 1])
    bad = net.copy()
    b, e = int(ip[v]), int(ip[v + 1])
    bad[b:e] = bad[b:e][::-1]
    assert datagen.first_unsorted_list(ip, bad) == v
    with pytest.raises(AssertionError, match=f"node {v}'s list are not non-decreasing"):
        datagen.write_dataset(str(tmp_path / "bad"), g, minimal=True, edge_type=bad, num_edge_type=4)
    first3 = int(np.searchsorted(ip, np.flatnonzero(net == 3)[0], side="right") - 1)
    with pytest.raises(AssertionError, match=f"node {first3}'s list holds a type >= num_edge_type = 3"):
        datagen.write_dataset(str(tmp_path / "bad"), g, minimal=True, edge_type=net, num_edge_type=3)
    for R in (0, 33, None):
        with pytest.raises(AssertionError, match="num_edge_type"):
            datagen.write_dataset(str(tmp_path / "bad"), g, minimal=True, edge_type=net, num_edge_type=R)
    with pytest.raises(AssertionError, match="one type per edge"):
        datagen.write_dataset(str(tmp_path / "bad"), g, minimal=True, edge_type=net[:-1], num_edge_type=4)
    with pytest.raises(AssertionError, match="num_edge_type without edge_type"):
        datagen.write_dataset(str(tmp_path / "bad"), g, minimal=True, num_edge_type=4)


# ---- the C entry points: refusals, all of them before any device call (so they can be seen without a GPU) -----------

def _lib():
    import xgnn_amd
    return xgnn_amd.lib()


def _graph(num_part=0):
    from xgnn_amd import _lib as L
    g = L.Graph()
    g.indptr, g.indices, g.num_node, g.num_part = 0x1000, 0x2000, 100, num_part
    return g


def test_abi_version_sample_type_and_workspace():
    from xgnn_amd import common, ops
    h = _lib()
    assert h.ggms_abi_version() == 3
    assert ops.KHOP_TYPED == 10 and common.kKHopTyped == 10 and common.sample_types["khop_typed"] == 10
    # the generic size serves every R; the call's own is exact for its R (R boundary words + 3 words per seed)
    assert h.ggms_sample_workspace_bytes(10, 1000, 10) >= h.ggms_sample_khop_typed_workspace_bytes(1000, 32)
    assert h.ggms_sample_khop_typed_workspace_bytes(1000, 32) - h.ggms_sample_khop_typed_workspace_bytes(1000, 1) == 31 * 4000
    assert h.ggms_sample_khop_typed_workspace_bytes(1000, 0) == 0 and h.ggms_sample_khop_typed_workspace_bytes(1000, 33) == 0


def test_leaf_refuses_bad_arguments():
    h = _lib()
    ws = h.ggms_sample_khop_typed_workspace_bytes(10, 3)
    P = 0x1000  # never dereferenced: every call below is refused first

    def call(graph=None, et=P, R=3, tf=(2, 0, 3), inp=P, n=10, src=P, dst=P, pos=P, typ=P, num=P, w=P, wb=ws):
        g = graph if graph is not None else _graph()
        f = (C.c_uint32 * len(tf))(*tf) if tf is not None else None
        return h.ggms_sample_khop_typed(C.byref(g), et, R, f, inp, n, 1, src, dst, pos, typ, num, w, wb, None)
    assert call(graph=_graph(num_part=2)) == INVALID  # positions are those of one CSR
    assert call(R=0) == INVALID and call(R=33, tf=(1,) * 33) == INVALID
    assert call(tf=(2, 128, 3)) == INVALID and call(tf=(0, 0, 0)) == INVALID and call(tf=None) == INVALID
    for null in ("et", "inp", "src", "dst", "pos", "typ", "num", "w"):
        assert call(**{null: None}) == INVALID, null
    assert call(wb=ws - 4) == INVALID
    assert b"invalid argument" in h.ggms_last_error()
    # R = 32 with the largest fanouts is within the limits: refused only for its workspace here
    assert call(R=32, tf=(127,) * 32, wb=h.ggms_sample_khop_typed_workspace_bytes(10, 32) - 4) == INVALID


def test_batch_refuses_bad_arguments():
    from xgnn_amd import _lib as L
    h = _lib()
    P = 0x1000
    f = (C.c_size_t * 2)(5, 4)
    ws = h.ggms_sample_batch_typed_workspace_bytes(64, f, 2, 3, None)
    assert ws > 0
    assert h.ggms_sample_batch_typed_workspace_bytes(64, f, 2, 0, None) == 0
    assert h.ggms_sample_batch_typed_workspace_bytes(64, f, 2, 33, None) == 0
    ht = L.HashTable()
    ht.o2n, ht.n2o, ht.num_items_dev, ht.o2n_size, ht.n2o_size, ht.direct = P, P, P, 100, 1 << 20, 1
    ptrs = (C.c_void_p * 2)(P, P)

    def call(graph=None, seeds=P, eid=ptrs, etype=ptrs, et=P, R=3, tf=(2, 0, 3, 1, 3, 0), wb=ws, t=True):
        g = graph if graph is not None else _graph()
        tfa = (C.c_uint32 * len(tf))(*tf) if tf is not None else None
        tt = L.Typed(et, R, tfa)
        return h.ggms_sample_batch_typed(C.byref(g), seeds, 64, f, 2, C.byref(ht), ptrs, ptrs, eid, etype, P,
                                         C.byref(tt) if t else None, None, P, wb, None)
    assert call(graph=_graph(num_part=2)) == INVALID
    assert call(seeds=None) == INVALID and call(eid=None) == INVALID and call(etype=None) == INVALID
    assert call(eid=(C.c_void_p * 2)(P, None)) == INVALID and call(etype=(C.c_void_p * 2)(P, None)) == INVALID
    assert call(et=None) == INVALID and call(tf=None) == INVALID and call(t=False) == INVALID
    assert call(R=0) == INVALID and call(R=33, tf=(1,) * 66) == INVALID
    assert call(tf=(2, 0, 3, 1, 2, 0)) == INVALID  # row 1 sums to 3, fanouts[1] is 4
    f0 = (C.c_size_t * 2)(5, 0)
    tt = L.Typed(P, 3, (C.c_uint32 * 6)(2, 0, 3, 0, 0, 0))
    assert h.ggms_sample_batch_typed(C.byref(_graph()), P, 64, f0, 2, C.byref(ht), ptrs, ptrs, ptrs, ptrs, P, C.byref(tt),
                                     None, P, ws, None) == INVALID  # a zero row
    f128 = (C.c_size_t * 2)(5, 128)
    tt = L.Typed(P, 3, (C.c_uint32 * 6)(2, 0, 3, 128, 0, 0))
    assert h.ggms_sample_batch_typed(C.byref(_graph()), P, 64, f128, 2, C.byref(ht), ptrs, ptrs, ptrs, ptrs, P,
                                     C.byref(tt), None, P, 1 << 30, None) == INVALID  # a k_r >= 128
    assert call(wb=ws - 4) == INVALID
    # the plain batch call refuses the type and names the typed call
    rc = h.ggms_sample_batch(10, C.byref(_graph()), P, 64, f, 2, C.byref(ht), None, 0, ptrs, ptrs, P, None, P, ws, None)
    assert rc == INVALID and b"ggms_sample_batch_typed" in h.ggms_last_error()
    # the raw seeds' local ids: host arithmetic, type 10 included
    out = C.c_void_p()
    assert h.ggms_sample_batch_seed_ids(10, 64, f, 2, None, P, C.byref(out)) == 0 and out.value >= P
