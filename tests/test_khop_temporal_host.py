"""khop_temporal without a GPU: the numpy statement (tests/khop_temporal_ref.py) against a brute-force loop and against
khop_labor_ref where the two must agree, the batch's cut rule and its no-leak property, the uniform marginals, datagen's
time-sorted CSR, and the argument refusals of the C entry points (all made before any device call)."""
import ctypes as C

import numpy as np
import pytest

import khop_labor_ref as labor
import khop_temporal_ref as ref

INF = ref.INF
INVALID = -1  # GGMS_ERR_INVALID


def multigraph(num_node=200, seed=0, max_deg=60, num_id=None):
    """Lists of random length with many parallel edges (ids from a small range), times sorted inside every list."""
    rng = np.random.RandomState(seed)
    deg = rng.randint(0, max_deg, num_node)
    deg[rng.randint(0, num_node, 5)] = 0
    ip = np.zeros(num_node + 1, np.uint32)
    ip[1:] = np.cumsum(deg)
    ix = rng.randint(0, num_id or num_node, int(ip[-1])).astype(np.uint32)
    return ip, ix, ref.sorted_times(ip, rng, 1, 40)


def brute_positions(ids, times, cut, fanout, salt, pick):
    """The definition, entry by entry: eligible = time < cut; UNIFORM = the fanout smallest (hash, position) pairs."""
    elig = [p for p in range(len(ids)) if int(times[p]) < cut]
    if pick == ref.RECENT:
        return elig[max(0, len(elig) - fanout):]
    keyed = sorted((int(labor.fmix32(int(ids[p]) ^ salt)), p) for p in elig)
    return sorted(p for _, p in keyed[:fanout])


@pytest.mark.parametrize("pick", [ref.UNIFORM, ref.RECENT], ids=["uniform", "recent"])
def test_reference_equals_the_brute_force_loop(pick):
    ip, ix, et = multigraph()
    rng = np.random.RandomState(1)
    seeds = rng.randint(0, 200, 300).astype(np.uint32)
    cuts = rng.randint(0, 45, 300).astype(np.uint32)
    cuts[:6] = [0, 1, INF, 40, 39, 2]
    for fanout, salt in ((1, 7), (5, 0x4329F67E), (127, 3)):
        where, src, dst, pos = ref.sample_layer(ip, ix, et, seeds, cuts, fanout, salt, pick)
        k = 0
        for j, (s, c) in enumerate(zip(seeds.tolist(), cuts.tolist())):
            b, e = int(ip[s]), int(ip[s + 1])
            want = brute_positions(ix[b:e], et[b:e], c, fanout, salt, pick)
            got = pos[where == j]
            assert got.tolist() == [b + p for p in want], (j, s, c)
            assert (et[got] < c).all() and (ix[got] == dst[where == j]).all() and (src[where == j] == s).all()
            k += len(want)
        assert k == pos.size


def test_sort_lists_by_time_and_the_precondition(tmp_path):
    from xgnn_amd import datagen
    rng = np.random.RandomState(2)
    ip, ix, _ = multigraph(seed=2)
    E = ix.size
    t = rng.randint(0, 30, E).astype(np.uint32)
    feat = np.arange(E, dtype=np.float32)
    six, st, sfeat, perm = datagen.sort_lists_by_time(ip, ix, t, feat)
    assert sorted(perm.tolist()) == list(range(E))
    np.testing.assert_array_equal(six, ix[perm])
    np.testing.assert_array_equal(st, t[perm])
    np.testing.assert_array_equal(sfeat, feat[perm])
    for v in range(ip.size - 1):
        b, e = int(ip[v]), int(ip[v + 1])
        assert ((perm[b:e] >= b) & (perm[b:e] < e)).all()  # a list keeps its edges
        assert (np.diff(st[b:e].astype(np.int64)) >= 0).all()
        same = np.flatnonzero(np.diff(st[b:e].astype(np.int64)) == 0)
        assert (perm[b:e][same] < perm[b:e][same + 1]).all()  # stable: equal times keep their order
    assert datagen.first_unsorted_list(ip, st) is None
    # a decrease ACROSS two lists is fine, one inside a list is named by its node
    deg = np.diff(ip.astype(np.int64))
    v = int(np.flatnonzero(deg >= 3)[4])
    bad = st.copy()
    bad[ip[v] + 1] = bad[ip[v] + 2] + 1
    assert datagen.first_unsorted_list(ip, bad) == v
    g = dict(indptr=ip, indices=six, train_set=np.arange(10, dtype=np.uint32), meta=dict(feat_dim=4, num_class=2))
    datagen.write_dataset(str(tmp_path / "ok"), g, minimal=True, edge_time=st)
    np.testing.assert_array_equal(np.fromfile(str(tmp_path / "ok" / "edge_time.bin"), dtype="<u4"), st)
    with pytest.raises(AssertionError, match=f"node {v}'s list"):
        datagen.write_dataset(str(tmp_path / "bad"), g, minimal=True, edge_time=bad)


@pytest.mark.parametrize("fanouts", [[5], [5, 4], [3, 4, 5]], ids=["L1", "L2", "L3"])
def test_no_cut_equals_khop_labor(fanouts):
    """cut = +inf on every seed: leaf and batch are khop_labor's, edge for edge."""
    ip, ix, et = multigraph(seed=3)
    seeds = np.random.RandomState(3).randint(0, 200, 120).astype(np.uint32)
    inf = np.full(seeds.size, INF, np.uint32)
    where, src, dst, pos = ref.sample_layer(ip, ix, et, seeds, inf, fanouts[0], 99)
    lw, ls, ld = labor.sample_layer(ip, ix, seeds, fanouts[0], 99)
    assert (where.tolist(), src.tolist(), dst.tolist()) == (lw.tolist(), ls.tolist(), ld.tolist())
    assert (ix[pos] == dst).all()
    got = ref.sample_batch(ip, ix, et, seeds, inf, fanouts, 1234)
    want = labor.sample_batch(ip, ix, seeds, fanouts, 1234)
    np.testing.assert_array_equal(got["input_nodes"], want["input_nodes"])
    assert (got["node_cut"] == INF).all()
    for g, w in zip(got["layers"], want["layers"]):
        for key in ("row", "col"):
            np.testing.assert_array_equal(g[key], w[key])
        assert (g["num_src"], g["num_dst"]) == (w["num_src"], w["num_dst"])


@pytest.mark.parametrize("T", [0, 1, 17, 40, 41])
def test_one_time_for_all_seeds_is_khop_labor_on_the_filtered_graph(T):
    ip, ix, et = multigraph(seed=4)
    fip, fix, back = ref.filtered_csr(ip, ix, et, T)
    seeds = np.random.RandomState(T).randint(0, 200, 150).astype(np.uint32)
    cuts = np.full(seeds.size, T, np.uint32)
    where, src, dst, pos = ref.sample_layer(ip, ix, et, seeds, cuts, 6, 5)
    lw, ls, ld = labor.sample_layer(fip, fix, seeds, 6, 5)
    assert (where.tolist(), src.tolist(), dst.tolist()) == (lw.tolist(), ls.tolist(), ld.tolist())
    # positions mapped back: the filtered graph's selected positions, in the original CSR
    fpos = np.concatenate([fip[s] + labor.select_positions(fix[fip[s]:fip[s + 1]], 6, 5) for s in seeds.tolist()] or
                          [np.zeros(0, np.int64)]).astype(np.int64)
    np.testing.assert_array_equal(back[fpos], pos)
    fanouts = [4, 3]
    got = ref.sample_batch(ip, ix, et, seeds, cuts, fanouts, 77)
    want = labor.sample_batch(fip, fix, seeds, fanouts, 77)
    np.testing.assert_array_equal(got["input_nodes"], want["input_nodes"])
    assert (got["node_cut"] == T).all()
    for g, w in zip(got["layers"], want["layers"]):
        np.testing.assert_array_equal(g["row"], w["row"])
        np.testing.assert_array_equal(g["col"], w["col"])
        assert (et[g["eid"]] < T).all()


def check_no_leak(b, et, seeds, seed_time):
    """What "no leak" means for a batch `b` in khop_temporal_ref.sample_batch's form.
    reach_i[v] = the smallest time among the roots whose computation tree holds node v as an input of layer i (a root
    holds itself at every depth: a block's destination nodes are among its sources).  Then, for every layer i:
      the cut a frontier node was sampled with is at most reach_i of that node  (never later than a root it serves);
      every edge lies strictly before the cut its col was sampled with          (hence before every such root);
      the final cut of its row is at most that cut                              (the row's own samples come earlier).
    The FINAL cuts (node_cut) are the minimum over all layers: node_cut <= every snapshot.  They are NOT what an edge
    is compared with: an edge f -> t of this very layer may lower f's own final cut below the snapshot f was sampled
    with (t reaches f later, or f is a seed that another, earlier seed samples), which leaks nothing -- that lower cut
    governs the samples f's NEW role needs, and those are drawn in the layers after this one."""
    L = len(b["layers"])
    n = b["input_nodes"].size
    reach = np.full(n, np.iinfo(np.int64).max, np.int64)
    np.minimum.at(reach, b["seed_local"], np.asarray(seed_time, dtype=np.int64))
    final = b["node_cut"].astype(np.int64)
    for i in range(L - 1, -1, -1):
        lay = b["layers"][i]
        start = lay["cut_at_start"].astype(np.int64)
        assert (start <= reach[: start.size]).all(), f"layer {i}: a node was sampled with a cut later than a root it serves"
        assert (final[: start.size] <= start).all()
        t = et[lay["eid"]].astype(np.int64)
        assert (t < start[lay["col"]]).all(), f"layer {i}: an edge at or after its col's cut"
        assert (final[lay["row"]] <= start[lay["col"]]).all(), f"layer {i}: a row's cut above its col's"
        np.minimum.at(reach, lay["row"], reach[lay["col"]])


@pytest.mark.parametrize("pick", [ref.UNIFORM, ref.RECENT], ids=["uniform", "recent"])
@pytest.mark.parametrize("fanouts", [[5], [5, 4], [3, 4, 5]], ids=["L1", "L2", "L3"])
def test_batch_reference_never_leaks(fanouts, pick):
    ip, ix, et = multigraph(seed=5)
    rng = np.random.RandomState(len(fanouts))
    seeds = rng.randint(0, 200, 150).astype(np.uint32)
    seed_time = rng.randint(0, 45, 150).astype(np.uint32)
    seeds[100:] = seeds[:50]  # repeats with other times: sampled with the smaller one
    b = ref.sample_batch(ip, ix, et, seeds, seed_time, fanouts, 31, pick)
    check_no_leak(b, et, seeds, seed_time)
    L = len(fanouts)
    first = b["layers"][L - 1]
    for j in (0, 17, 49):
        both = min(int(seed_time[j]), int(seed_time[100 + j]))
        assert first["cut_at_start"][b["seed_local"][j]] <= both
    assert (b["input_nodes"][b["seed_local"]] == seeds).all()


def test_uniform_marginals_of_the_reference():
    """A list of 100 ids of which 40 are eligible, fanout 10, 4000 batch salts: every eligible position is picked
    1000 +- 137 times (5 sigma of Binomial(4000, 1/4)), no ineligible position ever."""
    rng = np.random.RandomState(9)
    ids = rng.permutation(1 << 20)[:100].astype(np.uint32)
    ip = np.array([0, 100], np.uint32)
    et = np.concatenate([np.arange(40) // 4, 50 + np.arange(60) // 4]).astype(np.uint32)  # 40 before cut 50, with ties
    picks = np.zeros(100, np.int64)
    for s in range(4000):
        salt = labor.layer_salt(labor.batch_salt(42, 0, s), 0)
        _, _, _, pos = ref.sample_layer(ip, ids, et, [0], [50], 10, salt)
        assert pos.size == 10
        picks[pos] += 1
    print("picks of the eligible positions: min", picks[:40].min(), "max", picks[:40].max())
    assert (picks[40:] == 0).all()
    assert (np.abs(picks[:40] - 1000) <= 137).all()


# ---- the C entry points: refusals, all of them before any device call (so they can be seen without a GPU) -----------

def _lib():
    import xgnn_amd
    return xgnn_amd.lib()


def _graph(num_part=0):
    from xgnn_amd import _lib as L
    g = L.Graph()
    g.indptr, g.indices, g.num_node, g.num_part = 0x1000, 0x2000, 100, num_part
    return g


def test_abi_version_and_sample_type():
    from xgnn_amd import ops
    assert _lib().ggms_abi_version() == 3
    assert ops.KHOP_TEMPORAL == 9 and (ops.PICK_UNIFORM, ops.PICK_RECENT) == (0, 1)
    assert _lib().ggms_sample_workspace_bytes(9, 1000, 10) >= 4 * 1000 * 4


def test_leaf_refuses_bad_arguments():
    h = _lib()
    ws = h.ggms_sample_workspace_bytes(9, 10, 5)
    P = 0x1000  # never dereferenced: every call below is refused first

    def call(graph=None, edge_time=P, inp=P, cut=P, n=10, fanout=5, pick=0, src=P, dst=P, pos=P, num=P, w=P, wb=ws):
        g = graph if graph is not None else _graph()
        return h.ggms_sample_khop_temporal(C.byref(g), edge_time, inp, cut, n, fanout, pick, 1, src, dst, pos, num, w, wb,
                                           None)
    assert call(graph=_graph(num_part=2)) == INVALID  # positions are those of one CSR
    assert call(fanout=0) == INVALID and call(fanout=128) == INVALID
    assert call(pick=2) == INVALID and call(pick=-1) == INVALID
    for null in ("edge_time", "inp", "cut", "src", "dst", "pos", "num", "w"):
        assert call(**{null: None}) == INVALID, null
    assert call(wb=ws - 4) == INVALID
    assert b"invalid argument" in h.ggms_last_error()


def test_batch_refuses_bad_arguments():
    from xgnn_amd import _lib as L
    h = _lib()
    P = 0x1000
    f = (C.c_size_t * 2)(5, 4)
    ws = h.ggms_sample_batch_temporal_workspace_bytes(64, f, 2, None)
    assert ws > 0
    ht = L.HashTable()
    ht.o2n, ht.n2o, ht.num_items_dev, ht.o2n_size, ht.n2o_size, ht.direct = P, P, P, 100, 1 << 20, 1
    ptrs = (C.c_void_p * 2)(P, P)

    def call(graph=None, seeds=P, times=P, eid=ptrs, node_cut=P, stamp=1, pick=0, edge_time=P, table=P, wb=ws, t=True):
        g = graph if graph is not None else _graph()
        tt = L.Temporal(edge_time, table, stamp, pick)
        return h.ggms_sample_batch_temporal(C.byref(g), seeds, times, 64, f, 2, C.byref(ht), ptrs, ptrs, eid, node_cut, P,
                                            C.byref(tt) if t else None, None, P, wb, None)
    assert call(graph=_graph(num_part=2)) == INVALID
    assert call(seeds=None) == INVALID and call(times=None) == INVALID and call(eid=None) == INVALID and call(node_cut=None) == INVALID
    assert call(eid=(C.c_void_p * 2)(P, None)) == INVALID
    assert call(stamp=0) == INVALID and call(pick=2) == INVALID and call(edge_time=None) == INVALID and call(table=None) == INVALID
    assert call(t=False) == INVALID and call(wb=ws - 4) == INVALID
    # the plain batch call refuses the type and names the temporal call
    rc = h.ggms_sample_batch(9, C.byref(_graph()), P, 64, f, 2, C.byref(ht), None, 0, ptrs, ptrs, P, None, P, ws, None)
    assert rc == INVALID and b"ggms_sample_batch_temporal" in h.ggms_last_error()
    # the raw seeds' local ids: host arithmetic, type 9 included
    out = C.c_void_p()
    assert h.ggms_sample_batch_seed_ids(9, 64, f, 2, None, P, C.byref(out)) == 0 and out.value >= P
