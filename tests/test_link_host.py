"""Link-prediction seeds on the host: the numpy statement (tests/link_ref.py) checked against the definition's own
examples, the uniformity of its candidates, the argument errors of ggms_link_seeds and ggms_sample_batch_seed_ids
(no GPU touched), and which configurations take `task = link_prediction`."""
import ctypes as C

import numpy as np
import pytest

import link_ref as ref
from config_run import ARCH0, run_config
from test_engine import make_dataset
from xgnn_amd import _lib
from xgnn_amd._lib import Graph, lib

INVALID = -1  # GGMS_ERR_INVALID


@pytest.fixture(scope="module")
def g64():
    """64 nodes: empty rows at the start (0, 1), in the middle (10 .. 12, 30) and at the end (62, 63); list lengths
    1 .. 9 elsewhere, a self-loop at node 5 and a multi-edge at node 6."""
    rng = np.random.RandomState(64)
    empty = {0, 1, 10, 11, 12, 30, 62, 63}
    lists = [[] if v in empty else rng.randint(0, 64, 1 + v % 9).tolist() for v in range(64)]
    lists[5][0] = 5
    lists[6] = [9, 9, 40, 9]
    return ref.graph_of_lists(lists)


def test_salt_and_candidate_vectors():
    assert ref.engine_salt(42, 3, 17) == int(ref.fmix32(0xDA2897D6 ^ 0x6C696E6B))
    # cand by hand: h0 = fmix32(e ^ salt), h = fmix32(h0 + golden * (8 j + a + 1)), (h * N) >> 32
    e, salt, N = 12345, 0xDEADBEEF, 1000
    h0 = int(ref.fmix32(e ^ salt))
    for j, a in [(0, 0), (0, 7), (3, 2), (63, 7)]:
        h = int(ref.fmix32((h0 + 0x9E3779B9 * (8 * j + a + 1)) & 0xFFFFFFFF))
        assert int(ref.cand(e, j, a, salt, N)) == (h * N) >> 32 < N
    assert ref.cand(7, np.arange(64)[:, None], np.arange(8)[None, :], 1, 1 << 31).shape == (64, 8)


def test_endpoints_of_the_reference(g64):
    ip, ix = g64
    E = int(ip[-1])
    assert ref.edge_endpoints(ip, ix, 0) == (2, int(ix[0]))           # edge 0 belongs to the first non-empty row
    assert ref.edge_endpoints(ip, ix, E - 1) == (61, int(ix[E - 1]))  # edge E - 1 to the last non-empty one
    for v in range(64):
        b, e = int(ip[v]), int(ip[v + 1])
        if b == e:
            continue
        assert ref.edge_endpoints(ip, ix, b) == (v, int(ix[b]))          # first edge of a list
        assert ref.edge_endpoints(ip, ix, e - 1) == (v, int(ix[e - 1]))  # last edge of a list
    for v in (2, 13, 31):  # rows that follow empty rows
        assert ip[v] == ip[v - 1] and ref.edge_endpoints(ip, ix, int(ip[v]))[0] == v
    out, forced = ref.link_seeds(ip, ix, [0, E - 1, int(ip[13]), E, E + 5], 3, ref.UNIFORM, 9)
    src, dst, neg = ref.split(out, 3)
    assert src.tolist() == [2, 61, 13, ref.EMPTY, ref.EMPTY] and dst.tolist()[:3] == [ix[0], ix[E - 1], ix[ip[13]]]
    assert (neg[3:] == ref.EMPTY).all() and (neg[:3] < 64).all() and forced == 0


@pytest.mark.parametrize("K", [1, 5, 64])
def test_exclusion_and_forced_rule_of_the_reference(g64, K):
    ip, ix = g64
    E = int(ip[-1])
    salt = 0x1234 + K
    out, forced = ref.link_seeds(ip, ix, np.arange(E), K, ref.EXCLUDE, salt)
    src, _, neg = ref.split(out, K)
    uni, _ = ref.link_seeds(ip, ix, np.arange(E), K, ref.UNIFORM, salt)
    seen_forced = retried = 0
    for e in range(E):
        u = int(src[e])
        banned = set(ix[ip[u]:ip[u + 1]].tolist()) | {u}
        for j in range(K):
            w = int(neg[e, j])
            c = ref.cand(e, j, np.arange(8), salt, 64).tolist()
            if w in banned:  # only a forced negative may be banned: all eight candidates were, and it is the last
                assert all(x in banned for x in c) and w == c[7]
                seen_forced += 1
            else:            # the first candidate that is not banned
                first = next(a for a in range(8) if c[a] not in banned)
                assert w == c[first]
                retried += first > 0
            assert int(ref.split(uni, K)[2][e, j]) == c[0]  # mode 0: attempt 0, nothing rejected
    assert seen_forced == forced and retried > 0


def test_complete_graph_forces_every_negative():
    ip, ix = ref.complete_graph(8)
    eids = np.array([0, 55, 7, 7, 20], np.int64)
    out, forced = ref.link_seeds(ip, ix, eids, 5, ref.EXCLUDE, 77)
    assert forced == eids.size * 5
    for i, e in enumerate(eids):
        assert ref.split(out, 5)[2][i].tolist() == ref.cand(e, np.arange(5), 7, 77, 8).tolist()
    assert ref.split(out, 5)[2][2].tolist() == ref.split(out, 5)[2][3].tolist()  # keyed by the edge id, not its place


@pytest.mark.parametrize("N,K", [(64, 4), (257, 16)])
def test_candidates_are_uniform_over_the_nodes(N, K):
    """Mode 0, one fixed edge, salts 0 .. 4095: every node is drawn 4096 K / N times, within 5 standard deviations of
    the binomial."""
    n = 4096 * K
    count = np.zeros(N, np.int64)
    for s in range(4096):
        count += np.bincount(ref.cand(37, np.arange(K), 0, s, N), minlength=N)
    p = 1.0 / N
    dev = np.abs(count - n * p) / np.sqrt(n * p * (1 - p))
    print(f"N {N} K {K}: worst deviation {dev.max():.2f} sd")
    assert count.sum() == n and dev.max() <= 5.0


def test_first_occurrence_ranks():
    ids, uniq = ref.first_occurrence_ranks(np.array([7, 3, 7, 9, 3, 3, 1], np.uint32))
    assert ids.tolist() == [0, 1, 0, 2, 1, 1, 3] and uniq.tolist() == [7, 3, 9, 1]


def test_link_seeds_argument_errors():
    l = lib()
    call = l.ggms_link_seeds
    p = C.c_void_p(1 << 20)  # never dereferenced: the checks come first
    g = Graph()
    g.indptr, g.indices, g.num_node = 1 << 22, 1 << 23, 1000
    for bad in (0, 65):
        assert call(C.byref(g), p, 10, bad, 1, 0, p, None, None) == INVALID
        assert b"num_negative" in l.ggms_last_error()
    assert call(C.byref(g), p, 10, 5, 2, 0, p, None, None) == INVALID       # unknown mode
    assert call(C.byref(g), p, 10, 5, -1, 0, p, None, None) == INVALID
    assert call(None, p, 10, 5, 1, 0, p, None, None) == INVALID             # no graph
    assert call(C.byref(g), None, 10, 5, 1, 0, p, None, None) == INVALID    # no edge ids
    assert call(C.byref(g), p, 10, 5, 1, 0, None, None, None) == INVALID    # no output
    assert call(C.byref(Graph()), p, 10, 5, 1, 0, p, None, None) == INVALID  # no CSR
    sharded = Graph()
    sharded.indptr, sharded.indices, sharded.num_node, sharded.num_part = 1 << 22, 1 << 23, 1000, 2
    assert call(C.byref(sharded), p, 10, 5, 1, 0, p, None, None) == INVALID
    assert b"num_part" in l.ggms_last_error()
    # nothing to do is fine, with the argument checks still in front of it
    assert call(C.byref(g), None, 0, 5, 1, 0, None, None, None) == 0
    assert call(C.byref(g), None, 0, 65, 1, 0, None, None, None) == INVALID
    assert call(C.byref(sharded), None, 0, 5, 1, 0, None, None, None) == INVALID


@pytest.mark.parametrize("sample_type", [0, 5, 7, 8], ids=["khop0", "khop2", "khop3", "khop_labor"])
@pytest.mark.parametrize("num_seeds,fanouts", [(1, [3]), (1285, [3, 2]), (40000, [15, 10, 5])])
def test_seed_ids_address_lies_inside_the_workspace(sample_type, num_seeds, fanouts):
    l = lib()
    L = len(fanouts)
    f = (C.c_size_t * L)(*fanouts)
    need = l.ggms_sample_batch_workspace_bytes(sample_type, num_seeds, f, L, None)
    assert need > 0
    for base in (1 << 30, (1 << 30) + 4, (1 << 30) + 12):  # the batch aligns its workspace to 16 bytes itself
        out = C.c_void_p()
        assert l.ggms_sample_batch_seed_ids(sample_type, num_seeds, f, L, None, C.c_void_p(base), C.byref(out)) == 0
        assert out.value % 16 == 0 and base <= out.value and out.value + 4 * num_seeds <= base + need


def test_seed_ids_argument_errors():
    l = lib()
    f = (C.c_size_t * 2)(3, 2)
    p, out = C.c_void_p(1 << 20), C.c_void_p()
    call = l.ggms_sample_batch_seed_ids
    assert call(7, 100, None, 2, None, p, C.byref(out)) == INVALID     # no fanouts
    assert call(7, 100, f, 2, None, None, C.byref(out)) == INVALID     # no workspace
    assert call(7, 100, f, 2, None, p, None) == INVALID                # nowhere to put the address
    assert call(7, 100, f, 0, None, p, C.byref(out)) == INVALID        # layer counts as ggms_sample_batch's
    assert call(7, 100, f, 17, None, p, C.byref(out)) == INVALID
    assert call(42, 100, f, 2, None, p, C.byref(out)) == INVALID       # unknown sample type
    extra = _lib.SampleExtra()
    assert call(7, 100, f, 2, C.byref(extra), p, C.byref(out)) == 0 and out.value is not None


def test_bindings_and_codes():
    import samgraph.torch as sam
    from xgnn_amd import ops
    assert (ops.NEG_UNIFORM, ops.NEG_EXCLUDE) == (ref.UNIFORM, ref.EXCLUDE) == (0, 1)
    assert callable(sam.get_graph_link_pairs) and callable(sam.get_graph_seed_ids) and callable(sam.num_negative)
    text = open(__file__.replace("tests/test_link_host.py", "include/ggms.h")).read()
    assert "#define GGMS_NEG_UNIFORM 0" in text and "#define GGMS_NEG_EXCLUDE 1" in text


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    return make_dataset(tmp_path_factory.mktemp("link_ds"))


LINK = dict(task="link_prediction")
DEDICATED = dict(sampler_ctx='cuda:0', trainer_ctx='cuda:1')


def test_arch1_takes_the_task(dataset):
    for extra in (LINK, dict(LINK, num_negative=64, negative_mode="uniform"), dict(task="node_classification"),
                  dict(LINK, _sample_type=8), dict(num_negative=99)):  # (without the task the key is not read)
        out = run_config(dataset["path"], dict(extra))
        assert out.returncode == 0, out.stderr[-2000:]
        assert out.stdout.split()[:3] == ["configured", "13", "20"]


@pytest.mark.parametrize("arch,extra", [
    ("arch0", ARCH0), ("arch3", dict(DEDICATED, _arch=3)),
    ("arch4", dict(_arch=4, sampler_ctx='cuda:1', trainer_ctx='cuda:0')),
    ("arch5", dict(_arch=5, num_sample_worker=1, num_train_worker=1)), ("arch6", dict(_arch=6, num_worker=1))])
def test_other_deployments_refuse_the_task_by_name(dataset, arch, extra):
    out = run_config(dataset["path"], dict(extra, **LINK))
    assert out.returncode != 0 and "configured" not in out.stdout
    assert arch in out.stderr and "task" in out.stderr and "link_prediction" in out.stderr, out.stderr[-2000:]


@pytest.mark.parametrize("key,value", [("num_negative", 0), ("num_negative", 65), ("num_negative", -3),
                                       ("num_negative", "many"), ("negative_mode", "degree"), ("task", "ranking")])
def test_bad_values_are_refused_by_key(dataset, key, value):
    out = run_config(dataset["path"], dict(LINK, **{key: value}))
    assert out.returncode != 0 and "configured" not in out.stdout
    assert key in out.stderr and str(value) in out.stderr, out.stderr[-2000:]


def test_random_walk_is_refused_with_the_task(dataset):
    walk = dict(_sample_type=3, random_walk_length=3, random_walk_restart_prob=0.5, num_random_walk=4, num_neighbor=5)
    out = run_config(dataset["path"], dict(LINK, **walk))
    assert out.returncode != 0 and "configured" not in out.stdout
    assert "task" in out.stderr and "random_walk" in out.stderr, out.stderr[-2000:]


def test_train_edge_set_is_checked_at_load(dataset, tmp_path):
    """An id beyond the edge count is fatal at load, by file name; a dataset without the file is taken (every edge)."""
    import shutil
    E = dataset["ix"].size
    path = str(tmp_path / "ds")
    shutil.copytree(dataset["path"], path)
    np.arange(E - 700, E, dtype=np.uint32).tofile(path + "/train_edge_set.bin")
    out = run_config(path, dict(LINK))
    assert out.returncode == 0 and "configured" in out.stdout, out.stderr[-2000:]
    np.array([3, E, 5], np.uint32).tofile(path + "/train_edge_set.bin")
    out = run_config(path, dict(LINK))
    assert out.returncode != 0 and "configured" not in out.stdout
    assert "train_edge_set.bin" in out.stderr and str(E) in out.stderr, out.stderr[-2000:]
    out = run_config(path, dict(task="node_classification"))  # the file is the link task's: nobody else reads it
    assert out.returncode == 0, out.stderr[-2000:]
