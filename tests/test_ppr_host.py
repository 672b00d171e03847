"""ppr_topk on the host: the integer reference (tests/ppr_ref.py) against the exact PPR vector, its code in the Python
tables, what config + data_init take and refuse by name (no GPU touched), and the C argument checks: GGMS_ERR_INVALID
with a message before any device call."""
import ctypes as C

import numpy as np
import pytest

import ppr_ref as ref
from config_run import ARCH0, run_config
from graphgen import feature_rows, powerlaw_csr
from xgnn_amd import _lib, datagen, lib

NAME = "ppr_topk"
P14 = dict(_sample_type=14, num_neighbor=4)
SLACK = 7.8e-10


def ring(n):
    return np.arange(0, 2 * n + 1, 2, dtype=np.uint32), np.array([[(i - 1) % n, (i + 1) % n] for i in range(n)],
                                                                 np.uint32).reshape(-1)


def path(n):
    lists = [[j for j in (i - 1, i + 1) if 0 <= j < n] for i in range(n)]
    return np.cumsum([0] + [len(l) for l in lists]).astype(np.uint32), np.array(sum(lists, []), np.uint32)


def dangling(n):
    """A power-law graph whose every seventh node has lost its list."""
    ip, ix = powerlaw_csr(n, mean_deg=5, seed=4)
    deg, keep = np.diff(ip.astype(np.int64)), np.ones(ix.size, bool)
    for u in range(0, n, 7):
        keep[ip[u]:ip[u + 1]] = False
    deg[0:n:7] = 0
    return np.cumsum(np.concatenate([[0], deg])).astype(np.uint32), ix[keep]


GRAPHS = dict(ring=ring(50), path=path(40), powerlaw=powerlaw_csr(200, mean_deg=6, seed=3), dangling=dangling(150))


@pytest.mark.parametrize("alpha", [0.05, 0.15, 0.5, 0.95])
@pytest.mark.parametrize("name", list(GRAPHS))
def test_reference_against_exact_ppr(name, alpha):
    """Forward push keeps exact = p + (what the residual still owes), so for every node
    -SLACK <= exact - p / 2^30 <= (2^30 - sum p) / 2^30 + SLACK.  Without rounding both slacks would be 0; the integer
    split (a floored, the remainder kept in r) moves a node's score by less than a unit of 2^-30 per push.  Measured over
    these 16 cases x 3 seeds from the reference alone: the upper side is never exceeded, the lower side by at most
    3.891e-10 (powerlaw, alpha 0.95: the lower bound of 0 holds only up to this rounding); SLACK is twice that.
    eps = 2^-20 and C = 256 >= every graph: no seed is truncated.  Mass conservation: sum r + sum p == 2^30."""
    ip, ix = GRAPHS[name]
    for s in (0, 1, (len(ip) - 1) // 2):
        state, rounds, truncated = ref.push(ip, ix, s, alpha, 2.0 ** -20, 256, 255)
        assert not truncated and rounds >= 1  # (the bound holds after any number of rounds: max_rounds may end them)
        assert sum(r + p for r, p in state.values()) == ref.ONE
        p = np.zeros(len(ip) - 1)
        for u, (_, pu) in state.items():
            p[u] = pu
        diff = ref.exact_ppr(ip, ix, s, alpha) - p / ref.ONE
        assert diff.min() >= -SLACK and diff.max() <= (ref.ONE - p.sum()) / ref.ONE + SLACK, (diff.min(), diff.max())


def test_python_names_and_abi():
    import samgraph.torch as sam
    from xgnn_amd import common, ops
    assert sam.sample_types[NAME] == common.kPPRTopK == ops.PPR_TOPK == 14
    assert callable(ops.sample_ppr) and callable(ops.PprBatchSampler)
    assert lib().ggms_abi_version() == 3


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    root = tmp_path_factory.mktemp("ppr_cfg")
    ip, ix = powerlaw_csr(600, mean_deg=9, seed=2)
    g = dict(indptr=ip, indices=ix, train_set=np.arange(0, 600, 3, dtype=np.uint32), meta=dict(feat_dim=20, num_class=13))
    datagen.write_dataset(str(root / "ok"), g, feat=feature_rows(np.arange(600), 20), label=np.arange(600) % 13)
    return str(root / "ok")


@pytest.mark.parametrize("extra", [{}, dict(induced_subgraph="on"), dict(hash_table="hashed", ppr_alpha=0.95, ppr_eps=1,
                                   ppr_max_nodes=2048, ppr_max_rounds=255, num_neighbor=127)], ids=str)
def test_accepted(dataset, extra):
    out = run_config(dataset, dict(P14, **extra))
    assert out.returncode == 0 and out.stdout.split() == ["configured", "13", "20"], out.stderr[-2000:]


OTHER_ARCH = dict(arch0=ARCH0, arch3=dict(_arch=3, trainer_ctx="cuda:1"), arch4=dict(_arch=4, sampler_ctx="cuda:1"),
                  arch5=dict(_arch=5, num_sample_worker=1, num_train_worker=1), arch6=dict(_arch=6, num_worker=1))
REFUSED = [(a, kw, [a, NAME, "arch1's batches"]) for a, kw in OTHER_ARCH.items()] + [
    ("dist-graph", dict(use_dist_graph=0.5), [NAME, "use_dist_graph", "ONE CSR"]),
    ("link_prediction", dict(task="link_prediction"), ["task = link_prediction", NAME]),
    ("hetero_batch", dict(hetero_batch="on"), ["hetero_batch with _sample_type 14"]),
    ("typed_feat", dict(typed_feat="on"), ["typed_feat without hetero_batch"]),
    ("edge_ids", dict(edge_ids="on"), ["edge_ids", NAME]),
    ("edge_feat", dict(edge_feat="on"), ["edge_feat", NAME]),
    ("exclude_seed_edges", dict(exclude_seed_edges="self"), [NAME, "exclude_seed_edges = self"]),
    ("inline_heads", dict(inline_heads=1), [NAME, "inline_heads = 1"]),
    ("alpha-low", dict(ppr_alpha=0.01), ["ppr_alpha = 0.01"]), ("alpha-high", dict(ppr_alpha=0.99), ["ppr_alpha = 0.99"]),
    ("eps-low", dict(ppr_eps=1e-7), ["ppr_eps = 1e-07"]), ("eps-high", dict(ppr_eps=1.5), ["ppr_eps = 1.5"]),
    ("nodes-low", dict(ppr_max_nodes=32), ["ppr_max_nodes = 32"]),
    ("nodes-odd", dict(ppr_max_nodes=100), ["ppr_max_nodes = 100", "power of two"]),
    ("nodes-high", dict(ppr_max_nodes=4096), ["ppr_max_nodes = 4096", "2048"]),
    ("rounds-low", dict(ppr_max_rounds=0), ["ppr_max_rounds = 0"]),
    ("rounds-high", dict(ppr_max_rounds=256), ["ppr_max_rounds = 256"]),
    ("K-low", dict(num_neighbor=0), ["num_neighbor = 0", NAME]), ("K-high", dict(num_neighbor=128), ["num_neighbor = 128"]),
    ("K-nodes", dict(num_neighbor=64, ppr_max_nodes=64), ["num_neighbor = 64 with ppr_max_nodes = 64"]),
]


@pytest.mark.parametrize("case", REFUSED, ids=[c[0] for c in REFUSED])
def test_refused_by_name(dataset, case):
    _, extra, words = case
    out = run_config(dataset, dict(P14, **extra))
    assert out.returncode < 0 and "configured" not in out.stdout, out.stderr[-2000:]  # SIGABRT, like every fatal
    for w in words:
        assert w in out.stderr, (w, out.stderr[-2000:])


C_REFUSED = [(dict(num_part=2), "unsharded"), (dict(alpha=0.01), "alpha 0.01"), (dict(alpha=0.99), "alpha 0.99"),
             (dict(alpha=float("nan")), "alpha nan"), (dict(eps=2.0 ** -21), "eps "), (dict(eps=1.5), "eps 1.5"),
             (dict(C=32), "max_nodes 32"), (dict(C=100), "max_nodes 100"), (dict(C=4096), "max_nodes 4096"),
             (dict(rounds=0), "max_rounds 0"), (dict(rounds=256), "max_rounds 256"), (dict(K=0), "K 0"),
             (dict(K=128), "K 128"), (dict(K=64, C=64), "K 64"), (dict(ws=64), "workspace_bytes 64")]


@pytest.mark.parametrize("case", C_REFUSED, ids=[c[1].strip().replace(" ", "-") + str(i) for i, c in enumerate(C_REFUSED)])
def test_c_argument_checks_touch_no_device(case):
    """Every pointer is a made-up address: a call that went past its checks would fault or report a HIP error."""
    a = dict(num_part=0, alpha=0.15, eps=1e-4, C=1024, rounds=32, K=4, ws=None)
    a.update(case[0])
    h, fake = lib(), C.c_void_p(0x1000)
    need = h.ggms_sample_ppr_workspace_bytes(10, a["K"])
    g = _lib.Graph(0x1000, 0x1000, None, None, a["num_part"], 0, 100, 0)
    rc = h.ggms_sample_ppr(C.byref(g), fake, 10, a["alpha"], a["eps"], a["C"], a["rounds"], a["K"], fake, fake, fake, fake,
                           None, fake, need if a["ws"] is None else a["ws"], None)
    assert rc == -1 and case[1] in h.ggms_last_error().decode(), h.ggms_last_error().decode()  # GGMS_ERR_INVALID


def test_generic_batch_names_the_ppr_call():
    h, fake = lib(), C.c_void_p(0x1000)
    g, ht, f, ptrs = _lib.Graph(0x1000, 0x1000, None, None, 0, 0, 100, 0), _lib.HashTable(), (C.c_size_t * 1)(4), (C.c_void_p * 1)(0x1000)
    rc = h.ggms_sample_batch(14, C.byref(g), fake, 10, f, 1, C.byref(ht), None, 0, ptrs, ptrs, fake, None, fake, 1 << 30, None)
    assert rc == -1 and "ggms_sample_batch_ppr" in h.ggms_last_error().decode()
