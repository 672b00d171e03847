"""ggms_link_seeds_typed on the GPU against its numpy statement (tests/link_typed_ref.py), bit for bit: endpoints,
relations and the forced count on link_typed_ref.edge_case_graph -- every segment length at which the search or the
chunked walk changes shape, at the head, in the middle and at the tail of a list, the hub, the forced cases and the
relation that must not reject; later grid rounds; the uniformity of typed_uniform over a type of 32 nodes."""
import numpy as np
import pytest

import link_ref as ref
import link_typed_ref as tref
from test_gpu_link_seeds import dev, host_u32, ops  # noqa: F401  (fixture)

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
GRID_CAP = 3  # GGMS_DEBUG_GRID_CAP
MODES = {"uniform": tref.TYPED_UNIFORM, "exclude": tref.TYPED_EXCLUDE}


@pytest.fixture(scope="module")
def graph(ops):
    ip, ix, et, nt, T, cases = tref.edge_case_graph()
    nodes, base = ops.type_lists(torch.from_numpy(nt).cuda(), T)
    np.testing.assert_array_equal(host_u32(nodes), tref.type_lists(nt, T)[0])
    return dict(ip=ip, ix=ix, et=et, nt=nt, T=T, cases=cases, g=ops.DeviceGraph(dev(ip), dev(ix)),
                args=(torch.from_numpy(et).cuda(), torch.from_numpy(nt).cuda(), nodes, base))


def check(ops, d, eids, K, mode, salt):
    """GPU == twin; returns (src, dst, neg, forced) of the GPU"""
    out, rel, forced = ops.link_seeds_typed(d["g"], *d["args"], dev(eids), K, mode, salt)
    want, want_rel, want_forced = tref.link_seeds_typed(d["ip"], d["ix"], d["et"], d["nt"], d["T"], eids, K, mode, salt)
    np.testing.assert_array_equal(host_u32(out), want)
    np.testing.assert_array_equal(rel.cpu().numpy(), want_rel)
    assert int(forced.item()) == want_forced and ops.device_status() == 0
    src, dst, neg = ref.split(host_u32(out), K)
    ok = dst != ref.EMPTY
    assert (d["nt"][neg[ok]] == d["nt"][dst[ok]][:, None]).all()  # every negative is of its positive destination's type
    return src, dst, neg, want_forced


@pytest.mark.parametrize("salt", [0x1234, 0xA5A5F00D])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("K", [1, 5, 64])
def test_equals_the_reference(ops, graph, K, mode, salt):
    """every segment's first and last position, edge 0, E - 1, ids >= E between them, and random base edges"""
    E = int(graph["ip"][-1])
    eids = np.array(sorted(graph["cases"].values()) + [E, 0, E + 7, E - 1, 0xFFFFFFFF]
                    + np.random.RandomState(K).randint(0, E, 40).tolist(), np.uint32)
    src, dst, neg, forced = check(ops, graph, eids, K, MODES[mode], salt)
    c, x = graph["cases"], {int(e): i for i, e in enumerate(eids.tolist())}
    if mode == "exclude":
        # one node of the type, all nodes of the type in the segment: every negative is forced
        assert forced >= 3 * K and (neg[x[c["single.0a"]]] == dst[x[c["single.0a"]]]).all()
        # G1 .. G3 are u's neighbours under ANOTHER relation: they are drawn, G0 (the positive) is not
        drawn = set(neg[x[c["other.0a"]]].tolist())
        assert drawn <= set(graph["ix"][c["other.1a"]:c["other.1z"] + 1].tolist()) and (K < 64 or len(drawn) == 3)
    elif K == 64:  # the source is of the destination's type and is drawn
        assert src[x[c["g3"]]] in neg[x[c["g3"]]]


@pytest.mark.parametrize("cap", [1, 3])
def test_later_grid_rounds(ops, graph, cap):
    from xgnn_amd import lib
    eids = np.random.RandomState(cap).randint(0, int(graph["ip"][-1]) + 50, 3400).astype(np.uint32)
    lib().ggms_debug_set_knob(GRID_CAP, cap)
    try:
        check(ops, graph, eids, 5, tref.TYPED_EXCLUDE, 99)
    finally:
        lib().ggms_debug_set_knob(GRID_CAP, -1)


def test_typed_uniform_is_uniform_over_the_type(ops, graph):
    """one positive into the type of 32 nodes, K = 64, 2000 salts: n = 128 000 draws, p = 1 / 32, every node's count
    within 5 sigma = 5 sqrt(n p (1 - p)) = 311 of n p = 4000"""
    e, salts = dev(np.array([graph["cases"]["all.0a"]], np.uint32)), 2000
    neg = torch.stack([ops.link_seeds_typed(graph["g"], *graph["args"], e, 64, tref.TYPED_UNIFORM, 7919 * s)[0][2:]
                       for s in range(salts)])
    count = np.bincount(host_u32(neg.flatten()).astype(np.int64) - (tref.N_BASE + 1), minlength=32)
    n, p = salts * 64, 1 / 32
    print("counts", count.min(), count.max())
    assert count.size == 32 and np.abs(count - n * p).max() <= 5 * np.sqrt(n * p * (1 - p))
