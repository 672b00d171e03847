"""khop_budget on the GPU against its numpy statement (tests/khop_budget_ref.py), bit for bit: src, dst, pos, the
count, M, the number chosen, and the map all zero afterwards.  One graph: a fan of 40 nodes whose lists all hold the
same 20 targets (M is known: budgets of M - 1, M, M + 1; a candidate shared by more than 64 seeds of one tile), a list
with parallel edges, a node of degree 0, a hub list of 5000 entries (longer than an edge tile and than a wave's list)
and one of 9000 distinct targets (more eligible entries than the hub's LDS buffer), in front of a power-law graph of 4000
nodes (more than 2048 candidates)."""
import numpy as np
import pytest

import khop_budget_ref as ref
from graphgen import powerlaw_csr

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

FAN, MULTI, EMPTY, HUB, WIDE, RANDOM, NRAND = 0, 40, 41, 42, 43, 44, 10000
FAN_M = 20


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (run with -m gpu on an MI355X box)")
    from xgnn_amd import ops as _ops
    return _ops


def dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def zoo():
    rng = np.random.RandomState(7)
    lists = [[RANDOM + 100 + j for j in range(FAN_M)] for _ in range(40)]               # 0 .. 39: the fan
    lists += [[RANDOM + 5, RANDOM + 5, RANDOM + 6, RANDOM + 5, RANDOM + 7]]             # 40: parallel edges
    lists += [[]]                                                                       # 41: degree 0
    lists += [(RANDOM + rng.randint(0, 600, 5000)).tolist()]                            # 42: a hub over 600 targets
    lists += [(RANDOM + rng.permutation(NRAND)[:9000]).tolist()]                        # 43: 9000 distinct targets
    rip, rix = powerlaw_csr(NRAND, mean_deg=8, seed=5)
    ip = np.concatenate([np.cumsum([0] + [len(l) for l in lists]), len(sum(lists, [])) + rip[1:].astype(np.int64)])
    return ip.astype(np.uint32), np.concatenate([np.array(sum(lists, []), np.uint32), rix + np.uint32(RANDOM)])


@pytest.fixture(scope="module")
def graph(ops):
    ip, ix = zoo()
    g = ops.DeviceGraph(dev(ip), dev(ix))
    yield ip, ix, g, ops.budget_map(ip.size - 1, "cuda")
    g.detach_heads()


FANS = list(range(FAN, FAN + 40)) * 2  # 80 seeds on 20 targets, inside one edge tile
MIXED = [MULTI, EMPTY, HUB, MULTI, RANDOM + 3, HUB] + (RANDOM + np.random.RandomState(1).randint(0, NRAND, 700)).tolist()

#        seeds          S          k    grid cap
CASES = [(FANS,         FAN_M - 1, 3,   None),
         (FANS,         FAN_M,     127, None),
         (FANS,         FAN_M + 1, 1,   None),
         (MIXED,        300,       5,   None),   # M above a selection tile; the hub keeps 5 of many eligible entries
         (MIXED,        2500,      127, None),
         (MIXED,        1,         1,   None),
         ([WIDE, HUB],  8000,      100, None),   # more eligible entries than the hub's LDS buffer: the exact route
         ([WIDE, HUB],  3000,      7,   None),   # the hub's LDS search
         ([],           5,         5,   None),
         (MIXED,        300,       5,   1),      # every kernel's later grid-stride rounds
         (MIXED,        2500,      10,  3)]


@pytest.mark.parametrize("mode", [ref.UNIFORM, ref.LADIES], ids=["uniform", "ladies"])
@pytest.mark.parametrize("case", CASES, ids=[f"n{len(c[0])}-S{c[1]}-k{c[2]}-cap{c[3]}" for c in CASES])
def test_leaf_equals_the_reference(ops, graph, case, mode):
    from xgnn_amd import lib
    ip, ix, g, bmap = graph
    inp, S, k, cap = case
    inp = np.array(inp, np.uint32)
    if cap:
        lib().ggms_debug_set_knob(3, cap)  # GGMS_DEBUG_GRID_CAP
    try:
        src, dst, pos, num, stat = ops.sample_khop_budget(g, dev(inp), S, k, 0x1234 + S, mode=mode, map=bmap)
        m = int(num.cpu()[0])
    finally:
        lib().ggms_debug_set_knob(3, -1)
    _, wsrc, wdst, wpos, M, chosen = ref.sample_layer(ip, ix, inp, S, k, mode, 0x1234 + S)
    assert stat.cpu().tolist() == [M, chosen] and m == wsrc.size
    for got, want in ((src, wsrc), (dst, wdst), (pos, wpos)):
        np.testing.assert_array_equal(got.cpu().numpy()[:m].view(np.uint32), want)
    assert not bmap.any().item() and ops.device_status() == 0
    if inp.size == len(FANS):  # the cases are what they claim to be
        assert M == FAN_M and chosen == min(S, FAN_M)


@pytest.mark.parametrize("mode", [ref.UNIFORM, ref.LADIES], ids=["uniform", "ladies"])
def test_batch_equals_the_reference_chain(ops, graph, mode):
    ip, ix, g, _ = graph
    seeds = np.array(MIXED[:60] + [MULTI], np.uint32)
    fanouts, nodes = [4, 6], [500, 200]
    bs = ops.BudgetBatchSampler(g, fanouts, nodes, batch_size=len(seeds), mode=mode)
    for salt in (9, 10):  # the second batch meets the map the first one left
        bs.sample(dev(seeds), salt=salt)
        got, want = bs.result(), ref.sample_batch(ip, ix, seeds, fanouts, nodes, mode, salt)
        np.testing.assert_array_equal(got["input_nodes"].cpu().numpy().view(np.uint32), want["input_nodes"])
        for gl, wl in zip(got["layers"], want["layers"]):
            for name in ("row", "col", "eid"):
                np.testing.assert_array_equal(gl[name].cpu().numpy().view(np.uint32), wl[name], err_msg=name)
            assert (gl["num_src"], gl["num_dst"]) == (wl["num_src"], wl["num_dst"])
        assert want["layers"][1]["num_src"] - len(set(seeds.tolist())) <= nodes[1]
        assert want["layers"][0]["num_src"] - want["layers"][1]["num_src"] <= nodes[0]
        assert not bs.map.any().item()
