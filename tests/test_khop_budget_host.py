"""khop_budget without a GPU: the type code, the header's refusals (reached through ctypes with fake pointers: every one
returns before a device call), and the numpy statement's own identities and draw frequencies."""
import ctypes as C

import numpy as np
import pytest

import khop_budget_ref as ref
from graphgen import powerlaw_csr

IP, IX = powerlaw_csr(300, mean_deg=6, seed=2)
SEEDS = np.arange(0, 300, 7, dtype=np.uint32)


def test_type_code():
    from xgnn_amd import common, ops
    assert common.sample_types["khop_budget"] == common.kKHopBudget == ops.KHOP_BUDGET == 15
    assert (ops.BUDGET_UNIFORM, ops.BUDGET_LADIES) == (ref.UNIFORM, ref.LADIES) == (0, 1)


#                 num_part  n        S  k    mode  map   in the message
@pytest.mark.parametrize("part,n,S,k,mode,bmap,word", [
    (2, 4, 5, 5, 1, 64, "unsharded"), (0, 4, 0, 5, 1, 64, "budget"), (0, 4, 5, 0, 1, 64, "fanout"),
    (0, 4, 5, 128, 1, 64, "fanout"), (0, 4, 5, 5, 2, 64, "mode"), (0, 1 << 22, 5, 5, 0, 64, "2^22"),
    (0, 4, 5, 5, 0, None, "map")])
def test_refusals(part, n, S, k, mode, bmap, word):
    from xgnn_amd import _lib, lib
    g = _lib.Graph()
    g.indptr, g.indices, g.num_node, g.num_part = 64, 64, 10, part
    fake = C.c_void_p(64)
    rc = lib().ggms_sample_khop_budget(C.byref(g), fake, n, S, k, mode, 0, C.c_void_p(bmap), fake, fake, fake, fake, None,
                                       fake, 1 << 40, None)
    assert rc != 0 and "ggms_sample_khop_budget" in lib().ggms_last_error().decode()
    assert word in lib().ggms_last_error().decode()


def test_refusals_of_sizes_and_the_plain_batch():
    from xgnn_amd import _lib, lib
    assert lib().ggms_sample_khop_budget_workspace_bytes(10, 5, (1 << 32) - 1) == 0
    assert lib().ggms_sample_khop_budget_workspace_bytes(10, 5, (1 << 32) - 2) > 8 * ((1 << 32) - 2)
    f = (C.c_size_t * 1)(5)
    fake, ptrs = C.c_void_p(64), (C.c_void_p * 1)(64)
    rc = lib().ggms_sample_batch(15, C.byref(_lib.Graph()), fake, 4, f, 1, C.byref(_lib.HashTable()), None, 0, ptrs, ptrs,
                                 fake, None, fake, 1 << 40, None)
    assert rc != 0 and "ggms_sample_batch_budget" in lib().ggms_last_error().decode()


@pytest.mark.parametrize("mode", [ref.UNIFORM, ref.LADIES])
def test_without_a_binding_budget_the_layer_is_the_frontier(mode):
    where, src, dst, pos, M, chosen = ref.sample_layer(IP, IX, SEEDS, 10 ** 6, 10 ** 6, mode, 5)
    want = np.concatenate([np.arange(IP[s], IP[s + 1]) for s in SEEDS])
    assert chosen == M == np.unique(IX[want]).size
    np.testing.assert_array_equal(pos, want)
    np.testing.assert_array_equal(dst, IX[want])
    np.testing.assert_array_equal(src, np.repeat(SEEDS, (IP[SEEDS + 1] - IP[SEEDS]).astype(np.int64)))


@pytest.mark.parametrize("S,k", [(1, 3), (17, 2), (40, 127)])
def test_a_binding_budget_gives_exactly_S_destinations(S, k):
    where, _, dst, _, M, chosen = ref.sample_layer(IP, IX, SEEDS, S, k, ref.LADIES, 11)
    assert M > S == chosen
    # with k at least the largest degree every chosen node keeps an edge; a smaller cap can drop all edges of one
    assert np.unique(dst).size == S if k >= 127 else np.unique(dst).size <= S
    assert np.bincount(where).max() <= k


@pytest.mark.parametrize("mode", [ref.UNIFORM, ref.LADIES])
def test_budget_one_draws_in_proportion_to_the_weight(mode):
    """S = 1 over R distinct salts: candidate t is the one chosen with probability p = W_t / sum W, so its count is
    binomial(R, p) and stays within five standard deviations, 5 sqrt(R p (1 - p))."""
    seeds, R = SEEDS[:6], 3000
    t, w, _ = ref.candidates(IP, IX, seeds, mode, 0)
    p = w.astype(np.float64) / w.astype(np.float64).sum()
    hits = np.zeros(t.size, np.int64)
    for salt in range(R):
        _, _, dst, _, _, _ = ref.sample_layer(IP, IX, seeds, 1, 127, mode, salt)
        hits[np.searchsorted(t, dst[0])] += 1
    assert (np.abs(hits - R * p) <= 5 * np.sqrt(R * p * (1 - p))).all()
