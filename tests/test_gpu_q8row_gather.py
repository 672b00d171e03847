"""Q8ROW (row-scaled 8-bit) tables through the converting gathers (ggms_*_convert, include/ggms.h): every output is, bit
for bit, numpy's codes.astype(float32) * scale[:, None] + bias[:, None] narrowed by feat_formats.from_f32 (computed once
per table).  The tables are made so that another row's scale or bias cannot pass, the pad bytes of every row hold 0xFF,
and every output sits between canaries (tests/gather_harness.py; the tables and parameter lists are feat_formats.Q8)."""
import ctypes as C

import numpy as np
import pytest
import torch

from feat_formats import ALL_ONES, E4M3, E5M2, F16, F32, NAMES, OUTS, Q8, Q8ROW, U8, make_table, stride
from gather_harness import (Out, cached_case, full_cache_case, ids, long_row_calls, main_calls, pairs, shared_table,
                            shifted_out_calls, tiered_case, to_device)

OUT_IDS = [NAMES[o] for o in OUTS]

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from xgnn_amd import ops as o
    return o


@pytest.mark.parametrize("dim", Q8.dims)
@pairs(Q8, ids=OUT_IDS)
def test_gather_decodes_with_the_rows_own_scale_and_bias(ops, pair, dim):
    main_calls(ops, Q8, pair, dim)


# the long-row kernel on both sides of its threshold, by chunk count: odd dims move in 1-element chunks (8191: tile
# sweep, 8193: long rows); 8 x 8191 and 8 x 8192 elements in 8-element chunks into the 16-bit types (tile sweep / long
# rows; into f32 both are long rows of 4-element chunks)
@pytest.mark.parametrize("dim", Q8.long_dims)
@pairs(Q8, ids=OUT_IDS)
def test_long_rows_on_both_sides_of_the_threshold(ops, pair, dim):
    long_row_calls(ops, Q8, pair, dim)


@pairs(Q8, ids=OUT_IDS)
def test_misaligned_out_takes_a_narrower_chunk(ops, pair):
    """`out` one element past an aligned base: only 1-element chunks are aligned on the output side."""
    shifted_out_calls(ops, Q8, pair)


@pytest.mark.parametrize("frac,P", [(0.0, 0), (0.3, 0), (0.3, 3), (1.0, 2)])
@pairs(Q8, ids=OUT_IDS)
def test_extract_cached_convert(ops, pair, frac, P):
    """Hits from P shards (0: one array) of stored rows, misses from the pinned host table; the miss count equals the
    plain call's, whose rows are the table's bytes."""
    cached_case(ops, Q8.store(pair[0], "cached"), pair[1], frac, P)


@pairs(Q8, ids=OUT_IDS)
def test_extract_cached_convert_full_cache_in_node_order(ops, pair):
    """table == NULL: slot = node id, no miss tier."""
    full_cache_case(ops, Q8.store(pair[0], "full"), pair[1], 3)


@pytest.mark.parametrize("P", [1, 2, 3])
@pairs(Q8, ids=OUT_IDS)
def test_extract_tiered_convert(ops, pair, P):
    """Replica + P shards + the host slot, all stored rows; the four tier counters equal the plain call's."""
    tiered_case(ops, Q8.store(pair[0], "tiered"), pair[1], P)


def test_the_table_carries_what_it_promises():
    """Every code in column 0, scales 2^20 apart and biases of either sign in neighbouring rows, rows of scale 0, and
    the rounding edges as exact f32 values."""
    t = make_table(512, 20, seed=1020)
    assert sorted(t.codes[:256, 0].tolist()) == list(range(256))
    s = np.abs(t.scale.astype(np.float64))
    both = (s[:-1] > 0) & (s[1:] > 0)
    ratio = np.maximum(s[:-1], s[1:])[both] / np.minimum(s[:-1], s[1:])[both]
    assert ratio.max() >= 2.0 ** 19 and (t.scale == 0).sum() >= 512 // 7 and (t.scale < 0).any()
    assert (np.sign(t.bias[:-1]) * np.sign(t.bias[1:]) < 0).sum() > 400
    assert (t.stored[:, 20:24] == 0xFF).all()
    f32 = t.bits(F32).view(np.float32)
    assert f32[256, 0] == 65520.0 and f32[257, 0] == 1 + 2.0 ** -11 and f32[257, 1] == 1 + 3 * 2.0 ** -11
    assert f32[258, 0] == 1 + 2.0 ** -8 and f32[258, 1] == 1 + 3 * 2.0 ** -8
    assert np.isinf(t.bits(F16).view(np.float16)[256, 0])  # 65520 is the f16 overflow tie: to even, which is inf


@pytest.mark.parametrize("out_dt", OUTS, ids=OUT_IDS)
def test_a_source_base_off_the_8_byte_boundary_is_refused(ops, out_dt):
    """The trailer is read by one 8-byte load: a base 4 bytes off is GGMS_ERR_INVALID with a message, nothing launched."""
    from xgnn_amd import lib
    t = make_table(64, 20, seed=3)
    src = to_device(t.stored, Q8ROW, offset=4)
    assert src.data_ptr() % 8 == 4
    out = Out(64, 20, out_dt)
    rc = lib().ggms_gather_scatter_convert(out.t.data_ptr(), src.data_ptr(), ids(np.arange(64)).data_ptr(), None, 64, None, 20,
                                           Q8ROW, out_dt, ALL_ONES, torch.cuda.current_stream().cuda_stream)
    assert rc == -1 and b"8-byte aligned" in lib().ggms_last_error()
    torch.cuda.synchronize()
    assert out.untouched()
    # the same through a shard pointer and through the host slot of the cached gather
    good = to_device(t.stored, Q8ROW)
    for parts, host in [([src], good), ([good], src)]:
        rc = lib().ggms_extract_cached_convert(out.t.data_ptr(), ids(np.arange(64)).data_ptr(), 64, None,
                                               ids(np.arange(64)).data_ptr(), ops.part_pointer_table(parts).ptr(), 0,
                                               host.data_ptr(), 20, Q8ROW, out_dt, None,
                                               torch.cuda.current_stream().cuda_stream)
        assert rc == -1 and b"8-byte aligned" in lib().ggms_last_error()
    torch.cuda.synchronize()
    assert out.untouched()


def test_the_plain_byte_gather_moves_the_packed_rows(ops):
    """A Q8ROW table that has to move as bytes is a GGMS_U8 table of dim = stride: trailer and pad bytes included."""
    for dim, n in [(100, 1000), (128, 257), (3, 65)]:
        t, t_src = shared_table(Q8, Q8ROW, 512, dim)
        index = np.random.RandomState(1).randint(0, 512, n).astype(np.uint32)
        out = torch.zeros((n, stride(dim)), dtype=torch.uint8, device="cuda")
        ops.gather_scatter(out, t_src, ids(index), None)
        assert out.cpu().numpy().tobytes() == t.stored[index].tobytes()


def test_illegal_pairs_launch_nothing(ops):
    """Q8ROW is a source of the converting gathers into F32 / F16 / BF16 and nothing else: as an output, into U8 or FP8,
    into itself, or through a plain entry point it is GGMS_ERR_INVALID with a message."""
    from xgnn_amd import lib
    h = lib()
    out = torch.full((8, 16), 0x5a, dtype=torch.uint8, device="cuda")
    src = torch.zeros((8, 16), dtype=torch.float32, device="cuda")
    index = ids(np.arange(8))
    s = torch.cuda.current_stream().cuda_stream
    for src_dt, dst_dt in [(F32, Q8ROW), (F16, Q8ROW), (U8, Q8ROW), (E4M3, Q8ROW), (Q8ROW, U8), (Q8ROW, E4M3), (Q8ROW, E5M2),
                           (Q8ROW, Q8ROW), (Q8ROW, 1), (Q8ROW, 6)]:
        assert h.ggms_gather_scatter_convert(out.data_ptr(), src.data_ptr(), index.data_ptr(), None, 8, None, 4, src_dt,
                                             dst_dt, ALL_ONES, s) == -1, (src_dt, dst_dt)
        assert b"no conversion" in h.ggms_last_error(), (src_dt, dst_dt, h.ggms_last_error())
    ptab = ops.part_pointer_table([src])
    assert h.ggms_extract_cached_convert(out.data_ptr(), index.data_ptr(), 8, None, None, ptab.ptr(), 0, None, 4, F32,
                                         Q8ROW, None, s) == -1 and b"no conversion" in h.ggms_last_error()
    t = ops._feature_tiers(None, None, ptab, 1, 0, None)
    assert h.ggms_extract_tiered_convert(out.data_ptr(), index.data_ptr(), 8, None, C.byref(t), 4, Q8ROW, U8, None,
                                         s) == -1 and b"no conversion" in h.ggms_last_error()
    # the plain entry points: no element size, the existing invalid-argument refusal
    assert h.ggms_extract(out.data_ptr(), src.data_ptr(), index.data_ptr(), 8, 4, Q8ROW, s) == -1
    assert len(h.ggms_last_error()) > 0
    assert h.ggms_gather_scatter(out.data_ptr(), src.data_ptr(), index.data_ptr(), None, 8, None, 4, Q8ROW, s) == -1
    assert len(h.ggms_last_error()) > 0
    assert h.ggms_gather_scatter_masked(out.data_ptr(), src.data_ptr(), index.data_ptr(), None, 8, None, 4, Q8ROW, 7,
                                        s) == -1 and b"no conversion" in h.ggms_last_error()
    assert h.ggms_extract_cached(out.data_ptr(), index.data_ptr(), 8, None, None, ptab.ptr(), 0, None, 4, Q8ROW, None,
                                 s) == -1
    assert h.ggms_extract_tiered(out.data_ptr(), index.data_ptr(), 8, None, C.byref(t), 4, Q8ROW, None, s) == -1
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 0x5a).all()
