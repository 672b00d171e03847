"""The converting gathers (ggms_*_convert, include/ggms.h) between F16, BF16 and F32 against numpy / torch conversions on
the CPU, bit for bit and between canaries (tests/gather_harness.py; the tables and parameter lists are feat_formats.FLOAT)."""
import ctypes as C

import numpy as np
import pytest
import torch

from feat_formats import ALL_ONES, BF16, F16, F32, FLOAT, U8, tensor_bits
from gather_harness import (Out, cached_case, full_cache_case, ids, long_row_calls, main_calls, pairs, shared_table,
                            shifted_out_calls, tiered_case)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from xgnn_amd import ops as o
    return o


@pytest.mark.parametrize("dim", FLOAT.dims)
@pairs(FLOAT)
def test_gather_scatter_convert(ops, pair, dim):
    """Every pair x every row shape, over n x {identity, dst_index} x {host count, device count} x {no mask, 2^4 - 1}."""
    main_calls(ops, FLOAT, pair, dim)


@pairs(FLOAT, (F16, F32), (F32, BF16))
def test_long_rows(ops, pair):
    """dim 65536 = 16384 chunks of 4 elements: the one-workgroup-per-row kernel."""
    long_row_calls(ops, FLOAT, pair, 65536)


@pairs(FLOAT)
def test_misaligned_out_takes_a_narrower_chunk_and_gives_the_same_bits(ops, pair):
    """`out` two elements past an aligned base: only 2-element chunks are still aligned on the output side."""
    shifted_out_calls(ops, FLOAT, pair)


@pytest.mark.parametrize("P", [0, 1, 3])
@pairs(FLOAT, (F16, F32), (F32, BF16), (BF16, F16))
def test_extract_cached_convert(ops, pair, P):
    """Hits from P shards (0: one array), misses from a pinned host table; the miss count equals the plain call's."""
    cached_case(ops, FLOAT.store(pair[0], "cached"), pair[1], 0.4, P)


@pytest.mark.parametrize("P", [0, 3])
def test_extract_cached_convert_full_cache_in_node_order(ops, P):
    """table == NULL: slot = node id, no miss tier."""
    full_cache_case(ops, FLOAT.store(F16, "full"), F32, P)


@pytest.mark.parametrize("P", [1, 2, 3])
@pairs(FLOAT, (F16, F32), (F32, F16))
def test_extract_tiered_convert(ops, pair, P):
    """Replica + P shards + host rows behind a host_row_mask; the four tier counters equal the plain call's."""
    tiered_case(ops, FLOAT.store(pair[0], "tiered"), pair[1], P, FLOAT.host_mask)


def test_invalid_arguments_launch_nothing(ops):
    from xgnn_amd import lib
    h = lib()
    out = Out(8, 4, F32)
    src = torch.zeros((8, 4), dtype=torch.float32, device="cuda")
    index = ids(np.arange(8))
    s = torch.cuda.current_stream().cuda_stream
    I64 = 6

    def call(o, dim, src_dt, dst_dt):
        return h.ggms_gather_scatter_convert(o, src.data_ptr(), index.data_ptr(), None, 8, None, dim, src_dt, dst_dt,
                                             ALL_ONES, s)
    for args, word in [((out.t.data_ptr(), 4, F32, U8), b"conversion"), ((out.t.data_ptr(), 4, I64, F32), b"conversion"),
                       ((out.t.data_ptr(), 0, F16, F32), b"invalid argument"), ((None, 4, F16, F32), b"invalid argument"),
                       ((out.t.data_ptr(), 4, F16, 8), b"invalid argument")]:
        assert call(*args) == -1, args
        assert word in h.ggms_last_error(), (args, h.ggms_last_error())
    ptab = ops.part_pointer_table([src])
    assert h.ggms_extract_cached_convert(out.t.data_ptr(), index.data_ptr(), 8, None, None, ptab.ptr(), 0, None, 4, F32,
                                         U8, None, s) == -1
    assert h.ggms_extract_cached_convert(out.t.data_ptr(), index.data_ptr(), 8, None, None, ptab.ptr(), 9, None, 4, F32,
                                         F16, None, s) == -1  # too many parts
    t = ops._feature_tiers(None, None, ptab, 1, 0, None)
    assert h.ggms_extract_tiered_convert(out.t.data_ptr(), index.data_ptr(), 8, None, C.byref(t), 4, I64, F32, None,
                                         s) == -1
    assert h.ggms_extract_tiered_convert(out.t.data_ptr(), index.data_ptr(), 8, None, None, 4, F16, F32, None, s) == -1
    torch.cuda.synchronize()
    assert out.untouched()


def test_same_dtype_is_the_plain_gather(ops):
    """(F32, F32): byte-identical to ggms_gather_scatter_masked; the same holds for a dtype that never converts."""
    from xgnn_amd import lib
    n, dim = 1000, 100
    t, t_src = shared_table(FLOAT, F32, 2048, dim)
    index = np.random.RandomState(1).randint(0, 1 << 31, n).astype(np.uint32)
    t_index = ids(index)
    out, ref = Out(n, dim, F32), Out(n, dim, F32)
    ops.gather_scatter_convert(out.t, t_src, t_index, None, src_row_mask=1023)
    rc = lib().ggms_gather_scatter_masked(ref.t.data_ptr(), t_src.data_ptr(), t_index.data_ptr(), None, n, None, dim, F32,
                                          1023, torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    assert tensor_bits(out.flat, F32).tobytes() == tensor_bits(ref.flat, F32).tobytes()
    assert tensor_bits(out.t, F32).tobytes() == t.stored[index & 1023].tobytes()
    bytes_src = torch.arange(64 * 10, dtype=torch.uint8, device="cuda").view(64, 10)
    got = torch.zeros((5, 10), dtype=torch.uint8, device="cuda")
    ops.gather_scatter_convert(got, bytes_src, ids([3, 1, 63, 0, 3]), None)
    assert torch.equal(got, bytes_src[[3, 1, 63, 0, 3]])
