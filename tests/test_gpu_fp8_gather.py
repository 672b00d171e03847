"""FP8 (E4M3 / E5M2) tables through the converting gathers (ggms_*_convert, include/ggms.h): every output is the CPU cast
of the closed-form truth table (feat_formats.truth, checked against torch in test_fp8_decode_table.py) -- bitwise, because
every finite code is exact in f32, f16 and bf16; NaN codes must give NaN; -0.0 stays -0.0 (tests/gather_harness.py; the
tables and parameter lists are feat_formats.FP8)."""
import ctypes as C

import numpy as np
import pytest
import torch

from feat_formats import ALL_ONES, E4M3, E5M2, F16, F32, FP8, NAMES, TORCH, U8
from gather_harness import (cached_case, full_cache_case, ids, long_row_calls, main_calls, pairs, shared_table,
                            shifted_out_calls, table_offset_calls, tiered_case)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from xgnn_amd import ops as o
    return o


@pytest.mark.parametrize("dim", FP8.dims)
@pairs(FP8)
def test_gather_decodes_every_code(ops, pair, dim):
    main_calls(ops, FP8, pair, dim)


# the long-row kernel on both sides of its threshold, by chunk count: odd dims move in 1-element chunks (8191: tile
# sweep, 8193: long rows); 8 x 8191 and 8 x 8192 elements in 8-element chunks into the 16-bit types (tile sweep / long
# rows; into f32 both are long rows of 4-element chunks)
@pytest.mark.parametrize("dim", FP8.long_dims)
@pairs(FP8)
def test_long_rows_on_both_sides_of_the_threshold(ops, pair, dim):
    long_row_calls(ops, FP8, pair, dim)


@pytest.mark.parametrize("offset", FP8.offsets)
@pairs(FP8)
def test_misaligned_table_takes_a_narrower_chunk(ops, pair, offset):
    """The table's base 1, 2 and 4 bytes past a 16-byte boundary: chunks of 1, 2 and 4 elements are what stays aligned."""
    table_offset_calls(ops, FP8, pair, offset)


@pairs(FP8)
def test_misaligned_out_takes_a_narrower_chunk(ops, pair):
    """`out` one element past an aligned base: only 1-element chunks are aligned on the output side."""
    shifted_out_calls(ops, FP8, pair)


@pytest.mark.parametrize("frac,P", [(0.0, 0), (0.3, 0), (0.3, 3), (1.0, 2)])
@pairs(FP8)
def test_extract_cached_convert(ops, pair, frac, P):
    """Hits from P shards (0: one array) of stored rows, misses from the pinned host table; the miss count equals the
    plain call's, whose rows are the table's bytes."""
    cached_case(ops, FP8.store(pair[0], "cached"), pair[1], frac, P)


@pairs(FP8)
def test_extract_cached_convert_full_cache_in_node_order(ops, pair):
    """table == NULL: slot = node id, no miss tier."""
    full_cache_case(ops, FP8.store(pair[0], "full"), pair[1], 3)


@pytest.mark.parametrize("P", [1, 2, 3])
@pairs(FP8)
def test_extract_tiered_convert(ops, pair, P):
    """Replica + P shards + the host slot, all stored rows; the four tier counters equal the plain call's."""
    tiered_case(ops, FP8.store(pair[0], "tiered"), pair[1], P)


@pytest.mark.parametrize("fmt", FP8.formats, ids=[NAMES[f] for f in FP8.formats])
def test_same_dtype_is_the_plain_byte_gather(ops, fmt):
    """src_dtype == out_dtype == F8*: the rows' bytes, as ggms_gather_scatter_masked moves a U8 table."""
    from xgnn_amd import lib
    for dim, n in [(100, 1000), (128, 257), (3, 65)]:
        t, t_src = shared_table(FP8, fmt, 512, dim)
        index = np.random.RandomState(1).randint(0, 1 << 31, n).astype(np.uint32)
        t_index = ids(index)
        out = torch.zeros((n, dim), dtype=TORCH[fmt], device="cuda")
        ops.gather_scatter_convert(out, t_src, t_index, None, src_row_mask=511)
        ref = torch.zeros((n, dim), dtype=torch.uint8, device="cuda")
        rc = lib().ggms_gather_scatter_masked(ref.data_ptr(), t_src.data_ptr(), t_index.data_ptr(), None, n, None, dim, U8,
                                              511, torch.cuda.current_stream().cuda_stream)
        assert rc == 0
        want = t.stored[index & 511].tobytes()
        assert out.view(torch.uint8).cpu().numpy().tobytes() == ref.cpu().numpy().tobytes() == want
        plain = torch.zeros((n, dim), dtype=TORCH[fmt], device="cuda")
        ops.gather_scatter(plain, t_src, ids(index & 511), None)
        assert plain.view(torch.uint8).cpu().numpy().tobytes() == want


def test_illegal_pairs_launch_nothing(ops):
    """FP8 is a source only: as the output of another source, or of the other FP8 format, it is GGMS_ERR_INVALID with a
    message; codes 8 .. 15 stay unknown."""
    from xgnn_amd import lib
    h = lib()
    out = torch.full((8, 4), 0x5a, dtype=torch.uint8, device="cuda")
    src = torch.zeros((8, 4), dtype=torch.float32, device="cuda")
    index = ids(np.arange(8))
    s = torch.cuda.current_stream().cuda_stream
    for src_dt, dst_dt, word in [(F32, E4M3, b"conversion"), (F32, E5M2, b"conversion"), (F16, E4M3, b"conversion"),
                                 (E4M3, E5M2, b"conversion"), (E5M2, E4M3, b"conversion"), (E4M3, U8, b"conversion"),
                                 (E4M3, 8, b"invalid argument"), (12, F32, b"invalid argument")]:
        assert h.ggms_gather_scatter_convert(out.data_ptr(), src.data_ptr(), index.data_ptr(), None, 8, None, 4, src_dt,
                                             dst_dt, ALL_ONES, s) == -1, (src_dt, dst_dt)
        assert word in h.ggms_last_error() and len(h.ggms_last_error()) > 0, (src_dt, dst_dt, h.ggms_last_error())
    ptab = ops.part_pointer_table([src])
    assert h.ggms_extract_cached_convert(out.data_ptr(), index.data_ptr(), 8, None, None, ptab.ptr(), 0, None, 4, F32,
                                         E4M3, None, s) == -1
    t = ops._feature_tiers(None, None, ptab, 1, 0, None)
    assert h.ggms_extract_tiered_convert(out.data_ptr(), index.data_ptr(), 8, None, C.byref(t), 4, F16, E5M2, None,
                                         s) == -1
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 0x5a).all()
