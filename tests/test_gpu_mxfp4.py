"""GGMS_MXFP4 on the GPU: the converting gathers decode bit for bit what mxfp4_ref.decode states (every (code, scale
byte) pair is in every call's index head; outputs sit between canaries, tests/gather_harness.py), ggms_quantize_rows
writes the bytes of datagen.pack_mxfp4(*quantize_mxfp4(v)), and an engine run with feat_store_dtype = MXFP4 delivers the
twin's decode of the twin's encode."""
import numpy as np
import pytest
import torch

from engine_harness import batch_keys, drive
from feat_formats import BF16, F32, NAMES, OUTS, from_f32, write_finite_dataset
from gather_harness import Out, cached_case, full_cache_case, gather_case, ids, long_row_calls, main_calls, pairs, to_device
from mxfp4_ref import MX, MXFP4, decode
from test_mxfp4_host import edge_rows
from xgnn_amd import datagen

pytestmark = pytest.mark.gpu
OUT_IDS = [NAMES[o] for o in OUTS]
GRID_CAP = 3  # GGMS_DEBUG_GRID_CAP (include/ggms.h)
N_ROWS = 13 * 256 + 65  # at least four rounds per workgroup under a cap of 3, the last one partial


@pytest.fixture(scope="module")
def ops():
    from xgnn_amd import ops as o
    return o


@pytest.fixture()
def cap3(ops):
    from xgnn_amd import lib
    lib().ggms_debug_set_knob(GRID_CAP, 3)
    yield
    lib().ggms_debug_set_knob(GRID_CAP, -1)


@pytest.mark.parametrize("dim", MX.dims)
@pairs(MX, ids=OUT_IDS)
def test_gather_decodes_every_code_under_every_scale(ops, pair, dim):
    main_calls(ops, MX, pair, dim)


@pytest.mark.parametrize("dim", MX.long_dims)
@pairs(MX, ids=OUT_IDS)
def test_long_rows(ops, pair, dim):
    long_row_calls(ops, MX, pair, dim)


@pairs(MX, ids=OUT_IDS)
def test_cached_full_cache_and_tiered(ops, pair):
    cached_case(ops, MX.store(MXFP4, "cached"), pair[1], 0.3, 3)
    full_cache_case(ops, MX.store(MXFP4, "full"), pair[1], 2)
    # tiered: 40 replica rows, 2 shards of the next 220 ranked rows, the rest from the pinned host table
    t, n, R, P = MX.store(MXFP4, "tiered"), 300, 40, 2
    rank = np.random.RandomState(6).permutation(512)
    tab = np.full(512, 0xFFFFFFFF, np.uint32)
    tab[rank[:260]] = np.arange(260, dtype=np.uint32)
    replica = to_device(np.ascontiguousarray(t.stored[rank[:R]]), MXFP4)
    ptab = ops.part_pointer_table([to_device(np.ascontiguousarray(t.stored[rank[R + p:260:P]]), MXFP4) for p in range(P)])
    host = torch.from_numpy(np.array(t.stored)).pin_memory()
    nodes = np.random.RandomState(4).randint(0, 512, n).astype(np.uint32)
    out, counters = Out(n, t.dim, pair[1]), torch.zeros(4, dtype=torch.int64, device="cuda")
    ops.extract_tiered_convert(out.t, MXFP4, ids(nodes), ids(tab), replica, ptab, P, 1, host, tier_rows=counters)
    out.check(np.arange(n), t, nodes, "tiered")
    slots = tab[nodes].astype(np.int64)
    hit = slots != 0xFFFFFFFF
    assert counters.cpu().tolist() == [int((~hit).sum()), int((hit & (slots >= R) & ((slots - R) % P != 1)).sum()),
                                       int((hit & (slots >= R) & ((slots - R) % P == 1)).sum()), int((slots < R).sum())]


@pairs(MX, (MXFP4, BF16), (MXFP4, F32), ids=["BF16", "F32"])
def test_gather_later_grid_rounds(ops, cap3, pair):
    gather_case(ops, MX, *pair, 128, N_ROWS, scatter=True, dev_count=True)


def quantiser_rows(rows, dim, src):
    """edge_rows (ties, +-0, saturation, a zero block, the largest f32; F16: scaled into its range) in front of random rows."""
    rs = np.random.RandomState(rows + dim)
    v = (rs.standard_normal((rows, dim)) * 10.0 ** rs.uniform(-3, 3, (rows, 1))).astype(np.float32)
    edge = np.resize(edge_rows(64), (17, dim)) if dim >= 64 else edge_rows(64)[:, :dim]
    if src == np.float16:
        edge = np.where(np.abs(edge) > 6e4, 6e4, edge)
    v[:min(rows, 17)] = edge[:min(rows, 17)]
    return v.astype(src)


@pytest.mark.parametrize("src", [np.float32, np.float16], ids=["F32", "F16"])
@pytest.mark.parametrize("dim", [32, 100, 768])
def test_quantiser_bytes_equal_the_numpy_rule(ops, dim, src):
    for rows in (1, 257):
        v = quantiser_rows(rows, dim, src)
        got = ops.quantize_rows(torch.from_numpy(v).cuda(), ops.MXFP4).cpu().numpy()
        want = datagen.pack_mxfp4(*datagen.quantize_mxfp4(v))
        bad = np.flatnonzero((got != want).any(axis=1))
        assert got.shape == want.shape and bad.size == 0, f"rows {bad[:8].tolist()} differ; row {bad[0]}: got " \
                                                          f"{got[bad[0]].tolist()}, want {want[bad[0]].tolist()}"


def test_quantiser_bad_rows_and_later_grid_rounds(ops, cap3):
    v = quantiser_rows(N_ROWS, 100, np.float32)
    v[5, 99], v[3000, 0] = np.nan, -np.inf
    t = torch.from_numpy(v).cuda()
    with pytest.raises(ValueError, match=r"row 1005 holds NaN or inf"):
        ops.quantize_rows(t, ops.MXFP4, first_row=1000)
    got = ops.quantize_rows(t, ops.MXFP4, check=False).cpu().numpy()
    assert not got[5].any() and not got[3000].any()
    good = np.setdiff1d(np.arange(N_ROWS), [5, 3000])
    np.testing.assert_array_equal(got[good], datagen.pack_mxfp4(*datagen.quantize_mxfp4(v[good])))


def test_engine_store_dtype_arch1(tmp_path):
    d = write_finite_dataset(tmp_path / "f32x128", F32, 128)
    run, = drive(d, str(tmp_path / "out"), "arch1", dict(feat_store_dtype="MXFP4", feat_out_dtype="bf16"))
    want = from_f32(decode(*datagen.quantize_mxfp4(d["values"])), BF16)
    assert len(batch_keys(run)) >= 4
    for key in batch_keys(run):
        nodes = run[f"{key}:input_nodes"].view(np.uint32)
        assert str(run[f"{key}:feat_dtype"]) == "torch.bfloat16"
        np.testing.assert_array_equal(run[f"{key}:feat_bits"].view(np.uint16), want[nodes], err_msg=f"batch {key}")
