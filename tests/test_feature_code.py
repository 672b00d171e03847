"""graphgen's feature code (exact_features / feature_rows and their torch twins): what the gather tests rely on.

Every byte-copy gather test fills its table with this code and compares bytes.  The code must therefore (a) be the same
in numpy and torch at every element number, (b) survive every dtype the tests store it in, and (c) tell rows apart:
within a table, and above all between a row and the row a TRUNCATED byte offset lands on.  The form before this one,
feat[i, j] = (i * dim + j) & 0xFFFF, failed (c) at exactly the offsets the full-size tests exist for; the last test here
shows it."""
import numpy as np
import pytest

from graphgen import code_bits, exact_features, feature_code, feature_rows, torch_feature_code, torch_feature_rows

torch = pytest.importorskip("torch")

EXTRACT_DTYPES = [np.float32, np.float64, np.int16, np.uint8, np.int32, np.int64]  # test_gpu_parity.py:test_extract
TORCH_OF = {np.float32: torch.float32, np.float64: torch.float64, np.float16: torch.float16, np.int16: torch.int16,
            np.uint8: torch.uint8, np.int32: torch.int32, np.int64: torch.int64}

PAPERS = (111_059_956, 128)  # test_gpu_full_size.py: papers100M, f32
FRIENDSTER = (65_608_366, 256)


def old_rows(ids, dim):
    """The closed form this code replaced."""
    return ((np.asarray(ids, np.int64)[:, None] * dim + np.arange(dim)) & 0xFFFF).astype(np.float32)


def test_code_widths():
    assert [code_bits(d) for d in (np.float32, np.float64, np.int32, np.int64, np.float16, np.int16, np.uint8)] == \
        [24, 24, 24, 24, 11, 15, 8]
    assert code_bits(torch.float32) == 24 and code_bits(torch.float16) == 11 and code_bits(torch.uint8) == 8


def test_numpy_and_torch_twins_are_bit_equal():
    """Element numbers all over the 64-bit range: around 2^31, 2^32, 2^40, 2^63 (where the int64 twin is negative)."""
    rs = np.random.RandomState(0)
    near = np.concatenate([np.arange(-70, 70, dtype=np.int64) + (1 << k) for k in (0, 16, 24, 31, 32, 33, 40, 48, 62)])
    near = near[near >= 0].astype(np.uint64)
    wide = rs.randint(0, 1 << 62, 20_000).astype(np.uint64) * np.uint64(4) + rs.randint(0, 4, 20_000).astype(np.uint64)
    elem = np.concatenate([near, wide, np.array([(1 << 63) - 1, 1 << 63, (1 << 64) - 1], np.uint64)])
    assert (elem > np.uint64(1 << 32)).sum() > 10_000 and (elem > np.uint64(1 << 40)).sum() > 10_000
    t_elem = torch.from_numpy(elem.view(np.int64))
    for bits in (8, 11, 15, 24):
        want = feature_code(elem, bits)
        assert want.min() >= 0 and want.max() < 1 << bits
        assert np.array_equal(torch_feature_code(t_elem, bits).numpy(), want)
    # the same through the row generators, node ids whose element numbers pass 2^32 and 2^40
    ids = np.array([0, 1, 33_554_431, 33_554_432, 111_059_955, (1 << 32) - 1, 1 << 33], np.uint64)
    for dt, tdt in TORCH_OF.items():
        for dim in (1, 7, 128, 1024):
            got = torch_feature_rows(torch.from_numpy(ids.view(np.int64)), dim, tdt)
            assert got.numpy().tobytes() == feature_rows(ids, dim, dt).tobytes(), (dt, dim)
    assert exact_features(100, 9, np.float16).tobytes() == feature_rows(np.arange(100), 9, np.float16).tobytes()


def test_the_mixer_sees_all_64_bits():
    """An input cut to 32 bits before mixing would bring a period of 2^32 elements back."""
    e = np.arange(0, 4096, dtype=np.uint64)
    for k in range(32, 64):
        assert (feature_code(e, 24) != feature_code(e + np.uint64(1 << k), 24)).mean() > 0.99, k


@pytest.mark.parametrize("dtype", EXTRACT_DTYPES + [np.float16])
def test_values_round_trip_through_the_dtype(dtype):
    ids = np.concatenate([np.arange(300), np.arange(300) + (1 << 25)])
    for dim in (1, 7, 100):
        rows = feature_rows(ids, dim, dtype)
        elem = ids.astype(np.uint64)[:, None] * np.uint64(dim) + np.arange(dim, dtype=np.uint64)
        code = feature_code(elem, code_bits(dtype))
        assert rows.dtype == np.dtype(dtype) and np.array_equal(rows.astype(np.int64), code)
        assert np.array_equal(rows.astype(np.float64), code.astype(np.float64)) and np.isfinite(rows.astype(np.float64)).all()


def test_no_float_holds_an_output_sentinel():
    """Integers below 2^24 as f32 (2^11 as f16) never have the bit patterns the tests fill their outputs with."""
    assert np.float32(np.uint32(0x5A5A5A5A).view(np.float32)) > 2.0 ** 24  # 1.5e16
    assert float(np.uint16(0x5A5A).view(np.float16)) == 203.25  # no integer
    f = exact_features(50_000, 32, np.float32).view(np.uint32)
    assert not (f == 0x5A5A5A5A).any()
    h = exact_features(50_000, 32, np.float16).view(np.uint16)
    assert not (h == 0x5A5A).any()


# every (rows, dim, dtype) a test of the tree builds with this code (the large tables of test_gpu_large_offsets.py are
# checked at their boundaries below: 10^7 rows and more are not sorted here)
SHAPES = [(5000, dim, dt) for dt, dim in [(np.float32, 100), (np.float32, 128), (np.float32, 256), (np.float32, 1),
                                          (np.float64, 5), (np.int16, 7), (np.uint8, 3), (np.uint8, 33), (np.int32, 32),
                                          (np.int64, 1), (np.float32, 602)]]                  # test_extract
SHAPES += [(1 << b, 100, np.float32) for b in (1, 7, 13)]                                     # test_mock_extract
SHAPES += [(200_064, 32, np.float32), (50_064, 100, np.float32), (50_064, 1, np.float32),    # test_gpu_device_counts
           (50_064, 4, np.float32),                                                           # test_gpu_owner_split
           (50_000, 32, np.float32), (20_000, 100, np.float32), (20_000, 128, np.float32),    # test_gpu_parity
           (3000, 20, np.float32), (3000, 20, np.float16), (3000, 20, np.uint8),              # test_engine.make_dataset
           (3000, 7, np.float32), (3000, 7, np.float16), (3000, 7, np.uint8), (4000, 16, np.float32),
           (3000, 9, np.float16), (3000, 9, np.float64), (3000, 9, np.float32),               # test_gpu_arch3
           (2_449_029, 100, np.float32)]                                                      # test_extract_large_properties
# fewer than 40 bits of code in a row: with thousands of rows some MUST or may coincide, nothing is claimed for them
TOO_NARROW = {(5000, 1, np.float32), (5000, 1, np.int64), (5000, 3, np.uint8), (50_064, 1, np.float32)}


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}-{np.dtype(s[2]).name}")
def test_rows_of_every_table_in_the_tree_are_pairwise_distinct(shape):
    N, dim, dt = shape
    if dim * code_bits(dt) < 40:
        assert shape in TOO_NARROW
        return
    assert shape not in TOO_NARROW
    # the first columns that hold 40 bits of code, packed into one word per row: rows that differ there differ
    bits = code_bits(dt)
    cols = -(-40 // bits)
    assert cols <= dim and cols * bits <= 64
    lead = feature_rows(np.arange(N), cols, dt).astype(np.uint64) if cols == dim else \
        feature_code(np.arange(N, dtype=np.uint64)[:, None] * np.uint64(dim) + np.arange(cols, dtype=np.uint64), bits).astype(np.uint64)
    assert np.array_equal(lead[:50].astype(np.int64), feature_rows(np.arange(min(N, 50)), dim, dt)[:, :cols].astype(np.int64))
    key = np.zeros(N, np.uint64)
    for c in range(cols):
        key = (key << np.uint64(bits)) | lead[:, c]
    assert np.unique(key).size == N


@pytest.mark.parametrize("row_bytes,dtype", [(100, np.uint8), (136, np.uint8), (256, np.float16), (400, np.float32),
                                             (512, np.float32), (1024, np.float32), (4096, np.float32)])
def test_rows_a_power_of_two_of_bytes_apart_differ(row_bytes, dtype):
    """Row r and the row at or just before / after r * row_bytes + 2^k bytes, k = 16 .. 36: what a gather that drops
    or adds bit k of a byte offset reads instead.  Row sizes that do not divide 2^k: both neighbouring rows."""
    dim = row_bytes // np.dtype(dtype).itemsize
    r = np.concatenate([np.arange(200), np.random.RandomState(row_bytes).randint(0, 1 << 22, 300)]).astype(np.int64)
    mine = feature_rows(r, dim, dtype)
    for k in range(16, 37):
        for other in {(1 << k) // row_bytes, -((1 << k) // -row_bytes)}:
            assert other > 0
            theirs = feature_rows(r + other, dim, dtype)
            assert (mine != theirs).any(axis=1).all(), (k, other)
            assert (mine != theirs).mean() > 0.9, (k, other)


def masked_gather(row_of, ids, dim, mask_bits):
    """What a 4-byte-element gather returns whose BYTE offset row * dim * 4 + 4 j is cut to mask_bits bits: element
    (offset & mask) / 4 of the table, computed from the table's closed form `row_of` (no 57 GB array)."""
    off = (np.asarray(ids, np.int64)[:, None] * dim + np.arange(dim)) * 4
    elem = (off & ((1 << mask_bits) - 1)) // 4
    rows, cols = elem // dim, elem % dim
    out = np.empty(elem.shape, np.float32)
    for c in np.unique(cols):  # row_of gives whole rows: take each needed column of them
        m = cols == c
        out[m] = row_of(rows[m], dim)[:, c]
    return out


@pytest.mark.parametrize("N,dim", [PAPERS, FRIENDSTER], ids=["papers100M", "friendster"])
@pytest.mark.parametrize("mask_bits", [31, 32])
def test_a_truncated_gather_is_rejected_and_the_old_form_accepted_it(N, dim, mask_bits):
    """The full-size shapes (dim 128 / 256 f32: 512- / 1024-byte rows, tables of 56.9 and 67.2 GB).  Ids whose byte
    offsets pass 2^31 and 2^32: the first row past each, one inside, the last."""
    first = (1 << mask_bits) // (dim * 4)
    ids = np.array([first, first + 1, (1 << 32) // (dim * 4), (1 << 32) // (dim * 4) + 1, 50_000_000, N - 1], np.int64)
    assert (ids * dim * 4 >= 1 << mask_bits).all() and ids.max() < N
    new = lambda r, d: feature_rows(r, d, np.float32)  # noqa: E731
    # the new code: every row of the truncated gather differs from the row asked for
    got = masked_gather(new, ids, dim, mask_bits)
    want = new(ids, dim)
    assert (got != want).any(axis=1).all()
    assert np.array_equal(masked_gather(new, ids, dim, 63), want)  # (the untruncated gather is the identity)
    # the old closed form: 2^31 and 2^32 bytes are multiples of its period, the truncated gather passed its check
    assert np.array_equal(masked_gather(old_rows, ids, dim, mask_bits), old_rows(ids, dim))
