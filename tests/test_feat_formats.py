"""tests/feat_formats.py itself, on the host: the tables and expected values it generates are pinned by SHA-256 digests
(tests/golden/feat_format_digests.json, recorded with the per-format helper modules this one replaced), and the checker
that judges every gather output refuses what it must."""
import hashlib
import json
import os

import numpy as np
import pytest

from feat_formats import (BF16, E4M3, E5M2, F16, F32, FAMILY, NAMES, OUTS, Q8ROW, check_output, from_f32, sentinel,
                          write_dataset)

FORMATS = (F16, BF16, F32, E4M3, E5M2, Q8ROW)


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _digests(t):
    """The stored bytes; per output dtype the expected bits (0 where NaN is expected) and the NaN positions."""
    nan = t.nan(slice(None))
    return {"stored": _sha(t.stored), **{NAMES[o]: _sha(np.where(nan, 0, t.bits(o)).astype(t.bits(o).dtype)) + ":" + _sha(nan)
                                         for o in OUTS}}


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "feat_format_digests.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("shape", [(512, 20), (8, 8193)], ids=["512x20", "8x8193"])
@pytest.mark.parametrize("fmt", FORMATS, ids=[NAMES[f] for f in FORMATS])
def test_tables_and_expected_bits_are_the_recorded_ones(golden, fmt, shape):
    """The shared gather tables (the family's own seed), short rows and rows past the long-row threshold."""
    assert _digests(FAMILY[fmt].table(fmt, *shape)) == golden[f"{NAMES[fmt]}:{shape[0]}x{shape[1]}"]


@pytest.mark.parametrize("fmt", FORMATS, ids=[NAMES[f] for f in FORMATS])
def test_dataset_tables_are_the_recorded_ones(golden, tmp_path, fmt):
    d = write_dataset(tmp_path / "d", fmt, 20)
    want = dict(golden[f"{NAMES[fmt]}:dataset20"])
    assert _sha(np.fromfile(os.path.join(d["path"], "feat.bin"), np.uint8)) == want.pop("file")
    assert _digests(d["table"]) == want
    assert {k: _sha(d[k]) for k in ("ip", "ix", "train", "label")} == golden["graph"]


# ---- check_output: a 6 x 4 output between canaries, rows 1, 3 and 4 written ------------------------------------------------
LEAD, SHAPE, DST = 5, (6, 4), np.array([3, 1, 4])


def _output(dt, nan_payload=0):
    """(flat bits of a correct buffer, expected bits, NaN mask): values -0.0, 1.5, NaN and inf per row."""
    vals = np.tile(np.array([-0.0, 1.5, np.nan, np.inf], np.float32), (3, 1)) * np.array([[1], [2], [-3]], np.float32)
    want = from_f32(np.ascontiguousarray(vals), dt).copy()
    nan = np.isnan(vals)
    flat = np.full(LEAD + 24 + 7, sentinel(dt), want.dtype)
    body = flat[LEAD:LEAD + 24].reshape(SHAPE)
    body[DST] = want
    body[DST[0], 2] ^= nan_payload
    return flat, want, nan


def _flat_index(row, col):
    return LEAD + row * SHAPE[1] + col


@pytest.mark.parametrize("dt", OUTS, ids=[NAMES[o] for o in OUTS])
def test_check_output_accepts_a_correct_output_whose_nan_has_another_payload(dt):
    flat, want, nan = _output(dt, nan_payload=1)
    assert flat[_flat_index(3, 2)] != want[0, 2]
    check_output(flat, dt, LEAD, SHAPE, DST, want, nan)


WRONG = {
    "front-canary": lambda f, dt: f.__setitem__(LEAD - 1, 0),
    "back-canary": lambda f, dt: f.__setitem__(LEAD + 24, 0),
    "row-outside-dst": lambda f, dt: f.__setitem__(_flat_index(2, 1), 0),
    "row-past-the-count": lambda f, dt: f.__setitem__(_flat_index(5, 3), 0),
    "one-bit": lambda f, dt: f.__setitem__(_flat_index(1, 1), f[_flat_index(1, 1)] ^ 1),
    "plus-zero-for-minus-zero": lambda f, dt: f.__setitem__(_flat_index(3, 0), 0),
    "finite-for-nan": lambda f, dt: f.__setitem__(_flat_index(4, 2), from_f32(np.array([1.0], np.float32), dt)[0]),
    "nan-for-finite": lambda f, dt: f.__setitem__(_flat_index(1, 1), f[_flat_index(1, 2)]),
}


@pytest.mark.parametrize("dt", OUTS, ids=[NAMES[o] for o in OUTS])
@pytest.mark.parametrize("what", WRONG)
def test_check_output_refuses(what, dt):
    flat, want, nan = _output(dt)
    check_output(flat.copy(), dt, LEAD, SHAPE, DST, want, nan)
    WRONG[what](flat, dt)
    with pytest.raises(AssertionError):
        check_output(flat, dt, LEAD, SHAPE, DST, want, nan, what)
