"""The learnable feature table on a host without a GPU: the numpy twin of ggms_update_rows against float64, the C ABI's
refusals (INVALID before any device call), the header's constants, and which configurations config + data_init take
with the key feat_learnable and which they refuse, naming the deployment or the key."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import update_rows_ref as ref
from config_run import ARCH0, run_config
from test_engine import make_dataset
from xgnn_amd import _lib, ops
from xgnn_amd._lib import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1  # GGMS_ERR_INVALID
U = 2.0 ** -24  # unit roundoff of f32 (round to nearest): |fl(x) - x| <= U |x| for a normal result


def _err():
    return lib().ggms_last_error().decode()


# ---- the twin against float64 ---------------------------------------------------------------------------------------------
def _normal_values(rs, shape, lo, hi, nonneg=False):
    v = np.power(10.0, rs.uniform(lo, hi, shape))
    if not nonneg:
        v *= rs.choice([-1.0, 1.0], shape)
    return v.astype(np.float32)


@pytest.mark.parametrize("rule", [ref.SGD, ref.ADAGRAD], ids=["sgd", "adagrad"])
def test_twin_against_float64(rule):
    """Magnitudes 1e-6 .. 1e6 (every intermediate a NORMAL f32, so each f32 operation errs by at most U relative to its
    exact result; float64's own error, 2^-53 per operation, is 2^-29 of that and is covered by the slack of 1 U below).

    SGD: step' = lr g (1 + d1), w' = (w - step')(1 + d2), |d| <= U.  Against the exact w - lr g:
        |w' - exact| <= U |step| + U |w - step'| + O(U^2) <= U |step| + U (|w| + |step|)  <=  3 U max(|w|, |step|).
    Adagrad: five roundings reach the step -- g g, s + g g, sqrt, + eps, lr g, and the divide makes six:
        s' = (s + g g (1 + d1))(1 + d2): relative error <= 2 U (both terms are >= 0, nothing cancels);
        sqrt halves that and adds its own: r = sqrt(s')(1 + d3), relative error <= 2 U;
        den = (r + eps)(1 + d4), eps > 0: relative error <= 3 U;  num = lr g (1 + d5): U;
        step' = num / den (1 + d6): relative error <= U + 3 U + U = 5 U (+ O(U^2));
        w' = (w - step')(1 + d7): |w' - exact| <= 5 U |step| + U (|w| + |step|)  <=  7 U max(|w|, |step|).
    The state itself: |s' - exact| <= 2 U |exact|.
    The bounds are asserted with one more U for the second-order terms and the float64 yardstick's own rounding."""
    rs = np.random.RandomState(11 + rule)
    n = 200_000
    w = _normal_values(rs, n, -6, 6)
    g = _normal_values(rs, n, -6, 6)
    s = _normal_values(rs, n, -6, 6, nonneg=True)
    lr, eps = np.float32(0.0123), np.float32(1e-10)
    w64, s64, step64 = ref.rule_f64(rule, w, s, g, lr, eps)
    scale = np.maximum(np.abs(w.astype(np.float64)), np.abs(step64))
    if rule == ref.SGD:
        got = ref.sgd(w, g, lr)
        assert got.dtype == np.float32
        assert (np.abs(got.astype(np.float64) - w64) <= (3 + 1) * U * scale).all()
    else:
        got, s2 = ref.adagrad(w, s, g, lr, eps)
        assert got.dtype == np.float32 and s2.dtype == np.float32
        assert (np.abs(s2.astype(np.float64) - s64) <= (2 + 1) * U * s64).all()
        assert (np.abs(got.astype(np.float64) - w64) <= (7 + 1) * U * scale).all()


def test_twin_rounds_every_operation():
    """Cases where one fused operation would give other bits than two rounded ones: the twin gives the two-rounding
    result (computed here by hand from exact integers)."""
    # lr * g = (1 + 2^-12)^2 = 1 + 2^-11 + 2^-24 rounds to 1 + 2^-11 (tie to even); w - that = 2^-24 exactly under an FMA
    lr = g = np.float32(1 + 2.0 ** -12)
    w = np.float32(1 + 2.0 ** -11)
    assert ref.sgd(np.array([w]), np.array([g]), lr)[0] == 0.0
    assert float(w) - float(lr) * float(g) == -2.0 ** -24  # what a single rounding would have left
    # the accumulator's add: fl(g g) = 1 + 2^-11 has lost the 2^-24 that, with s = 2^-30, would carry the sum past the tie
    s2 = ref.adagrad(np.array([0], np.float32), np.array([2.0 ** -30], np.float32), np.array([g]), 0.0, 1.0)[1][0]
    assert s2 == np.float32(1 + 2.0 ** -11)  # fl(2^-30 + fl(g g)); fused: 1 + 2^-11 + 2^-23 after one rounding
    assert np.float32(2.0 ** -30 + float(g) * float(g)) == np.float32(1 + 2.0 ** -11 + 2.0 ** -23)


def test_twin_table_update_rules():
    """Distinct nodes, EMPTY skipped, a count below the bound, other rows untouched, repeats refused."""
    rs = np.random.RandomState(3)
    table = rs.randn(10, 3).astype(np.float32)
    state = np.abs(rs.randn(10, 3)).astype(np.float32)
    t0, s0 = table.copy(), state.copy()
    nodes = np.array([7, ref.EMPTY, 2, 9], np.uint32)
    grad = rs.randn(4, 3).astype(np.float32)
    ref.update_rows(table, state, nodes, grad, ref.ADAGRAD, 0.1, 1e-10, count=3)
    touched = np.zeros(10, bool)
    touched[[7, 2]] = True
    assert (table[~touched] == t0[~touched]).all() and (state[~touched] == s0[~touched]).all()
    want_w, want_s = ref.adagrad(t0[[7, 2]], s0[[7, 2]], grad[[0, 2]], 0.1, 1e-10)
    assert (table[[7, 2]] == want_w).all() and (state[[7, 2]] == want_s).all()
    with pytest.raises(AssertionError):
        ref.update_rows(table, state, np.array([1, 1], np.uint32), grad[:2], ref.SGD, 0.1)


# ---- the C ABI ------------------------------------------------------------------------------------------------------------
def test_update_rows_refusals():
    l = lib()
    p = C.c_void_p(1 << 20)  # never dereferenced: the checks come first
    SGD, ADA = ops.UPDATE_SGD, ops.UPDATE_ADAGRAD
    call = l.ggms_update_rows
    cases = [
        ("null table", (None, p, p, 8, None, p, 4, SGD, 0.1, 1e-10, None), "table"),
        ("null nodes", (p, p, None, 8, None, p, 4, SGD, 0.1, 1e-10, None), "nodes"),
        ("null grad", (p, p, p, 8, None, None, 4, SGD, 0.1, 1e-10, None), "grad"),
        ("dim 0", (p, p, p, 8, None, p, 0, SGD, 0.1, 1e-10, None), "dim"),
        ("unknown rule", (p, p, p, 8, None, p, 4, 2, 0.1, 1e-10, None), "rule"),
        ("negative rule", (p, p, p, 8, None, p, 4, -1, 0.1, 1e-10, None), "rule"),
        ("adagrad without state", (p, None, p, 8, None, p, 4, ADA, 0.1, 1e-10, None), "state"),
        ("lr nan", (p, None, p, 8, None, p, 4, SGD, float("nan"), 1e-10, None), "lr"),
        ("lr inf", (p, None, p, 8, None, p, 4, SGD, float("inf"), 1e-10, None), "lr"),
        ("eps 0", (p, p, p, 8, None, p, 4, ADA, 0.1, 0.0, None), "eps"),
        ("eps negative", (p, p, p, 8, None, p, 4, ADA, 0.1, -1e-10, None), "eps"),
        ("eps nan", (p, p, p, 8, None, p, 4, ADA, 0.1, float("nan"), None), "eps"),
        ("eps inf", (p, p, p, 8, None, p, 4, ADA, 0.1, float("inf"), None), "eps"),
        ("misaligned table", (C.c_void_p((1 << 20) + 2), None, p, 8, None, p, 4, SGD, 0.1, 1e-10, None), "aligned"),
    ]
    for name, args, word in cases:
        assert call(*args) == INVALID, name
        assert "update_rows" in _err() and "invalid argument" in _err() and word in _err(), (name, _err())
    # nothing to do is fine; SGD does not read eps
    assert call(p, None, p, 0, None, p, 4, SGD, 0.1, 0.0, None) == 0
    assert call(p, p, p, 0, None, p, 4, ADA, 0.1, 1e-10, None) == 0
    assert call(None, None, None, 0, None, None, 4, SGD, 0.1, 0.0, None) == 0
    assert call(p, p, p, 0, None, p, 0, SGD, 0.1, 0.0, None) == INVALID  # (values are checked even then)


def test_constants_of_the_header():
    text = open(os.path.join(ROOT, "include", "ggms.h")).read()
    defs = dict(re.findall(r"#define (GGMS_UPDATE_[A-Z]+) (\d+)", text))
    assert defs == {"GGMS_UPDATE_SGD": str(ops.UPDATE_SGD), "GGMS_UPDATE_ADAGRAD": str(ops.UPDATE_ADAGRAD)}
    assert (ops.UPDATE_SGD, ops.UPDATE_ADAGRAD) == (ref.SGD, ref.ADAGRAD) == (0, 1)
    assert ops.EMPTY_KEY == ref.EMPTY
    assert lib().ggms_abi_version() == 3 and _lib.COUNTS_WORDS(2) == 3 * 2 + 8  # neither moved


# ---- configurations -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    return make_dataset(tmp_path_factory.mktemp("learn_ds"))


@pytest.fixture(scope="module")
def dataset_f16(tmp_path_factory):
    return make_dataset(tmp_path_factory.mktemp("learn_ds16"), dtype=np.float16)


SGD = dict(feat_learnable="sgd", feat_lr=0.05)
ADAGRAD = dict(feat_learnable="adagrad", feat_lr=0.05)
DEDICATED = dict(sampler_ctx='cuda:0', trainer_ctx='cuda:1')


def test_arch1_takes_the_keys(dataset):
    for extra in (SGD, ADAGRAD, dict(ADAGRAD, feat_eps=1e-6), dict(SGD, task="link_prediction"),
                  dict(ADAGRAD, lookahead=0), dict(SGD, feat_out_dtype="f32"), dict(SGD, feat_lr="-1e-3"),
                  dict(SGD, feat_eps="nonsense")):  # (SGD does not read feat_eps)
        out = run_config(dataset["path"], dict(extra))
        assert out.returncode == 0, out.stderr[-2000:]
        assert out.stdout.split()[:3] == ["configured", "13", "20"]


def test_without_the_key_the_others_are_not_read(dataset):
    out = run_config(dataset["path"], dict(feat_lr="fast", feat_eps=-1))
    assert out.returncode == 0 and "configured" in out.stdout, out.stderr[-2000:]
    out = run_config(dataset["path"], dict(feat_lr=0.1), env_extra={"SAMGRAPH_EMPTY_FEAT": "10"})
    assert out.returncode == 0 and "configured" in out.stdout, out.stderr[-2000:]


@pytest.mark.parametrize("arch,extra", [
    ("arch0", ARCH0), ("arch3", dict(DEDICATED, _arch=3)),
    ("arch4", dict(_arch=4, sampler_ctx='cuda:1', trainer_ctx='cuda:0')),
    ("arch5", dict(_arch=5, num_sample_worker=1, num_train_worker=1)), ("arch6", dict(_arch=6, num_worker=1))])
@pytest.mark.parametrize("rule", [SGD, ADAGRAD], ids=["sgd", "adagrad"])
def test_other_deployments_refuse_by_name(dataset, arch, extra, rule):
    out = run_config(dataset["path"], dict(extra, **rule))
    assert out.returncode != 0 and "configured" not in out.stdout
    assert arch in out.stderr and "feat_learnable" in out.stderr, out.stderr[-2000:]


def test_f16_dataset_is_refused(dataset_f16):
    out = run_config(dataset_f16["path"], dict(SGD))
    assert out.returncode != 0 and "configured" not in out.stdout
    assert "feat_learnable" in out.stderr and "FEAT_DATA_TYPE" in out.stderr and "F16" in out.stderr, out.stderr[-2000:]
    out = run_config(dataset_f16["path"], {})  # the dataset itself is fine
    assert out.returncode == 0, out.stderr[-2000:]


REFUSED = [
    ("store-dtype", dict(SGD, feat_store_dtype="F16"), None, ["feat_learnable", "feat_store_dtype"]),
    ("out-dtype-f16", dict(SGD, feat_out_dtype="f16"), None, ["feat_learnable", "feat_out_dtype", "f16"]),
    ("out-dtype-bf16", dict(ADAGRAD, feat_out_dtype="bf16"), None, ["feat_learnable", "feat_out_dtype", "bf16"]),
    ("mock-table", dict(SGD), {"SAMGRAPH_EMPTY_FEAT": "10"}, ["feat_learnable", "SAMGRAPH_EMPTY_FEAT"]),
    ("unknown-rule", dict(feat_learnable="adam", feat_lr=0.1), None, ["feat_learnable", "adam"]),
    ("missing-lr", dict(feat_learnable="sgd"), None, ["feat_learnable", "feat_lr"]),
    ("missing-lr-with-lr", dict(feat_learnable="sgd", lr=0.3), None, ["feat_learnable", "feat_lr"]),
    ("lr-word", dict(SGD, feat_lr="fast"), None, ["feat_lr", "fast"]),
    ("lr-trailing", dict(SGD, feat_lr="0.1x"), None, ["feat_lr", "0.1x"]),
    ("lr-empty", dict(SGD, feat_lr=""), None, ["feat_lr"]),
    ("lr-nan", dict(SGD, feat_lr="nan"), None, ["feat_lr", "nan"]),
    ("lr-inf", dict(ADAGRAD, feat_lr="inf"), None, ["feat_lr", "inf"]),
    ("lr-beyond-f32", dict(SGD, feat_lr="1e39"), None, ["feat_lr", "1e39"]),
    ("eps-zero", dict(ADAGRAD, feat_eps=0), None, ["feat_eps", "0"]),
    ("eps-negative", dict(ADAGRAD, feat_eps=-1e-8), None, ["feat_eps", "-1e-08"]),
    ("eps-word", dict(ADAGRAD, feat_eps="tiny"), None, ["feat_eps", "tiny"]),
    ("eps-nan", dict(ADAGRAD, feat_eps="nan"), None, ["feat_eps", "nan"]),
    ("eps-below-f32", dict(ADAGRAD, feat_eps="1e-60"), None, ["feat_eps", "1e-60"]),
]


@pytest.mark.parametrize("case", REFUSED, ids=[c[0] for c in REFUSED])
def test_conflicts_and_bad_values_are_refused_by_key(dataset, case):
    _, extra, env, words = case
    out = run_config(dataset["path"], dict(extra), env_extra=env)
    assert out.returncode != 0 and "configured" not in out.stdout
    for w in words:
        assert w in out.stderr, (w, out.stderr[-2000:])
