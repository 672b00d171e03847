"""ggms_update_rows on the GPU against its numpy twin (tests/update_rows_ref.py), bit for bit.

Every case compares the WHOLE table and the whole state with the twin's, so rows the call must not touch are checked
with the rows it updates, and both lie between canaries.  Values span 1e-20 .. 1e20 in both signs with exact zeros and
f32 subnormals among them: g * g then reaches subnormals and inf, lr * g subnormals, and the Adagrad state saturates at
inf (step 0) -- all plain IEEE, no NaN arises (asserted on the twin's result, whose NaN payloads would not be pinned).
Shapes are the smallest that reach every path: rows of 4, 8, 12, 16, 100, 512 and 516 bytes (4-, 8- and 16-byte chunks,
a row that is no multiple of the widest chunk), tiles of 1, 63, 64, 65 rows and several waves (257), the long-row kernel
(8192 chunks per row), a base that is 4- or 8- but not 16-byte aligned, a device count below the bound, and one table
past 2^32 bytes."""
import numpy as np
import pytest

import update_rows_ref as ref
from graphgen import torch_feature_rows

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

EMPTY = ref.EMPTY
SENT = -123456.0  # canary value (exact in f32)
PAD = 64          # canary floats on either side: 256 bytes, so the table's base keeps its 16-byte alignment
RULES = [ref.SGD, ref.ADAGRAD]
RULE_IDS = ["sgd", "adagrad"]
LR, EPS = 0.0123, 1e-10


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (run with -m gpu on an MI355X box)")
    from xgnn_amd import ops as _ops
    return _ops


def wide_values(rs, shape, nonneg=False):
    """float32 of magnitudes 1e-20 .. 1e20, both signs, with exact zeros and subnormals sprinkled in."""
    v = np.power(10.0, rs.uniform(-20, 20, shape))
    if not nonneg:
        v *= rs.choice([-1.0, 1.0], shape)
    kind = rs.randint(0, 16, shape)
    v = np.where(kind == 0, 0.0, v)
    v = np.where(kind == 1, (-1.0 if not nonneg else 1.0) * 0.0, v)
    v = np.where(kind == 2, 1e-40 * rs.uniform(0.1, 9, shape), v)  # f32 subnormals
    v = np.where(kind == 3, 1.4e-45, v)                             # the smallest one
    out = v.astype(np.float32)
    assert np.isfinite(out).all()
    return out


def distinct_nodes(rs, rows, count, num_empty):
    """`count` entries: pairwise distinct rows in random (unsorted) order, num_empty of them replaced by EMPTY."""
    nodes = rs.permutation(rows)[:count].astype(np.uint32)
    if num_empty:
        nodes[rs.permutation(count)[:num_empty]] = EMPTY
    return nodes


def i32_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).cuda()


class Guarded:
    """A (rows, dim) f32 device table inside a flat buffer: `lead` floats of slack in front (to misalign the base), then
    PAD canary floats on either side of the table."""

    def __init__(self, host, lead=0):
        rows, dim = host.shape
        self.flat = torch.full((lead + PAD + rows * dim + PAD,), SENT, dtype=torch.float32, device="cuda")
        self.lo = lead + PAD
        self.t = self.flat[self.lo:self.lo + rows * dim].view(rows, dim)
        self.t.copy_(torch.from_numpy(host))

    def check(self, want, what):
        assert bool((self.flat[:self.lo] == SENT).all()) and bool((self.flat[self.lo + self.t.numel():] == SENT).all()), \
            f"{what}: canary overwritten"
        got = self.t.cpu().numpy()
        same = got.view(np.uint32) == want.view(np.uint32)
        assert same.all(), f"{what}: {(~same).sum()} elements differ, first at {np.argwhere(~same)[0]}: " \
                           f"got {got[~same][0]!r} want {want[~same][0]!r}"


def run_case(ops, rule, rows, dim, count, seed, lead=0, repeat=1, bound=None, num_empty=None):
    """One call (or `repeat` calls with fresh gradients over the same rows) against the twin.  bound: the call passes
    it as num with the device count `count`; rows of grad behind the count are canaries that must not be applied."""
    rs = np.random.RandomState(seed)
    n_arg = count if bound is None else bound
    table = wide_values(rs, (rows, dim))
    state = wide_values(rs, (rows, dim), nonneg=True)
    if num_empty is None:
        num_empty = min(3, n_arg // 8)
    nodes = distinct_nodes(rs, rows, n_arg, num_empty)
    d_table, d_state = Guarded(table, lead), Guarded(state, lead)
    assert d_table.t.data_ptr() % 4 == 0 and (lead == 0 or d_table.t.data_ptr() % 16 != 0)
    d_nodes = i32_dev(nodes)
    num_dev = None if bound is None else torch.tensor([count], dtype=torch.int64, device="cuda")
    for _ in range(repeat):
        grad = wide_values(rs, (n_arg, dim))
        ops.update_rows(d_table.t, d_nodes, torch.from_numpy(grad).cuda(), rule, LR, EPS,
                        state=d_state.t if rule == ref.ADAGRAD else None, num=n_arg, num_dev=num_dev)
        ref.update_rows(table, state, nodes, grad, rule, LR, EPS, count=count)
    torch.cuda.synchronize()
    assert not np.isnan(table).any() and not np.isnan(state).any()
    what = f"rule {rule} rows {rows} dim {dim} count {count}"
    d_table.check(table, what + " table")
    d_state.check(state, what + " state")  # SGD: untouched as a whole


@pytest.mark.parametrize("dim", [1, 2, 3, 4, 25, 128, 129])
@pytest.mark.parametrize("rule", RULES, ids=RULE_IDS)
def test_update_rows_matches_twin(ops, rule, dim):
    for k, count in enumerate([1, 63, 64, 65, 257]):
        run_case(ops, rule, 1000, dim, count, seed=1000 * dim + 10 * k + rule)


@pytest.mark.parametrize("rule", RULES, ids=RULE_IDS)
def test_update_rows_long_rows(ops, rule):
    """dim 32768: 8192 16-byte chunks per row, the one-workgroup-per-row kernel; 3 of 5 rows, one entry EMPTY."""
    run_case(ops, rule, 5, 32768, 3, seed=77 + rule, num_empty=0)
    run_case(ops, rule, 5, 32768, 4, seed=79 + rule, num_empty=1)


@pytest.mark.parametrize("rule", RULES, ids=RULE_IDS)
def test_update_rows_device_count(ops, rule):
    """The count is read on the device: rows of grad behind it (and their nodes) are not applied."""
    for dim, count, bound in [(25, 70, 257), (128, 64, 65), (4, 0, 130), (3, 1, 64)]:
        run_case(ops, rule, 1000, dim, count, seed=5000 + dim + rule, bound=bound)


@pytest.mark.parametrize("lead", [1, 2, 3])
@pytest.mark.parametrize("rule", RULES, ids=RULE_IDS)
def test_update_rows_misaligned_base(ops, rule, lead):
    """Table and state start 4, 8 or 12 bytes past a 16-byte boundary: rows of 512 bytes then move in 4- or 8-byte chunks."""
    for dim in (128, 2, 25):
        run_case(ops, rule, 300, dim, 129, seed=300 + lead + rule, lead=lead)


def test_update_rows_adagrad_accumulates(ops):
    """Three calls over the same rows: the state each call reads is the one the call before wrote."""
    for dim in (25, 128):
        run_case(ops, ref.ADAGRAD, 1000, dim, 257, seed=900 + dim, repeat=3)
    run_case(ops, ref.SGD, 1000, 25, 257, seed=950, repeat=3)


def test_update_rows_nothing_to_do(ops):
    """num 0 launches nothing; a call of EMPTY entries only changes nothing."""
    run_case(ops, ref.ADAGRAD, 100, 25, 0, seed=1)
    run_case(ops, ref.SGD, 100, 25, 5, seed=2, num_empty=5)


@pytest.mark.parametrize("rule", RULES, ids=RULE_IDS)
def test_update_rows_past_4g(ops, rule):
    """A table a little past 2^32 bytes (torch.empty: only the watched rows are ever filled).  The updated rows lie on
    either side of the 2^31- and the 2^32-byte boundary; the watched rows are those, their neighbours, and the rows a
    row offset cut to 31 or 32 bits would land on.  Watched rows are compared with the twin's, updated or not."""
    dim = 128
    row_bytes = dim * 4
    rows = -(-((1 << 32) + (1 << 20)) // row_bytes)
    rs = np.random.RandomState(42 + rule)
    near = 40
    upd = np.concatenate([np.arange(b // row_bytes - near, b // row_bytes + near) for b in (1 << 31, 1 << 32)]
                         + [np.array([rows - 1, (1 << 31) // row_bytes + 12345])]).astype(np.int64)
    upd = upd[rs.permutation(upd.size)]
    assert upd.size % 64 and upd.max() < rows and (upd * row_bytes >= 1 << 32).sum() >= near
    landing = np.concatenate([(upd * row_bytes % (1 << 32)) // row_bytes, (upd * row_bytes % (1 << 31)) // row_bytes])
    watch = np.unique(np.concatenate([upd, upd - 1, upd + 1, landing, landing + 1]))
    watch = watch[(watch >= 0) & (watch < rows)]
    d_watch = torch.from_numpy(watch).cuda()

    tables = [torch.empty((rows, dim), dtype=torch.float32, device="cuda") for _ in range(2 if rule == ref.ADAGRAD else 1)]
    # the aperiodic feature code, scaled (exactly) into [0, 256) so that an Adagrad step of about lr moves every element:
    # table = code(row) / 2^16, state = code(row + rows) / 2^16
    for k, t in enumerate(tables):
        t[d_watch] = torch_feature_rows(d_watch + k * rows, dim, torch.float32) / 65536.0
    grad = (torch_feature_rows(torch.arange(upd.size, device="cuda") + 3 * rows, dim, torch.float32) / 3.0 - 2.0e6).contiguous()
    before = [t[d_watch].cpu().numpy() for t in tables]
    nodes = np.where(upd >= 1 << 31, upd - (1 << 32), upd).astype(np.int32)
    ops.update_rows(tables[0], torch.from_numpy(nodes).cuda(), grad, rule, LR, EPS,
                    state=tables[1] if rule == ref.ADAGRAD else None)
    torch.cuda.synchronize()
    want_t = before[0].copy()
    want_s = before[1].copy() if rule == ref.ADAGRAD else None
    ref.update_rows(want_t, want_s, np.searchsorted(watch, upd).astype(np.uint32), grad.cpu().numpy(), rule, LR, EPS)
    changed = (want_t.view(np.uint32) != before[0].view(np.uint32)).any(axis=1)
    assert changed.sum() == upd.size  # every updated row moved (the test would see an update that went nowhere)
    for t, want in zip(tables, [want_t, want_s]):
        got = t[d_watch].cpu().numpy()
        bad = np.flatnonzero((got.view(np.uint32) != want.view(np.uint32)).any(axis=1))
        assert bad.size == 0, f"rows {watch[bad][:8]} differ (byte offsets {watch[bad][:8] * row_bytes})"
    del tables
    torch.cuda.empty_cache()
