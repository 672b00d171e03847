"""Config key inline_heads on the host: which configurations config + data_init take (no GPU touched) and every refusal
by name."""
import numpy as np
import pytest

from config_run import ARCH0, run_config
from graphgen import feature_rows, powerlaw_csr
from xgnn_amd import datagen


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    path = tmp_path_factory.mktemp("heads_cfg")
    ip, ix = powerlaw_csr(600, mean_deg=9, seed=2)
    g = dict(indptr=ip, indices=ix, train_set=np.arange(0, 600, 3, dtype=np.uint32), meta=dict(feat_dim=20, num_class=13))
    datagen.write_dataset(str(path), g, feat=feature_rows(np.arange(600), 20), label=np.arange(600) % 13)
    return str(path)


ACCEPTED = [
    ("auto", dict(inline_heads="auto", _sample_type=7)),
    ("on", dict(inline_heads=1, _sample_type=7)),
    ("on-khop0", dict(inline_heads=1, _sample_type=0)),
    ("off", dict(inline_heads=0, _sample_type=7)),
    ("off-arch0", dict(ARCH0, inline_heads=0)),
    ("auto-arch0", dict(ARCH0, inline_heads="auto")),  # auto asks for nothing where nothing is built
    ("auto-khop2", dict(inline_heads="auto", _sample_type=5)),
]


@pytest.mark.parametrize("case", ACCEPTED, ids=[c[0] for c in ACCEPTED])
def test_accepted(dataset, case):
    out = run_config(dataset, case[1])
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.split() == ["configured", "13", "20"]


REFUSED = [
    ("bad-value", dict(inline_heads="yes"), ["inline_heads = yes", "auto (the default), 0 or 1"]),
    ("arch0", dict(ARCH0, inline_heads=1), ["inline_heads = 1", "arch1"]),
    ("arch3", dict(inline_heads=1, _arch=3, trainer_ctx="cuda:1"), ["inline_heads = 1", "arch1"]),
    ("khop2", dict(inline_heads=1, _sample_type=5), ["inline_heads = 1", "khop2", "permutes"]),
]


@pytest.mark.parametrize("case", REFUSED, ids=[c[0] for c in REFUSED])
def test_refused_by_name(dataset, case):
    _, extra, words = case
    out = run_config(dataset, extra)
    assert out.returncode < 0 and "configured" not in out.stdout, out.stderr[-2000:]  # SIGABRT, like every fatal
    for w in words:
        assert w in out.stderr, (w, out.stderr[-2000:])
