"""arch3 on the GPU: one GPU samples, another trains, each batch handed from the first to the second by
ggms_batch_handoff.  On a one-GPU box both contexts are mapped onto that GPU (SAMGRAPH_FORCE_DEVICE=0) and the hand-off
reads local memory; the two-device tests run where two GPUs are visible."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import oracle
from graphgen import exact_features
from test_engine import _check, _oracle_batches, make_dataset

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER3 = os.path.join(ROOT, "tests", "arch3_driver.py")
DRIVER1 = os.path.join(ROOT, "tests", "engine_driver.py")
FORCED = dict(os.environ, SAMGRAPH_FORCE_DEVICE="0")
UNFORCED = {k: v for k, v in os.environ.items() if k != "SAMGRAPH_FORCE_DEVICE"}


def _two_devices():
    return torch.cuda.is_available() and torch.cuda.device_count() >= 2


def _weighted_dataset(tmp_path):
    """make_dataset + valid per-edge tables of the weighted samplers (as test_arch1_weighted_and_random_walk)."""
    from xgnn_amd import datagen
    d = make_dataset(tmp_path)
    g = dict(indptr=d["ip"], indices=d["ix"], train_set=d["train"], meta=dict(feat_dim=d["feat"].shape[1], num_class=13))
    weights = datagen.edge_weights(g, "default", seed=3)
    datagen.write_dataset(d["path"], g, feat=d["feat"], label=d["label"], weights=weights)
    d["prob"] = np.fromfile(os.path.join(d["path"], "prob_table.bin"), np.float32)
    d["alias"] = np.fromfile(os.path.join(d["path"], "alias_table.bin"), np.uint32)
    return d


def _nstates(bs, fan):
    p = oracle.predict_num_nodes(int(bs * 1.25) + 1, fan, len(fan) - 1)
    return max(p, (p + 127) // 128 * 8, (p + 1023) // 1024 * 256)


def _presample_states(d, seed, bs, fan, epochs):
    """The RNG pool after the engine's presample (dist/pre_sampler.cc:39-139) consumed it, and the ranking it made."""
    st = oracle.random_states(_nstates(bs, fan), seed)
    N = d["ip"].size - 1
    freq = np.zeros(N, np.uint64)
    train = d["train"].copy()
    for e in range(epochs):
        train = oracle.shuffle_minstd0(train, seed + 0x5A5A5A + e)
        for off in range(0, train.size, bs):
            res = oracle.do_sample(oracle.KHOP3, d["ip"], d["ix"], train[off:off + bs], fan, st)
            freq[res["input_nodes"]] += 1
    keys = (freq << np.uint64(32)) | np.arange(N, dtype=np.uint64)
    return st, (np.sort(keys)[::-1] & np.uint64(0xFFFFFFFF)).astype(np.uint32)


# (sample_type, fanout, cache_percentage, cache_policy, extra keys, driver mode)
CASES = [
    ("khop3", [5, 4], 0.0, "degree", dict(lookahead=2, extract_streams=2), "step"),
    ("khop3", [5, 4], 0.4, "degree", dict(lookahead=0, extract_streams=1), "start"),
    ("khop3", [5, 4], 0.4, "pre_sample", dict(presample_epoch=1), "step"),
    ("khop3", [5, 4], 1.0, "degree", dict(lookahead=2, pipelines=2, extract_streams=2), "start"),
    ("khop0", [5, 4], 0.4, "degree", dict(extract_streams=1), "step"),
    ("khop0", [5, 4], 1.0, "degree", dict(lookahead=0), "start"),
    ("khop2", [5, 4], 0.0, "degree", dict(), "start"),
    ("khop2", [5, 4], 0.4, "degree", dict(extract_streams=1), "step"),
    ("random_walk", [5, 5, 5], 0.4, "degree", dict(), "step"),
    ("random_walk", [5, 5, 5], 0.0, "degree", dict(lookahead=0), "start"),
    ("weighted_khop", [5, 4], 1.0, "degree", dict(), "start"),
    ("weighted_khop", [5, 4], 0.0, "degree", dict(extract_streams=1), "step"),
]


def _run_against_oracle(tmp_path, case, env):
    sample_type, fan, ratio, policy, keys, mode = case
    d = _weighted_dataset(tmp_path / "ds") if sample_type == "weighted_khop" else make_dataset(tmp_path / "ds")
    prefix = str(tmp_path / "out")
    seed, bs, epochs = 7, 64, 3
    args = [f"sample_type={sample_type}", f"seed={seed}", f"batch_size={bs}", f"num_epoch={epochs}",
            "fanout=" + " ".join(map(str, fan)), f"cache_percentage={ratio}", f"cache_policy={policy}"]
    args += [f"{k}={v}" for k, v in keys.items()]
    r = subprocess.run([sys.executable, DRIVER3, d["path"], prefix, mode] + args, capture_output=True, text=True,
                       timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    kw = {}
    if sample_type == "random_walk":
        kw = dict(walk_length=3, restart_prob=0.5, num_walk=4)
    if sample_type == "weighted_khop":
        kw = dict(prob=d["prob"], alias=d["alias"])
    N = d["ip"].size - 1
    if policy == "pre_sample":
        states, rank = _presample_states(d, seed, bs, fan, keys["presample_epoch"])
        want = _oracle_batches(d, 0, 1, bs, epochs, fan, seed, arch6=False, states=states)
    else:
        from xgnn_amd import datagen
        rank = datagen.degree_rank(d["ip"])
        want = _oracle_batches(d, 0, 1, bs, epochs, fan, seed, arch6=False, sample_type=sample_type, **kw)
    npz = np.load(prefix + ".w0.npz")
    _check(npz, want, len(fan))
    cached = np.zeros(N, bool)
    cached[rank[: int(N * ratio)]] = True
    row_bytes = d["feat"].shape[1] * 4
    for key, w in want.items():  # misses: the input nodes outside the cached prefix of the ranking (none without a cache)
        nmiss = int((~cached[w["res"]["input_nodes"]]).sum()) if 0 < ratio else 0
        assert float(npz[f"{key}:miss_bytes"]) == nmiss * row_bytes, key
    if mode == "start":  # what the hand-off moved, as the profiler logs it
        info = json.load(open(prefix + ".info.json"))
        per_edge = 12 if sample_type == "random_walk" else 8
        assert len(info["steps"]) == len(want)
        for st in info["steps"]:
            w = want[st["key"]]
            assert st["graph_bytes"] == sum(l["row"].size for l in w["res"]["layers"]) * per_edge
            assert st["id_bytes"] == (w["res"]["input_nodes"].size + w["seeds"].size) * 4
            assert st["graph_copy_s"] > 0 and st["copy_s"] > 0
            assert st["feature_bytes"] == w["res"]["input_nodes"].size * row_bytes
    return prefix


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}-{c[3]}{c[2]}-{c[5]}-" + ",".join(f"{k}{v}" for k, v in c[4].items()))
def test_arch3_forced_equals_the_oracle(tmp_path, case):
    """Every batch of three epochs equals the oracle's replay of the arch1 shuffler + sampler + extract: COO per layer,
    num_src / num_dst, input / output nodes, feature rows, labels, kLogL1NumSample, and the miss bytes of the cache."""
    _run_against_oracle(tmp_path, case, FORCED)


def _feature_dataset(tmp_path, dtype):
    """make_dataset with another feature type: meta FEAT_DATA_TYPE says which."""
    from xgnn_amd import datagen
    d = make_dataset(tmp_path)
    names = {np.dtype(np.float16): "F16", np.dtype(np.float64): "F64", np.dtype(np.float32): "F32"}
    feat = exact_features(d["ip"].size - 1, 9, dtype)
    g = dict(indptr=d["ip"], indices=d["ix"], train_set=d["train"], meta=dict(feat_dim=9, num_class=13))
    datagen.write_dataset(d["path"], g, feat=feat, label=d["label"], feat_dtype=names[np.dtype(dtype)])
    return d


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,keys", [(np.float32, ["lookahead=2"]), (np.float16, ["lookahead=0"]),
                                        (np.float64, ["extract_streams=1"]), (np.float32, ["sample_type=khop0"])])
def test_arch3_batches_are_the_arch1_batches(tmp_path, dtype, keys):
    """Same keys and seed: every array of the arch3 run's dump is byte for byte the arch1 run's (tests/engine_driver.py)."""
    d = _feature_dataset(tmp_path / "ds", dtype)
    common = ["seed=11", "batch_size=64", "num_epoch=2", "fanout=5 4"] + keys
    r1 = subprocess.run([sys.executable, DRIVER1, d["path"], str(tmp_path / "a1"), "arch1", "1"] + common,
                        capture_output=True, text=True, timeout=600, env=UNFORCED)
    assert r1.returncode == 0, r1.stderr[-3000:]
    r3 = subprocess.run([sys.executable, DRIVER3, d["path"], str(tmp_path / "a3"), "step"] + common,
                        capture_output=True, text=True, timeout=600, env=FORCED)
    assert r3.returncode == 0, r3.stderr[-3000:]
    # (the archive itself carries write times: compared member by member, in order, dtype, shape and bytes)
    a1, a3 = np.load(str(tmp_path / "a1.w0.npz")), np.load(str(tmp_path / "a3.w0.npz"))
    assert len(a1.files) > 20 and a1.files == a3.files
    for k in a1.files:
        x, y = a1[k], a3[k]
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), k


@pytest.mark.gpu
def test_batch_handoff_leaf_against_numpy():
    """ggms_batch_handoff through xgnn_amd.ops: lengths 0 .. 2^20 + 5 elements of 1, 4 and 8 bytes, from the host
    and from a device word, one segment per launch and all in one launch; every destination is poisoned and must be
    untouched past its length, also when the device word asks for more than the buffers hold."""
    from xgnn_amd import ops
    dev = torch.device("cuda", 0)
    g = torch.Generator(device="cpu").manual_seed(5)
    lengths = [0, 1, 3, 4, 63, 4097, (1 << 20) + 5]
    dtypes = [torch.int32, torch.int64, torch.uint8]
    cases = []
    for i, n in enumerate(lengths):
        for j, dt in enumerate(dtypes):
            pad = 37 + i + j  # room behind the length: must stay poisoned
            src = torch.randint(0, 255 if dt == torch.uint8 else 1 << 30, (n + pad,), generator=g, dtype=dt).to(dev)
            dst = torch.full((n + pad,), 0x5A, dtype=dt, device=dev)
            on_device = (i + j) % 2 == 0
            count = torch.tensor([n], dtype=torch.int64, device=dev) if on_device else n
            cases.append((src, dst, count, n))

    def verify(items):
        torch.cuda.synchronize()
        for src, dst, _, n in items:
            s, o = src.cpu().numpy(), dst.cpu().numpy()
            assert np.array_equal(o[:n], s[:n]), (n, src.dtype)
            assert (o[n:] == 0x5A).all(), (n, src.dtype)

    for c in cases:  # one segment per launch
        ops.batch_handoff([c[:3]])
    verify(cases)
    for _, dst, _, _ in cases:
        dst.fill_(0x5A)
    ops.batch_handoff([c[:3] for c in cases])  # every segment in one launch
    verify(cases)
    # a device-side length beyond the buffers is clamped to max_count (here: the whole buffer, nothing past it)
    src = torch.arange(1000, dtype=torch.int32, device=dev)
    big = torch.full((1200,), -1, dtype=torch.int32, device=dev)
    ops.batch_handoff([(src, big[:1000], torch.tensor([5000], dtype=torch.int64, device=dev))])
    torch.cuda.synchronize()
    assert np.array_equal(big[:1000].cpu().numpy(), np.arange(1000)) and (big[1000:].cpu().numpy() == -1).all()


@pytest.mark.gpu
@pytest.mark.skipif(not _two_devices(), reason="fewer than two GPUs visible: arch3's cross-device path (peer reads over "
                                                "xGMI, tensors on the trainer GPU) is unexercised here")
def test_arch3_tensors_on_the_trainer_gpu(tmp_path):
    """No force: sampler_ctx cuda:0, trainer_ctx cuda:1 -- every tensor the facade returns reports cuda:1."""
    d = make_dataset(tmp_path / "ds")
    prefix = str(tmp_path / "out")
    r = subprocess.run([sys.executable, DRIVER3, d["path"], prefix, "start", "seed=3", "num_epoch=1",
                        "cache_percentage=0.4"], capture_output=True, text=True, timeout=600, env=UNFORCED)
    assert r.returncode == 0, r.stderr[-3000:]
    info = json.load(open(prefix + ".info.json"))
    assert info["devices"] and all(devs == ["cuda:1"] for devs in info["devices"])


@pytest.mark.gpu
@pytest.mark.skipif(not _two_devices(), reason="fewer than two GPUs visible: arch3's cross-device path (peer reads over "
                                                "xGMI, tensors on the trainer GPU) is unexercised here")
def test_arch3_sample_once_leaves_the_trainer_gpu_current(tmp_path):
    """The foreground loop (sample_once + get_next_batch, the example scripts' default) runs on the training thread:
    after init and after every call its current device is still the trainer GPU, so torch's current stream, events,
    synchronize() and bare 'cuda' allocations belong to the GPU that trains."""
    d = make_dataset(tmp_path / "ds")
    code = f"""
import sys; sys.path.insert(0, {ROOT!r})
import torch, samgraph.torch as sam
sam.config({{'dataset_path': {d['path']!r}, '_arch': sam.kArch3, '_sample_type': sam.kKHop3, 'batch_size': 64,
  'num_epoch': 1, '_cache_policy': sam.kCacheByDegree, 'cache_percentage': 0.4, 'max_sampling_jobs': 1,
  'max_copying_jobs': 1, 'omp_thread_num': 1, 'num_layer': 2, 'num_hidden': 8, 'lr': 0.1, 'dropout': 0.5,
  'num_fanout': 2, 'fanout': [5, 4], 'sampler_ctx': 'cuda:0', 'trainer_ctx': 'cuda:1', 'seed': 3}})
torch.cuda.set_device(1)
sam.init()
seen = [torch.cuda.current_device()]
for _ in range(sam.num_epoch() * sam.num_local_step()):
    sam.sample_once()
    seen.append(torch.cuda.current_device())
    key = sam.get_next_batch()
    seen.append(torch.cuda.current_device())
    assert sam.get_graph_feat(key).device == torch.device('cuda', 1)
sam.shutdown()
print('devices', sorted(set(seen)))
"""
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=UNFORCED)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "devices [1]" in r.stdout, r.stdout[-500:]


@pytest.mark.gpu
@pytest.mark.skipif(not _two_devices(), reason="fewer than two GPUs visible: arch3's cross-device path (peer reads over "
                                                "xGMI, tensors on the trainer GPU) is unexercised here")
@pytest.mark.parametrize("case", [CASES[0], CASES[1], CASES[2], CASES[3], CASES[8], CASES[10]],
                         ids=["khop3-c0-step", "khop3-c04-start", "khop3-presample-step", "khop3-c1-start", "rw-step",
                              "weighted-start"])
def test_arch3_two_devices_equals_the_oracle(tmp_path, case):
    """The oracle comparison of test_arch3_forced_equals_the_oracle on two real GPUs (no SAMGRAPH_FORCE_DEVICE)."""
    _run_against_oracle(tmp_path, case, UNFORCED)
