"""arch5 on the GPU: S sampler processes pack every batch into a slot of the batch queue (shared host memory), T
trainer processes unpack it onto their GPU and gather its rows.  On a one-GPU box every process is mapped onto that GPU
(SAMGRAPH_FORCE_DEVICE=0); a case that needs two real devices skips when fewer are visible."""
import ctypes as C
import json
import mmap
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

import oracle
from test_arch5_config import dist_shuffler_slices
from test_engine import _check, make_dataset
from test_gpu_arch3 import _presample_states, _weighted_dataset
from xgnn_amd._lib import COUNTS_WORDS, COUNT_EDGES, COUNT_INPUT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER5 = os.path.join(ROOT, "tests", "arch5_driver.py")
FORCED = dict(os.environ, SAMGRAPH_FORCE_DEVICE="0")
UNFORCED = {k: v for k, v in os.environ.items() if k != "SAMGRAPH_FORCE_DEVICE"}

CODES = {"khop3": oracle.KHOP3, "khop0": oracle.KHOP0, "khop2": oracle.KHOP2, "weighted_khop": oracle.WEIGHTED_KHOP,
         "random_walk": oracle.RANDOM_WALK}


def _two_devices():
    return torch.cuda.is_available() and torch.cuda.device_count() >= 2


def _nstates(sample_type, bs, fan):
    """The engine's RNG pool size (as tests/test_engine.py::_oracle_batches restates it)."""
    max_seeds = int(bs * 1.25) + 1
    p = oracle.predict_num_nodes(max_seeds, fan, len(fan) - 1)
    if sample_type == "weighted_khop":
        return min(oracle.predict_num_nodes(max_seeds, fan, len(fan)), 512 * 1024)
    if sample_type == "random_walk":
        return (p + 63) // 64 * 256
    return max(p, (p + 127) // 128 * 8, (p + 1023) // 1024 * 256)


def _oracle_arch5(d, S, bs, epochs, fan, seed, sample_type, states0=None, **kw):
    """CPU replay of every sampler: the epoch's permutation seeded with the epoch number (the same on every sampler,
    applied to the previous epoch's order), the sampler's DistShuffler slice, its RNG pool seeded with
    seed + 1000003 * sampler id, keys epoch * steps_per_epoch + global step."""
    train = d["train"]
    steps = (train.size + bs - 1) // bs
    out = {}
    for w, (first, n_step, off, n_data) in enumerate(dist_shuffler_slices(train.size, bs, S)):
        states = states0 if (w == 0 and states0 is not None) else oracle.random_states(_nstates(sample_type, bs, fan),
                                                                                        seed + 1000003 * w)
        data = train.copy()
        for ep in range(epochs):
            data = oracle.shuffle_minstd0(data, ep)
            local = data[off:off + n_data]
            for st in range(n_step):
                seeds = local[st * bs:(st + 1) * bs]
                res = oracle.do_sample(CODES[sample_type], d["ip"], d["ix"], seeds, fan, states, **kw)
                out[ep * steps + first + st] = dict(res=res, seeds=seeds, feat=oracle.extract(d["feat"], res["input_nodes"]),
                                                    label=d["label"][seeds])
    return out


# (S, T, sample_type, fanout, cache_percentage, cache_policy, trainer mode, extra keys)
CASES = [
    (1, 1, "khop2", [5, 4], 0.0, "degree", "step", {}),
    (2, 1, "khop3", [5, 4], 0.4, "degree", "start", {"queue_depth": 2}),
    (1, 2, "khop0", [5, 4], 1.0, "degree", "step", {"extract_streams": 1}),
    (2, 2, "khop3", [5, 4], 0.4, "pre_sample", "start", {"presample_epoch": 1}),
    (2, 2, "weighted_khop", [5, 4], 0.0, "degree", "step", {}),
    (2, 1, "random_walk", [5, 5, 5], 0.4, "degree", "step", {}),
]


def _run_against_oracle(tmp_path, case, env):
    S, T, sample_type, fan, ratio, policy, mode, keys = case
    d = _weighted_dataset(tmp_path / "ds") if sample_type == "weighted_khop" else make_dataset(tmp_path / "ds")
    prefix = str(tmp_path / "out")
    seed, bs, epochs = 7, 48, 2  # 500 seeds: 11 steps per epoch, the last one of 20
    args = [f"sample_type={sample_type}", f"seed={seed}", f"batch_size={bs}", f"num_epoch={epochs}",
            "fanout=" + " ".join(map(str, fan)), f"cache_percentage={ratio}", f"cache_policy={policy}",
            "queue_timeout_s=60", "barrier_timeout=120"]
    args += [f"{k}={v}" for k, v in keys.items()]
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, DRIVER5, d["path"], prefix, str(S), str(T), mode]
                       + args, capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    kw = {}
    if sample_type == "random_walk":
        kw = dict(walk_length=3, restart_prob=0.5, num_walk=4)
    if sample_type == "weighted_khop":
        kw = dict(prob=d["prob"], alias=d["alias"])
    N = d["ip"].size - 1
    states0 = None
    if policy == "pre_sample":
        assert sample_type == "khop3"  # the presample replay (tests/test_gpu_arch3.py) samples khop3
        states0, rank = _presample_states(d, seed, bs, fan, keys["presample_epoch"])
    else:
        from xgnn_amd import datagen
        rank = datagen.degree_rank(d["ip"])
    want = _oracle_arch5(d, S, bs, epochs, fan, seed, sample_type, states0, **kw)
    steps = (d["train"].size + bs - 1) // bs
    assert sorted(want) == list(range(epochs * steps))
    # samplers: their step counts are the twin's
    for w, sl in enumerate(dist_shuffler_slices(d["train"].size, bs, S)):
        sj = json.load(open(f"{prefix}.s{w}.json"))
        assert sj["num_local_step"] == sl[1] and sj["steps_per_epoch"] == steps
        assert all(v == 0 for v in sj["epoch_items"]["KLogEpochSampleGetCacheMissIndexTime"])
        assert all(v > 0 for v in sj["epoch_items"]["kLogEpochSampleTotalTime"])
    cached = np.zeros(N, bool)
    cached[rank[: int(N * ratio)]] = True
    row_bytes = d["feat"].shape[1] * 4
    seen = []
    for w in range(T):
        npz = np.load(f"{prefix}.t{w}.npz")
        info = json.load(open(f"{prefix}.t{w}.json"))
        mine = sorted({int(k.split(":")[0]) for k in npz.files})
        # the scripts' split: steps w, w + T, ... of each epoch -- as many messages, whichever keys they carry
        assert len(info["keys"]) == len(mine) == epochs * len(range(w, steps, T))
        assert info["num_local_step"] == len(range(w, steps, T))
        _check(npz, {k: want[k] for k in mine}, len(fan))
        for key in mine:
            nmiss = int((~cached[want[key]["res"]["input_nodes"]]).sum()) if ratio > 0 else 0
            assert float(npz[f"{key}:miss_bytes"]) == nmiss * row_bytes, key
        for st in info["steps"]:
            assert st["kLogL2GraphCopyTime"] > 0 and st["kLogL1CopyTime"] >= st["kLogL1RecvTime"] >= 0
        seen += mine
    assert sorted(seen) == sorted(want)  # every key of every epoch arrived exactly once, across all trainers
    return prefix


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"S{c[0]}T{c[1]}-{c[2]}-{c[5]}{c[4]}-{c[6]}")
def test_arch5_forced_equals_the_oracle(tmp_path, case):
    """Every batch of two epochs, whichever trainer it reached, equals the oracle's replay of its sampler: COO per
    layer, num_src / num_dst, input / output nodes, feature rows, labels, kLogL1NumSample, and the cache's miss bytes."""
    _run_against_oracle(tmp_path, case, FORCED)


@pytest.mark.gpu
@pytest.mark.skipif(not _two_devices(), reason="fewer than two GPUs visible: samplers and trainers on separate devices "
                                                "are unexercised here")
def test_arch5_two_devices_equals_the_oracle(tmp_path):
    """No force: sampler cuda:0, trainer cuda:1 -- the oracle comparison, and every tensor on the trainer's GPU."""
    prefix = _run_against_oracle(tmp_path, (1, 1, "khop3", [5, 4], 0.4, "degree", "start", {}), UNFORCED)
    info = json.load(open(prefix + ".t0.json"))
    assert info["devices"] and all(devs == ["cuda:1"] for devs in info["devices"])


@pytest.mark.gpu
def test_arch5_sampler_that_exits_before_sending_ends_the_trainers(tmp_path):
    """The only sampler returns normally right after sample_init (no fault, no kill): both trainers wait for a batch
    that never comes and end at queue_timeout_s with the fatal message, instead of hanging."""
    d = make_dataset(tmp_path / "ds")
    t0 = time.time()
    r = subprocess.run(["timeout", "-k", "10", "120", sys.executable, DRIVER5, d["path"], str(tmp_path / "out"), "1", "2",
                        "step", "seed=3", "num_epoch=1", "exit_sampler=0", "queue_timeout_s=3", "barrier_timeout=60"],
                       capture_output=True, text=True, timeout=180, env=FORCED)
    assert r.returncode == 1, (r.returncode, r.stderr[-3000:])
    assert r.stderr.count("for a batch from the samplers") == 2, r.stderr[-3000:]
    assert "queue_timeout_s = 3 s passed" in r.stderr
    assert time.time() - t0 < 100


# ---- the pack / unpack kernels against numpy ------------------------------------------------------------------------
def _hip():
    torch.cuda.init()
    return C.CDLL("libamdhip64.so")


@pytest.mark.gpu
def test_queue_pack_unpack_leaf_against_numpy():
    """ggms_queue_pack into a slot of registered (mapped) host memory, then ggms_queue_unpack out of it: random lengths
    with 0 and byte sizes that are not a multiple of 16, every length read from device words (the pack: the batch's
    counts; the unpack: the slot's header), a length beyond its bound clamped to it.  The header carries key,
    num_output, num_layer and the counts words verbatim; the slot's seq word and every byte past each length (in the
    slot and in the destination buffers) stay untouched."""
    from xgnn_amd import ops
    hip = _hip()
    dev = torch.device("cuda", 0)
    rng = np.random.RandomState(11)
    L, max_edges, max_input, max_output = 3, [37, 1000, 4099], 777, 65
    lay = ops.queue_layout(max_edges, max_input, max_output, has_data=True)
    assert lay.slot_bytes % 4096 == 0 and lay.off_row[0] == 512
    size = lay.slot_bytes
    mm = mmap.mmap(-1, size)  # MAP_SHARED | MAP_ANONYMOUS, as the engine's queue
    host = np.frombuffer(mm, dtype=np.uint8)
    addr = C.addressof(C.c_char.from_buffer(mm))
    assert hip.hipHostRegister(C.c_void_p(addr), C.c_size_t(size), C.c_uint(2)) == 0  # hipHostRegisterMapped
    dptr = C.c_void_p()
    assert hip.hipHostGetDevicePointer(C.byref(dptr), C.c_void_p(addr), C.c_uint(0)) == 0
    try:
        segs = [(f"row{i}", lay.off_row[i], max_edges[i]) for i in range(L)] + \
               [(f"col{i}", lay.off_col[i], max_edges[i]) for i in range(L)] + \
               [(f"data{i}", lay.off_data[i], max_edges[i]) for i in range(L)] + \
               [("input", lay.off_input, max_input), ("output", lay.off_output, max_output)]
        for trial, edges in enumerate([[0, 1, 4099], [37, 999, 3], [5, 0, 4101], [36, 1000, 0]]):
            n_in = [0, 777, 13, 778][trial]
            n_out = [65, 0, 3, 99][trial]
            src = {name: torch.from_numpy(rng.randint(0, 1 << 31, bound, dtype=np.int64).astype(np.int32)).to(dev)
                   for name, _, bound in segs}
            counts = rng.randint(0, 1 << 40, COUNTS_WORDS(L)).astype(np.int64)
            for i in range(L):
                counts[COUNT_EDGES(i)] = edges[i]
            counts[COUNT_INPUT(L)] = n_in
            counts_dev = torch.from_numpy(counts).to(dev)
            host[:] = 0xA5
            key = 1000 + trial
            ops.queue_pack(dptr.value, lay, [src[f"row{i}"] for i in range(L)], [src[f"col{i}"] for i in range(L)],
                           [src[f"data{i}"] for i in range(L)], src["input"], src["output"], counts_dev, key, n_out)
            torch.cuda.synchronize()
            hdr = host[:512].view(np.uint64)
            assert hdr[0] == np.uint64(0xA5A5A5A5A5A5A5A5)  # seq: the host's
            assert (int(hdr[1]), int(hdr[2]), int(hdr[3])) == (key, min(n_out, max_output), L)
            assert (host[32:64] == 0xA5).all()
            assert np.array_equal(hdr[8:8 + COUNTS_WORDS(L)].view(np.int64), counts)
            assert (host[64 + 8 * COUNTS_WORDS(L):512] == 0xA5).all()
            lengths = {f"{a}{i}": min(edges[i], max_edges[i]) for a in ("row", "col", "data") for i in range(L)}
            lengths.update(input=min(n_in, max_input), output=min(n_out, max_output))
            for name, off, bound in segs:
                n = lengths[name]
                got = host[off:off + bound * 4].view(np.int32)
                assert np.array_equal(got[:n], src[name].cpu().numpy()[:n]), (trial, name)
                assert (host[off + n * 4:off + bound * 4] == 0xA5).all(), (trial, name)
            # unpack into poisoned buffers one element longer than the bound: nothing past the length is written
            dst = {name: torch.full((bound + 1,), -7, dtype=torch.int32, device=dev) for name, _, bound in segs}
            dcounts = torch.full((COUNTS_WORDS(L) + 1,), -7, dtype=torch.int64, device=dev)
            ops.queue_unpack(dptr.value, lay, [dst[f"row{i}"] for i in range(L)], [dst[f"col{i}"] for i in range(L)],
                             [dst[f"data{i}"] for i in range(L)], dst["input"], dst["output"], dcounts)
            torch.cuda.synchronize()
            assert np.array_equal(dcounts.cpu().numpy()[:-1], counts) and int(dcounts[-1]) == -7
            for name, _, bound in segs:
                n = lengths[name]
                got = dst[name].cpu().numpy()
                assert np.array_equal(got[:n], src[name].cpu().numpy()[:n]), (trial, name)
                assert (got[n:] == -7).all(), (trial, name)
    finally:
        torch.cuda.synchronize()
        assert hip.hipHostUnregister(C.c_void_p(addr)) == 0
