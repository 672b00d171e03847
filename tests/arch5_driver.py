"""Runs the samgraph_* engine as arch5 -- S sampler processes and T trainer processes joined by the batch queue -- in the
process layout of the reference's multi_gpu scripts (example/samgraph/multi_gpu/train_graphsage.py): the parent runs
config + data_init and touches no GPU, then forks S samplers and T trainers that meet at a global barrier.

    python tests/arch5_driver.py <dataset_dir> <out_prefix> <S> <T> <step|start> [extra k=v ...]

sampler w (ctx cuda:w):      sample_init, barrier, then num_epoch * num_local_step() sample_once() calls.
trainer w (ctx cuda:S + w):  barrier, train_init, then per epoch the steps w, w + T, ... of steps_per_epoch() (the
                             scripts' split): `step` calls sample_once() + get_next_batch() per step, `start` calls
                             extract_start(its count) once per epoch and get_next_batch() per step.
Each trainer writes every batch it received to <out_prefix>.t<w>.npz (the format of tests/engine_driver.py) and
<out_prefix>.t<w>.json (arrival order, tensor devices, profiler items); each sampler writes <out_prefix>.s<w>.json.

Extra keys that are not config keys: exit_sampler=<w> (that sampler calls sys.exit(0) right after sample_init and the
barrier, before it sends anything), barrier_timeout=<s>.  On a one-GPU box run it with SAMGRAPH_FORCE_DEVICE=0.
"""
import json
import multiprocessing as mp
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from engine_driver import base_config, record_batch  # noqa: E402


def run_sampler(sam, w, barrier, out_prefix, exit_now):
    sam.sample_init(w, f"cuda:{w}")
    barrier.wait()
    if exit_now:
        sys.exit(0)
    num_epoch, num_local = sam.num_epoch(), sam.num_local_step()
    for _ in range(num_epoch * num_local):
        sam.sample_once()
    items = {n: [sam.get_log_epoch_value(e, getattr(sam, n)) for e in range(num_epoch)]
             for n in ("kLogEpochSampleTime", "KLogEpochSampleGetCacheMissIndexTime", "kLogEpochSampleSendTime",
                       "kLogEpochSampleTotalTime")}
    with open(f"{out_prefix}.s{w}.json", "w") as f:
        json.dump({"num_local_step": num_local, "steps_per_epoch": sam.steps_per_epoch(), "epoch_items": items}, f)
    sam.shutdown()


def run_trainer(sam, w, S, T, barrier, num_layers, out_prefix, mode, record_batch):
    import torch
    barrier.wait()
    sam.train_init(w, f"cuda:{S + w}")
    num_epoch, num_step = sam.num_epoch(), sam.steps_per_epoch()
    batches, info = {}, {"keys": [], "devices": [], "steps": [], "num_local_step": sam.num_local_step()}
    for epoch in range(num_epoch):
        mine = list(range(w, num_step, T))  # train_graphsage.py: steps w, w + T, ... below num_step
        if mode == "start":
            sam.extract_start(len(mine))
        for _ in mine:
            if mode == "step":
                sam.sample_once()
            key = sam.get_next_batch()
            rec, devices = record_batch(sam, key, num_layers)
            for k, v in rec.items():
                batches[f"{key}:{k}"] = v
            info["keys"].append(int(key))
            info["devices"].append(sorted(devices))
            info["steps"].append({n: sam.get_log_step_value_by_key(key, getattr(sam, n))
                                  for n in ("kLogL1RecvTime", "kLogL1CopyTime", "kLogL2GraphCopyTime",
                                            "kLogL1GraphBytes", "kLogL1FeatureBytes")})
    info["epoch_items"] = {n: [sam.get_log_epoch_value(e, getattr(sam, n)) for e in range(num_epoch)]
                           for n in ("kLogEpochCopyTime", "kLogEpochFeatureBytes", "kLogEpochMissBytes")}
    torch.cuda.synchronize()
    np.savez(f"{out_prefix}.t{w}.npz", **batches)
    with open(f"{out_prefix}.t{w}.json", "w") as f:
        json.dump(info, f)
    sam.shutdown()


def main(record_batch=record_batch):
    """record_batch(sam, key, num_layers) -> (the batch's .npz entries, the devices of its tensors)."""
    dataset, out_prefix, S, T, mode = sys.argv[1], sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), sys.argv[5]
    assert mode in ("step", "start"), mode
    extra = dict(a.split("=", 1) for a in sys.argv[6:])
    import samgraph.torch as sam
    exit_sampler = int(extra.pop("exit_sampler", -1))
    barrier_timeout = float(extra.pop("barrier_timeout", 300))
    # the keys and defaults of tests/engine_driver.py
    cfg = base_config(sam, dataset, "arch5", {"num_sample_worker": S, "num_train_worker": T, "have_switcher": 0, **extra})
    num_layers = cfg["num_layer"]
    sam.config(cfg)
    sam.data_init()  # host only: the GPU is first touched in the children
    barrier = mp.get_context("fork").Barrier(S + T, timeout=barrier_timeout)
    pids = []
    for role, w in [("s", w) for w in range(S)] + [("t", w) for w in range(T)]:
        pid = os.fork()
        if pid == 0:
            code = 0
            try:
                if role == "s":
                    run_sampler(sam, w, barrier, out_prefix, w == exit_sampler)
                else:
                    run_trainer(sam, w, S, T, barrier, num_layers, out_prefix, mode, record_batch)
            except SystemExit as e:
                code = e.code or 0
            except BaseException as e:  # noqa: BLE001
                print(f"{'sampler' if role == 's' else 'trainer'} {w} failed:", repr(e), file=sys.stderr)
                code = 1
            sys.stdout.flush()
            sys.stderr.flush()
            os._exit(code)
        pids.append(pid)
    bad = 0
    for _ in pids:
        bad += sam.wait_one_child()
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
