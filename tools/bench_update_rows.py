"""The learnable feature table, timed on one GPU: ggms_update_rows beside the plain gather, and the arch1 step with and
without the config key feat_learnable.

    python tools/bench_update_rows.py --kernel [--out profiles/update_rows.txt]
    python tools/bench_update_rows.py --engine 3 [--parent-root DIR]

--kernel: products- and papers100M-shaped input sets (bench_extract.py's: 1.28 M of 2.45 M rows at dim 100, 2.96 M of
16 M rows at dim 128; distinct rows, as a batch's input nodes are).  Each case is ONE launch on the same node list --
the plain gather (ggms_extract), the SGD update, the Adagrad update -- 5 rounds x 20 launches in alternating order
between two events, median of the rounds.  Bytes per second are over the ALGORITHMIC bytes per row: 4 + 2 x dim x 4 for
the gather, 4 + 3 x dim x 4 for SGD, 4 + 5 x dim x 4 for Adagrad.  The yardstick is the gather's own rate in the same
process.
--engine R: the arch1 step (khop3, products, batch 8000, fanout 25 10; a table without feat.bin, zero-filled) through
samgraph.torch, each configuration in a child process, R runs each in alternating order: `plain` (no key),
`plain_one_stream` (no key, extract_streams = 1: what the forced single extract stream costs by itself) and `learn_sgd`
(feat_learnable = sgd, update_graph_feat after every batch with a READY gradient tensor, so no trainer compute is in the
number).  Wall clock per step over all epochs but the first.  --parent-root: another checkout of the project (built),
whose engine runs `plain` too, as `parent_plain`.  One JSON line per configuration.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")

SHAPES = [("products", 2_449_029, 1_280_000, 100), ("papers100M", 16_000_000, 2_960_000, 128)]
CONFIGS = {"plain": {}, "plain_one_stream": {"extract_streams": 1}, "learn_sgd": {"feat_learnable": "sgd", "feat_lr": 0.01}}


def run_kernel(args):
    sys.path.insert(0, ROOT)
    import torch
    from xgnn_amd import ops
    dev = torch.device("cuda", 0)
    lines = [f"ggms_update_rows beside the plain gather: one launch per case on the same distinct node list, 5 rounds x 20 "
             f"launches in alternating order, median of the rounds (min .. max); device: {torch.cuda.get_device_name(0)}"]

    def timeit(fn, reps=20):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps * 1e3  # us

    for name, table_rows, rows, dim in SHAPES:
        torch.manual_seed(1)
        table = torch.randn(table_rows, dim, device=dev)
        state = torch.rand(table_rows, dim, device=dev)
        nodes = torch.randperm(table_rows, device=dev)[:rows].to(torch.int32)
        grad = torch.randn(rows, dim, device=dev)
        out = torch.empty(rows, dim, device=dev)
        cases = [("gather", 4 + 2 * dim * 4, lambda: ops.extract(table, nodes, out=out)),
                 ("sgd", 4 + 3 * dim * 4, lambda: ops.update_rows(table, nodes, grad, ops.UPDATE_SGD, 1e-3)),
                 ("adagrad", 4 + 5 * dim * 4, lambda: ops.update_rows(table, nodes, grad, ops.UPDATE_ADAGRAD, 1e-3, state=state))]
        times = {c[0]: [] for c in cases}
        for rnd in range(5):
            for case, _, fn in (cases if rnd % 2 == 0 else cases[::-1]):
                times[case].append(timeit(fn))
        rate = {}
        lines.append(f"{name}: {rows} of {table_rows} rows, dim {dim}")
        for case, row_bytes, _ in cases:
            v = sorted(times[case])
            rate[case] = rows * row_bytes / (v[len(v) // 2] * 1e-6)
            lines.append(f"  {case:8s} {v[len(v) // 2]:8.1f} us  ({v[0]:.1f} .. {v[-1]:.1f})  {row_bytes} B/row  "
                         f"{rate[case] / 1e12:.3f} TB/s" + ("" if case == "gather" else f"  = {rate[case] / rate['gather']:.3f} of the gather's rate"))
        del table, state, nodes, grad, out
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


def engine_child(args):
    sys.path.insert(0, args.root)
    import torch
    import samgraph.torch as sam
    keys = json.loads(args.child_keys)
    cfg = {"dataset_path": args.engine_child, "_arch": sam.builtin_archs["arch1"]["arch"],
           "_sample_type": sam.sample_types["khop3"], "batch_size": 8000, "num_epoch": args.epochs,
           "_cache_policy": sam.cache_policies["degree"], "cache_percentage": 0.0, "max_sampling_jobs": 10,
           "max_copying_jobs": 1, "omp_thread_num": 16, "num_layer": 2, "num_hidden": 256, "lr": 0.003, "dropout": 0.5,
           "num_fanout": 2, "fanout": [25, 10], "sampler_ctx": "cuda:0", "trainer_ctx": "cuda:0", "seed": 42}
    cfg.update(keys)
    sam.config(cfg)
    sam.init()
    learn = "feat_learnable" in keys
    grad = torch.full((8000 * (1 + 10 + 250), sam.feat_dim()), 1e-3, device="cuda") if learn else None  # the batch bound
    steps, wall, rows = sam.steps_per_epoch(), 0.0, 0
    for e in range(sam.num_epoch()):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            sam.sample_once()
            key = sam.get_next_batch()
            n = sam.get_graph_num_src(key, 0)
            if learn:
                sam.update_graph_feat(key, grad[:n])
            if e:
                rows += n
        torch.cuda.synchronize()
        if e:
            wall += time.perf_counter() - t0
    timed = steps * (sam.num_epoch() - 1)
    sam.shutdown()
    print(json.dumps(dict(steps=timed, ms_per_step=round(wall / timed * 1e3, 4), input_nodes_per_step=rows // timed)), flush=True)


def run_engine(args):
    import shutil
    import tempfile
    sys.path.insert(0, ROOT)
    from xgnn_amd import datagen
    g = datagen.make_graph("products", seed=42)
    base = "/dev/shm" if os.path.isdir("/dev/shm") and shutil.disk_usage("/dev/shm").free > 2 * g["indices"].nbytes else None
    d = tempfile.mkdtemp(prefix="ggms_bench_update_", dir=base)
    runs = [(name, os.path.abspath(ROOT), keys) for name, keys in CONFIGS.items()]
    if args.parent_root:
        runs.insert(0, ("parent_plain", os.path.abspath(args.parent_root), {}))
    rec = {name: [] for name, _, _ in runs}
    try:
        datagen.write_dataset(d, g, minimal=True)
        for rnd in range(args.engine):
            for name, root, keys in (runs if rnd % 2 == 0 else runs[::-1]):
                cmd = [sys.executable, os.path.abspath(__file__), "--engine-child", d + "/", "--root", root, "--child-keys",
                       json.dumps(keys), "--epochs", str(args.epochs)]
                r = subprocess.run(["timeout", "-k", "10", str(args.child_timeout)] + cmd, capture_output=True, text=True)
                lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
                rec[name].append(json.loads(lines[-1]) if r.returncode == 0 and lines else dict(error=r.stderr[-300:]))
                if r.returncode in (124, 134, 137, 139):  # a time limit or a crash: nothing more on this GPU
                    print(json.dumps(rec), flush=True)
                    sys.exit(r.returncode)
        for name, got in rec.items():
            ms = sorted(x["ms_per_step"] for x in got if "ms_per_step" in x)
            print(json.dumps(dict(config=name, ms_per_step=ms, runs=got)), flush=True)
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--engine", type=int, default=0, metavar="R", help="the arch1 step, R runs per configuration")
    ap.add_argument("--parent-root", help="--engine: a built checkout of another commit, timed as parent_plain")
    ap.add_argument("--epochs", type=int, default=8)
    ap.add_argument("--out", help="--kernel: also write the report to this file")
    ap.add_argument("--child-timeout", type=int, default=300)
    ap.add_argument("--engine-child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--root", default=os.path.abspath(ROOT), help=argparse.SUPPRESS)
    ap.add_argument("--child-keys", default="{}", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.engine_child:
        return engine_child(args)
    if args.kernel:
        run_kernel(args)
    if args.engine:
        run_engine(args)


if __name__ == "__main__":
    main()
