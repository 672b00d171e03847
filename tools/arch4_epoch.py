"""arch4 (early prefetch, dynamic_cache) against arch3 with cache 0: step time and what the prefetch costs and buys.
Nothing here is part of bench.py.  Run on the GPU box; one JSON line per run.

    python tools/arch4_epoch.py epochs --preset products [--scale 1.0] --fanout 10 5 [--epochs 3] [--two-gpus]
        builds a datagen graph of the preset's shape (--scale shrinks its node count), then per setup -- arch3 cache 0,
        arch4, arch4 + dynamic_cache -- one child process on one forced GPU (SAMGRAPH_FORCE_DEVICE=0; --two-gpus adds
        the same on cuda:1 -> cuda:0 where two GPUs are visible).  Per run: ms/step over every epoch but the first,
        input rows per step (arch4: the superset) and their ratio to arch3's, kLogL1PrefetchAdvanced,
        kLogL1GetNeighbourTime, dynamic_cache's hit rate and the miss bytes per step.  Every row is read from pinned
        host memory (SAMGRAPH_FILL_FAKE_FEAT=1: a filled stand-in feature table, not one shared zero page).
    python tools/arch4_epoch.py child <dataset> <arch3|arch4|arch4_dynamic> --fanout ... (one run, used by `epochs`)
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child(a):
    import samgraph.torch as sam
    arch = "arch4" if a.setup.startswith("arch4") else "arch3"
    cfg = {"dataset_path": a.dataset, "_arch": sam.builtin_archs[arch]["arch"], "_sample_type": sam.sample_types["khop0"],
           "batch_size": a.batch_size, "num_epoch": a.epochs,
           "_cache_policy": sam.cache_policies["dynamic_cache" if a.setup == "arch4_dynamic" else "degree"],
           "cache_percentage": 0.0, "max_sampling_jobs": 10, "max_copying_jobs": 1, "omp_thread_num": 16,
           "num_layer": len(a.fanout), "num_hidden": 256, "lr": 0.003, "dropout": 0.5, "num_fanout": len(a.fanout),
           "fanout": a.fanout, "sampler_ctx": "cuda:1", "trainer_ctx": "cuda:0", "seed": 1}
    sam.config(cfg)
    sam.init()
    steps = sam.steps_per_epoch()
    keys, wall = [], 0.0
    for e in range(a.epochs):  # the first epoch warms up
        t0 = time.perf_counter()
        for _ in range(steps):
            sam.sample_once()
            key = sam.get_next_batch()
            if e:
                keys.append(key)
        if e:
            wall += time.perf_counter() - t0
    item = lambda k: sum(sam.get_log_step_value_by_key(key, k) for key in keys) / len(keys)  # noqa: E731
    rows, miss_b, feat_b = item(sam.kLogL1NumNode), item(sam.kLogL1MissBytes), item(sam.kLogL1FeatureBytes)
    res = {"setup": a.setup, "steps": len(keys), "ms_per_step": wall / len(keys) * 1e3, "rows_per_step": rows,
           "gather_us_per_step": item(sam.kLogL1CopyTime) * 1e6, "sample_us_per_step": item(sam.kLogL1SampleTime) * 1e6,
           "miss_MB_per_step": miss_b / 1e6, "feature_MB_per_step": feat_b / 1e6}
    if arch == "arch4":
        res["prefetch_advanced_us"] = item(sam.kLogL1PrefetchAdvanced) * 1e6
        res["get_neighbour_us"] = item(sam.kLogL1GetNeighbourTime) * 1e6
        res["hit_rate"] = 1.0 - miss_b / feat_b if feat_b else 0.0
    sam.shutdown()
    print(json.dumps(res), flush=True)


def epochs(a):
    import tempfile
    import torch
    from xgnn_amd import datagen
    preset = dict(datagen.PRESETS[a.preset])
    preset["num_node"] = int(preset["num_node"] * a.scale)
    g = datagen.make_graph(preset, seed=42)
    base = "/dev/shm" if os.path.isdir("/dev/shm") else None
    d = tempfile.mkdtemp(prefix="arch4_ds_", dir=base)
    try:
        datagen.write_dataset(d, g, minimal=True)
        del g
        places = [True] + ([False] if a.two_gpus and torch.cuda.device_count() >= 2 else [])
        arch3_rows = {}
        for forced in places:
            for setup in ("arch3", "arch4", "arch4_dynamic"):
                env = dict(os.environ, SAMGRAPH_FILL_FAKE_FEAT="1")
                env.pop("SAMGRAPH_FORCE_DEVICE", None)
                if forced:
                    env["SAMGRAPH_FORCE_DEVICE"] = "0"
                cmd = [sys.executable, os.path.abspath(__file__), "child", d, setup, "--batch-size", str(a.batch_size),
                       "--epochs", str(a.epochs), "--fanout"] + [str(f) for f in a.fanout]
                p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout, env=env)
                lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
                rec = {"preset": a.preset, "scale": a.scale, "num_node": preset["num_node"], "fanout": a.fanout,
                       "batch_size": a.batch_size, "forced_one_gpu": forced}
                if p.returncode != 0 or not lines:
                    rec.update(setup=setup, error=p.stderr[-800:])
                    print(json.dumps(rec), flush=True)
                    return 1
                rec.update(json.loads(lines[-1]))
                if setup == "arch3":
                    arch3_rows[forced] = rec["rows_per_step"]
                rec["rows_over_arch3"] = rec["rows_per_step"] / arch3_rows[forced]
                print(json.dumps(rec), flush=True)
    finally:
        import shutil
        shutil.rmtree(d, ignore_errors=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    e = sub.add_parser("epochs")
    e.add_argument("--preset", default="products")
    e.add_argument("--scale", type=float, default=1.0, help="fraction of the preset's node count")
    e.add_argument("--fanout", type=int, nargs="+", default=[10, 5])
    e.add_argument("--batch-size", type=int, default=8000)
    e.add_argument("--epochs", type=int, default=3, help="per run; the first warms up")
    e.add_argument("--two-gpus", action="store_true")
    e.add_argument("--timeout", type=float, default=600)
    c = sub.add_parser("child")
    c.add_argument("dataset")
    c.add_argument("setup", choices=["arch3", "arch4", "arch4_dynamic"])
    c.add_argument("--fanout", type=int, nargs="+", required=True)
    c.add_argument("--batch-size", type=int, default=8000)
    c.add_argument("--epochs", type=int, default=3)
    a = ap.parse_args()
    return epochs(a) if a.cmd == "epochs" else child(a)


if __name__ == "__main__":
    sys.exit(main() or 0)
