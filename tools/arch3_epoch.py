"""arch3 (sampler GPU + trainer GPU) measurements: the batch hand-off's copy rate and the engine's step time against
arch1.  Nothing here is part of bench.py.  Run on the GPU box; every number below is printed as one JSON line.

    python tools/arch3_epoch.py rate  [--mb 32 64 256] [--reps 20] [--rounds 3]
        ggms_batch_handoff (one segment, and the same bytes as 12 segments) against hipMemcpyAsync D2D
        (ggms_link_probe_copy with_kernel=0) for the same bytes, alternating, on cuda:0; with two GPUs visible also
        cuda:0 -> cuda:1 (peer reads over xGMI) against the same probe across the pair.
    python tools/arch3_epoch.py epochs --preset products --fanout 25 10 [--epochs 6] [--rounds 2] [--two-gpus]
                                       [--rocprof-dir DIR]
        arch1 and arch3 on one forced GPU (SAMGRAPH_FORCE_DEVICE=0), cache_percentage 1.0, batch 8000, alternating child
        processes; ms/step over every epoch but the first, and the hand-off's own time per step (kLogL2GraphCopyTime,
        from the launch timer on its dispatch).  --two-gpus adds arch3 on cuda:0 -> cuda:1 without the force.
        --rocprof-dir: afterwards one more forced child of each arch under `rocprofv3 --kernel-trace --stats` (runs of
        their own, traces in DIR/arch1 and DIR/arch3).
    python tools/arch3_epoch.py child <dataset> <arch1|arch3> --fanout ... (one run, used by `epochs`)
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _enable_peer(dev, peer):
    """hipDeviceEnablePeerAccess(peer) from `dev` (what the engine does at init for arch3)."""
    hip = C.CDLL("libamdhip64.so")
    hip.hipSetDevice(dev)
    rc = hip.hipDeviceEnablePeerAccess(peer, 0)
    return rc in (0, 704)  # hipSuccess, hipErrorPeerAccessAlreadyEnabled


def rate(a):
    import torch
    from xgnn_amd import _lib, ops
    lib = _lib.lib()
    pairs = [(0, 0)]
    if torch.cuda.device_count() >= 2 and _enable_peer(1, 0):
        pairs.append((0, 1))
    out = {"what": "hand-off rate", "reps": a.reps, "rounds": a.rounds, "results": []}
    for sdev, ddev in pairs:
        for mb in a.mb:
            n = mb << 20
            src = torch.randint(0, 1 << 30, (n // 4,), dtype=torch.int32, device=f"cuda:{sdev}")
            dst = torch.empty(n // 4, dtype=torch.int32, device=f"cuda:{ddev}")
            torch.cuda.set_device(ddev)
            stream = torch.cuda.current_stream(ddev)
            per = (n // 4 // 12) & ~3  # elements per piece: every piece starts 16-B aligned
            pieces = [(src[k * per:(k + 1) * per], dst[k * per:(k + 1) * per], per) for k in range(12)]

            def handoff(segs):
                nbytes = sum(s[2] for s in segs) * 4
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                for _ in range(3):
                    ops.batch_handoff(segs)
                t0.record(stream)
                for _ in range(a.reps):
                    ops.batch_handoff(segs)
                t1.record(stream)
                t1.synchronize()
                return nbytes * a.reps / (t0.elapsed_time(t1) * 1e-3) / 1e9

            def memcpy():
                g = C.c_double(0)
                _lib.check(lib.ggms_link_probe_copy(C.c_void_p(dst.data_ptr()), C.c_void_p(src.data_ptr()), n, a.reps, 0,
                                                    C.byref(g), C.c_void_p(stream.cuda_stream)), "ggms_link_probe_copy")
                return g.value

            rows = {"handoff_1seg": [], "handoff_12seg": [], "memcpy": []}
            for _ in range(a.rounds):  # alternating: every round runs each variant once
                rows["handoff_1seg"].append(handoff([(src, dst, n // 4)]))
                rows["memcpy"].append(memcpy())
                rows["handoff_12seg"].append(handoff(pieces))
            assert torch.equal(dst.cpu(), src.cpu())
            med = {k: sorted(v)[len(v) // 2] for k, v in rows.items()}
            out["results"].append({"src": f"cuda:{sdev}", "dst": f"cuda:{ddev}", "MB": mb, "GBps": rows,
                                   "median_GBps": med, "handoff_over_memcpy": med["handoff_1seg"] / med["memcpy"]})
            del src, dst, pieces
            torch.cuda.empty_cache()
    if len(pairs) == 1:
        out["two_gpus"] = "not measured on two GPUs (one device visible)"
    print(json.dumps(out), flush=True)


def child(a):
    import samgraph.torch as sam
    cfg = {"dataset_path": a.dataset, "_arch": sam.builtin_archs[a.arch]["arch"], "_sample_type": sam.sample_types["khop3"],
           "batch_size": a.batch_size, "num_epoch": a.epochs, "_cache_policy": sam.cache_policies["degree"],
           "cache_percentage": 1.0, "max_sampling_jobs": 10, "max_copying_jobs": 1, "omp_thread_num": 16,
           "num_layer": len(a.fanout), "num_hidden": 256, "lr": 0.003, "dropout": 0.5, "num_fanout": len(a.fanout),
           "fanout": a.fanout, "sampler_ctx": "cuda:0", "trainer_ctx": "cuda:1" if a.arch == "arch3" else "cuda:0",
           "seed": 1}
    sam.config(cfg)
    sam.init()
    steps = sam.steps_per_epoch()
    keys, wall, edges = [], 0.0, 0.0
    for e in range(a.epochs):  # the first epoch warms up; the others are reported
        t0 = time.perf_counter()
        for _ in range(steps):
            sam.sample_once()
            key = sam.get_next_batch()
            if e:
                keys.append(key)
        if e:
            wall += time.perf_counter() - t0
            edges += sam.get_log_epoch_value(e, sam.kLogEpochNumSample)
    item = lambda k: sum(sam.get_log_step_value_by_key(key, k) for key in keys) / len(keys)  # noqa: E731
    res = {"arch": a.arch, "steps": len(keys), "ms_per_step": wall / len(keys) * 1e3,
           "handoff_us_per_step": item(sam.kLogL2GraphCopyTime) * 1e6,
           "handoff_MB_per_step": (item(sam.kLogL1GraphBytes) + item(sam.kLogL1IdBytes)) / 1e6,
           "gather_us_per_step": item(sam.kLogL1CopyTime) * 1e6, "edges_per_step": edges / len(keys)}
    sam.shutdown()
    print(json.dumps(res), flush=True)


def epochs(a):
    import tempfile
    from xgnn_amd import datagen
    g = datagen.make_graph(a.preset, seed=42)
    base = "/dev/shm" if os.path.isdir("/dev/shm") else None
    d = tempfile.mkdtemp(prefix="arch3_ds_", dir=base)
    try:
        datagen.write_dataset(d, g, minimal=True)  # no feat.bin: a zero-filled table of the preset's width
        del g
        runs = [("arch1", True), ("arch3", True)] + ([("arch3", False)] if a.two_gpus else [])
        out = {"what": "arch3 vs arch1 step time", "preset": a.preset, "fanout": a.fanout, "batch_size": a.batch_size,
               "cache_percentage": 1.0, "loop": "sample_once + get_next_batch", "runs": []}
        for r in range(a.rounds):
            for arch, forced in runs:
                env = dict(os.environ)
                env.pop("SAMGRAPH_FORCE_DEVICE", None)
                if forced:
                    env["SAMGRAPH_FORCE_DEVICE"] = "0"
                cmd = [sys.executable, os.path.abspath(__file__), "child", d, arch, "--batch-size", str(a.batch_size),
                       "--epochs", str(a.epochs), "--fanout"] + [str(f) for f in a.fanout]
                p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout, env=env)
                lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
                if p.returncode != 0 or not lines:
                    out["runs"].append({"arch": arch, "forced": forced, "round": r, "error": p.stderr[-800:]})
                    print(json.dumps(out), flush=True)
                    return 1
                rec = json.loads(lines[-1])
                rec.update(forced=forced, round=r)
                out["runs"].append(rec)
        ms = lambda arch, forced: sorted(x["ms_per_step"] for x in out["runs"] if x["arch"] == arch and x["forced"] == forced)  # noqa: E731
        a1, a3 = ms("arch1", True), ms("arch3", True)
        out["median_ms_per_step"] = {"arch1": a1[len(a1) // 2], "arch3_forced": a3[len(a3) // 2]}
        out["arch3_over_arch1"] = a3[len(a3) // 2] / a1[len(a1) // 2]
        if not a.two_gpus:
            out["two_gpus"] = "not measured on two GPUs"
        if a.rocprof_dir:  # kernel times in runs of their own (tracing slows the host): one forced child per arch
            out["rocprof"] = {}
            for arch in ("arch1", "arch3"):
                cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d",
                       os.path.join(a.rocprof_dir, arch), "--", sys.executable, os.path.abspath(__file__), "child", d,
                       arch, "--batch-size", str(a.batch_size), "--epochs", str(a.epochs), "--fanout"]
                cmd += [str(f) for f in a.fanout]
                p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout,
                                   env=dict(os.environ, SAMGRAPH_FORCE_DEVICE="0"))
                out["rocprof"][arch] = {"cmd": f"rocprofv3 --kernel-trace --stats --output-format csv -d <dir>/{arch} -- "
                                               f"python tools/arch3_epoch.py child <dataset> {arch} ...", "rc": p.returncode}
        print(json.dumps(out), flush=True)
    finally:
        import shutil
        shutil.rmtree(d, ignore_errors=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    r = sub.add_parser("rate")
    r.add_argument("--mb", type=int, nargs="+", default=[32, 64, 256])
    r.add_argument("--reps", type=int, default=20)
    r.add_argument("--rounds", type=int, default=3)
    e = sub.add_parser("epochs")
    e.add_argument("--preset", default="products")
    e.add_argument("--fanout", type=int, nargs="+", default=[25, 10])
    e.add_argument("--batch-size", type=int, default=8000)
    e.add_argument("--rounds", type=int, default=2)
    e.add_argument("--epochs", type=int, default=6, help="per run; the first warms up")
    e.add_argument("--rocprof-dir", default=None)
    e.add_argument("--two-gpus", action="store_true")
    e.add_argument("--timeout", type=float, default=900)
    c = sub.add_parser("child")
    c.add_argument("dataset")
    c.add_argument("arch", choices=["arch1", "arch3"])
    c.add_argument("--fanout", type=int, nargs="+", required=True)
    c.add_argument("--batch-size", type=int, default=8000)
    c.add_argument("--epochs", type=int, default=6)
    a = ap.parse_args()
    return {"rate": rate, "epochs": epochs, "child": child}[a.cmd](a) or 0


if __name__ == "__main__":
    sys.exit(main())
