"""arch5 (sampler processes + trainer processes joined by the batch queue) measurements: the pack and unpack rates of a
queue slot and the per-step time against arch1.  Nothing here is part of bench.py.  Run on the GPU box; every number is
printed as one JSON line.

    python tools/arch5_epoch.py rate [--preset-bounds 8000 25 10] [--fill 1.0 0.5] [--reps 20] [--rounds 3]
        One slot of registered (mapped) host memory sized for batch 8000, fanout [25, 10].  ggms_queue_pack (the
        sampler GPU's stores into the slot, zero-copy) against hipMemcpyAsync D2H of the slot's bound size, and
        ggms_queue_unpack (the trainer GPU's loads from the slot) against hipMemcpyAsync H2D of the bound size,
        alternating, on cuda:0.  --fill: the fraction of every bound the batch uses (1.0: the same bytes as the DMA).
    python tools/arch5_epoch.py epochs --preset products --fanout 25 10 [--epochs 4] [--layouts 1x1 2x2 2x1]
        arch1, then arch5 with S samplers x T trainers, on one forced GPU (SAMGRAPH_FORCE_DEVICE=0), cache_percentage
        1.0, batch 8000; trainers call extract_start(count) per epoch and get_next_batch per step.  ms/step = wall
        time of every epoch but the first (first trainer start -> last trainer end) / its steps.  On one GPU the
        samplers and trainers share the device: these are plumbing numbers, not scaling numbers.
"""
import argparse
import ctypes as C
import json
import multiprocessing as mp
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def rate(a):
    import mmap
    import numpy as np
    import torch
    from xgnn_amd import _lib, ops
    torch.cuda.init()
    hip = C.CDLL("libamdhip64.so")
    lib = _lib.lib()
    bs, fan = a.preset_bounds[0], a.preset_bounds[1:]
    L = len(fan)
    max_seeds = int(bs * 1.25) + 1
    mi, me, mu = (C.c_size_t * L)(), (C.c_size_t * L)(), C.c_size_t()
    _lib.check(lib.ggms_sample_batch_capacity(max_seeds, (C.c_size_t * L)(*fan), L, mi, me, C.byref(mu)), "capacity")
    lay = ops.queue_layout(list(me), mu.value, max_seeds)
    size = lay.slot_bytes
    mm, mm_dma = mmap.mmap(-1, size), mmap.mmap(-1, size)  # the slot; the DMA copies' host side (keeps the slot intact)
    addr, addr_dma = C.addressof(C.c_char.from_buffer(mm)), C.addressof(C.c_char.from_buffer(mm_dma))
    for x in (addr, addr_dma):
        assert hip.hipHostRegister(C.c_void_p(x), C.c_size_t(size), C.c_uint(2)) == 0
    dptr = C.c_void_p()
    assert hip.hipHostGetDevicePointer(C.byref(dptr), C.c_void_p(addr), C.c_uint(0)) == 0
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    rows = [torch.randint(0, 1 << 30, (me[i],), dtype=torch.int32, device=dev) for i in range(L)]
    cols = [torch.randint(0, 1 << 30, (me[i],), dtype=torch.int32, device=dev) for i in range(L)]
    inp = torch.randint(0, 1 << 30, (mu.value,), dtype=torch.int32, device=dev)
    outn = torch.randint(0, 1 << 30, (max_seeds,), dtype=torch.int32, device=dev)
    drows = [torch.empty_like(r) for r in rows]
    dcols = [torch.empty_like(c) for c in cols]
    dinp, doutn = torch.empty_like(inp), torch.empty_like(outn)
    devbuf = torch.empty(size, dtype=torch.uint8, device=dev)
    out = {"what": "arch5 queue slot: pack / unpack vs a DMA copy of the bound size", "batch_size": bs, "fanout": fan,
           "slot_bytes": size, "reps": a.reps, "rounds": a.rounds, "results": []}

    def timed(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(3):
            fn()
        t0.record(stream)
        for _ in range(a.reps):
            fn()
        t1.record(stream)
        t1.synchronize()
        return t0.elapsed_time(t1) * 1e-3 / a.reps  # s per call

    s = C.c_void_p(stream.cuda_stream)
    for fill in a.fill:
        counts = np.zeros(_lib.COUNTS_WORDS(L), np.int64)
        for i in range(L):
            counts[_lib.COUNT_EDGES(i)] = int(me[i] * fill)
        counts[_lib.COUNT_INPUT(L)] = int(mu.value * fill)
        n_out = int(max_seeds * fill)
        counts_dev = torch.from_numpy(counts).to(dev)
        dcounts = torch.empty_like(counts_dev)
        moved = (sum(2 * counts[_lib.COUNT_EDGES(i)] for i in range(L)) + counts[_lib.COUNT_INPUT(L)] + n_out) * 4 + 8 * counts.size

        def pack():
            ops.queue_pack(dptr.value, lay, rows, cols, [None] * L, inp, outn, counts_dev, 1, n_out)

        def unpack():
            ops.queue_unpack(dptr.value, lay, drows, dcols, [None] * L, dinp, doutn, dcounts)

        def d2h():
            assert hip.hipMemcpyAsync(C.c_void_p(addr_dma), C.c_void_p(devbuf.data_ptr()), C.c_size_t(size), 2, s) == 0

        def h2d():
            assert hip.hipMemcpyAsync(C.c_void_p(devbuf.data_ptr()), C.c_void_p(addr_dma), C.c_size_t(size), 1, s) == 0

        t = {"pack": [], "dma_d2h_bound": [], "unpack": [], "dma_h2d_bound": []}
        pack()  # the slot's header holds this fill's lengths from here on (the unpack reads them)
        for _ in range(a.rounds):
            t["pack"].append(timed(pack))
            t["dma_d2h_bound"].append(timed(d2h))
            t["unpack"].append(timed(unpack))
            t["dma_h2d_bound"].append(timed(h2d))
        dinp.zero_()
        unpack()
        torch.cuda.synchronize()
        n_in, e_last = int(counts[_lib.COUNT_INPUT(L)]), counts[_lib.COUNT_EDGES(L - 1)]
        assert torch.equal(dinp[:n_in], inp[:n_in]) and torch.equal(drows[-1][:e_last], rows[-1][:e_last])
        med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
        out["results"].append({
            "fill": fill, "bytes_moved": int(moved),
            "us": {k: v * 1e6 for k, v in med.items()},
            "GBps": {"pack": moved / med["pack"] / 1e9, "unpack": moved / med["unpack"] / 1e9,
                     "dma_d2h_bound": size / med["dma_d2h_bound"] / 1e9, "dma_h2d_bound": size / med["dma_h2d_bound"] / 1e9},
            "pack_over_dma_time": med["pack"] / med["dma_d2h_bound"],
            "unpack_over_dma_time": med["unpack"] / med["dma_h2d_bound"]})
    torch.cuda.synchronize()
    for x in (addr, addr_dma):
        assert hip.hipHostUnregister(C.c_void_p(x)) == 0
    print(json.dumps(out), flush=True)


def _config(sam, a, dataset, arch, S=0, T=0):
    cfg = {"dataset_path": dataset, "_arch": sam.builtin_archs[arch]["arch"], "_sample_type": sam.sample_types["khop3"],
           "batch_size": a.batch_size, "num_epoch": a.epochs, "_cache_policy": sam.cache_policies["degree"],
           "cache_percentage": 1.0, "max_sampling_jobs": 10, "max_copying_jobs": 1, "omp_thread_num": 16,
           "num_layer": len(a.fanout), "num_hidden": 256, "lr": 0.003, "dropout": 0.5, "num_fanout": len(a.fanout),
           "fanout": a.fanout, "seed": 1}
    if arch == "arch1":
        cfg.update(sampler_ctx="cuda:0", trainer_ctx="cuda:0")
    else:
        cfg.update(num_sample_worker=S, num_train_worker=T, have_switcher=0)
    return cfg


def child_arch1(a, dataset):
    import samgraph.torch as sam
    sam.config(_config(sam, a, dataset, "arch1"))
    sam.init()
    steps = sam.steps_per_epoch()
    wall = 0.0
    for e in range(a.epochs):
        t0 = time.perf_counter()
        for _ in range(steps):
            sam.sample_once()
            sam.get_next_batch()
        if e:
            wall += time.perf_counter() - t0
    sam.shutdown()
    return {"arch": "arch1", "steps": steps * (a.epochs - 1), "ms_per_step": wall / (steps * (a.epochs - 1)) * 1e3}


def child_arch5(a, dataset, S, T):
    import samgraph.torch as sam
    sam.config(_config(sam, a, dataset, "arch5", S, T))
    sam.data_init()
    barrier = mp.get_context("fork").Barrier(S + T, timeout=600)
    rq, wq = os.pipe()
    pids = []
    for role, w in [("s", w) for w in range(S)] + [("t", w) for w in range(T)]:
        pid = os.fork()
        if pid == 0:
            code = 0
            try:
                if role == "s":
                    sam.sample_init(w, f"cuda:{w}")
                    barrier.wait()
                    for _ in range(sam.num_epoch() * sam.num_local_step()):
                        sam.sample_once()
                    rec = {"role": "s", "send_s": sum(sam.get_log_epoch_value(e, sam.kLogEpochSampleSendTime)
                                                      for e in range(1, a.epochs))}
                else:
                    barrier.wait()
                    sam.train_init(w, f"cuda:{S + w}")
                    steps = sam.steps_per_epoch()
                    t_start = t_end = 0.0
                    for e in range(a.epochs):
                        if e == 1:
                            t_start = time.monotonic()
                        mine = range(w, steps, T)
                        sam.extract_start(len(mine))
                        for _ in mine:
                            sam.get_next_batch()
                    t_end = time.monotonic()
                    rec = {"role": "t", "t_start": t_start, "t_end": t_end, "steps": steps,
                           "unpack_s": sum(sam.get_log_epoch_value(e, sam.kLogEpochCopyTime) for e in range(1, a.epochs))}
                os.write(wq, (json.dumps(rec) + "\n").encode())
                sam.shutdown()
            except BaseException as e:  # noqa: BLE001
                print(f"{role}{w} failed:", repr(e), file=sys.stderr)
                code = 1
            os._exit(code)
        pids.append(pid)
    os.close(wq)
    bad = sum(sam.wait_one_child() for _ in pids)
    recs = [json.loads(l) for l in os.fdopen(rq).read().splitlines() if l]
    if bad:
        raise RuntimeError(f"arch5 S{S}T{T}: {bad} workers failed")
    tr = [r for r in recs if r["role"] == "t"]
    steps = tr[0]["steps"] * (a.epochs - 1)
    wall = max(r["t_end"] for r in tr) - min(r["t_start"] for r in tr)
    return {"arch": "arch5", "S": S, "T": T, "steps": steps, "ms_per_step": wall / steps * 1e3,
            "sampler_send_ms_per_step": sum(r["send_s"] for r in recs if r["role"] == "s") / steps * 1e3,
            "trainer_copy_ms_per_step": sum(r["unpack_s"] for r in tr) / steps * 1e3}


def child(a):
    res = child_arch1(a, a.dataset) if a.layout == "arch1" else child_arch5(a, a.dataset, *map(int, a.layout.split("x")))
    print(json.dumps(res), flush=True)


def epochs(a):
    from xgnn_amd import datagen
    g = datagen.make_graph(a.preset, seed=42)
    base = "/dev/shm" if os.path.isdir("/dev/shm") else None
    d = tempfile.mkdtemp(prefix="arch5_ds_", dir=base)
    try:
        datagen.write_dataset(d, g, minimal=True)  # no feat.bin: a zero-filled table of the preset's width
        del g
        out = {"what": "arch5 vs arch1 step time, one GPU (plumbing, not scaling: every process shares the device)",
               "preset": a.preset, "fanout": a.fanout, "batch_size": a.batch_size, "cache_percentage": 1.0,
               "loop": "arch1: sample_once + get_next_batch; arch5 trainers: extract_start(count) per epoch",
               "runs": []}
        for layout in ["arch1"] + a.layouts:
            cmd = [sys.executable, os.path.abspath(__file__), "child", d, layout, "--batch-size", str(a.batch_size),
                   "--epochs", str(a.epochs), "--fanout"] + [str(f) for f in a.fanout]
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout,
                               env=dict(os.environ, SAMGRAPH_FORCE_DEVICE="0"))
            lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
            if p.returncode != 0 or not lines:
                out["runs"].append({"layout": layout, "error": p.stderr[-800:]})
                print(json.dumps(out), flush=True)
                return 1
            out["runs"].append(json.loads(lines[-1]))
        a1 = out["runs"][0]["ms_per_step"]
        out["over_arch1"] = {f"S{r['S']}T{r['T']}": r["ms_per_step"] / a1 for r in out["runs"][1:]}
        print(json.dumps(out), flush=True)
    finally:
        import shutil
        shutil.rmtree(d, ignore_errors=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    r = sub.add_parser("rate")
    r.add_argument("--preset-bounds", type=int, nargs="+", default=[8000, 25, 10], help="batch size, then the fanout")
    r.add_argument("--fill", type=float, nargs="+", default=[1.0, 0.5])
    r.add_argument("--reps", type=int, default=20)
    r.add_argument("--rounds", type=int, default=3)
    e = sub.add_parser("epochs")
    e.add_argument("--preset", default="products")
    e.add_argument("--fanout", type=int, nargs="+", default=[25, 10])
    e.add_argument("--batch-size", type=int, default=8000)
    e.add_argument("--epochs", type=int, default=4, help="per run; the first warms up")
    e.add_argument("--layouts", nargs="+", default=["1x1", "2x2", "2x1"])
    e.add_argument("--timeout", type=float, default=900)
    c = sub.add_parser("child")
    c.add_argument("dataset")
    c.add_argument("layout", help="arch1, or SxT for arch5")
    c.add_argument("--fanout", type=int, nargs="+", required=True)
    c.add_argument("--batch-size", type=int, default=8000)
    c.add_argument("--epochs", type=int, default=4)
    a = ap.parse_args()
    return {"rate": rate, "epochs": epochs, "child": child}[a.cmd](a) or 0


if __name__ == "__main__":
    sys.exit(main())
