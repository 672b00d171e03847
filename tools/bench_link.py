"""Link-prediction seeds (ggms_link_seeds) and the arch1 link_prediction step, timed on one GPU.

    python tools/bench_link.py --graph products              # the leaf alone: B x K x mode, next to khop3's first layer
    python tools/bench_link.py --graph papers100M
    python tools/bench_link.py --graph hub                   # a 10^6-neighbour hub as the source of one positive
    python tools/bench_link.py --graph products --engine     # + the whole arch1 step through samgraph.torch
    python tools/bench_link.py --graph products --no-leaf --drop --engine --exclude-ab 3
                                                             # exclude_seed_edges: the filter alone, and the arch1 step
                                                             # with `both` next to `none`, alternating

Leaf: B positive edges drawn uniformly from the graph's edges, K negatives each, both modes; the launch is issued
`--steps` times back to back between two events (buffers allocated once, the C entry point called directly), median
over `--rounds` rounds.  The yardstick in the same record is khop3's leaf launch sequence over the same B (2 + K)
endpoints with the first sampled layer's fanout (--fanout's last entry): what the batch's first layer costs for the seed
list this kernel produces.  Both figures include the host's issue time of their launches.
Engine (--engine): the graph is written in the on-disk format without feat.bin (zero-filled table) with a
train_edge_set.bin of 48 batches, and every configuration runs in a child process (the engine is a process-wide
singleton): two epochs, the second one's wall clock per step and the engine's own sampling time (kLogEpochSampleTime,
the sampling stream from the edge-id copy to the end of the batch).  The yardstick is the node_classification run with
batch_size = B (2 + K) node seeds.  One JSON line per record on stdout.
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

MODES = {"uniform": 0, "exclude": 1}


def make_graph(name, seed):
    from xgnn_amd import datagen
    if name != "hub":
        g = datagen.make_graph(name, seed=seed)
        return g
    rng = np.random.RandomState(seed)
    N = 1_000_000  # 1 M nodes of degree 50, node 0 with 10^6 neighbours (tools/bench_khop_labor.py's hub graph)
    deg = np.full(N, 50, np.int64)
    deg[0] = 1_000_000
    ip = np.zeros(N + 1, np.uint32)
    ip[1:] = np.cumsum(deg)
    ix = rng.randint(0, N, int(ip[-1])).astype(np.uint32)
    return dict(indptr=ip, indices=ix, train_set=rng.permutation(N)[: N // 10].astype(np.uint32),
                meta=dict(feat_dim=100, num_class=47))


def timed(fn, steps):
    import torch
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps * 1e3  # us


def leaf_records(args, g):
    import torch
    from xgnn_amd import ops
    from xgnn_amd._lib import check, lib
    dev = torch.device("cuda", 0)
    to_dev = lambda a: torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(dev)  # noqa: E731
    ip, ix = g["indptr"], g["indices"]
    E, N = int(ip[-1]), ip.size - 1
    graph = ops.DeviceGraph(to_dev(ip), to_dev(ix))
    fan = args.fanout[-1]
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rng = np.random.RandomState(args.seed)
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    cases = [(B, "") for B in args.batch]
    if args.graph == "hub":  # the same positives, one of them an edge of node 0's list
        cases = [(B, v) for B in args.batch for v in ("without_hub", "with_hub")]
    for B, variant in cases:
        eids = rng.randint(int(ip[1]) if args.graph == "hub" else 0, E, B).astype(np.uint32)
        if variant == "with_hub":
            eids[B // 2] = 123_456  # a position inside node 0's list
        t_eids = to_dev(eids)
        for K in args.num_negative:
            n = B * (2 + K)
            out = torch.empty(n, dtype=torch.int32, device=dev)
            forced = torch.zeros(1, dtype=torch.int64, device=dev)
            # the yardstick: khop3's leaf over the endpoint list
            nstates = max((n + 127) // 128 * 8, 8)
            states = ops.random_states(nstates, 7, dev)
            ws = torch.empty(lib().ggms_sample_workspace_bytes(ops.KHOP3, n, fan) // 4 + 16, dtype=torch.int32, device=dev)
            o_src = torch.empty(n * fan, dtype=torch.int32, device=dev)
            o_dst = torch.empty(n * fan, dtype=torch.int32, device=dev)
            num_out = torch.zeros(1, dtype=torch.int64, device=dev)

            def khop3():
                check(lib().ggms_sample_khop3(C.byref(graph.c), ptr(out), n, fan, ptr(o_src), ptr(o_dst), ptr(num_out),
                                              ptr(states), nstates, ptr(ws), ws.numel() * 4, stream), "khop3")

            rec = dict(graph=args.graph + ("/" + variant if variant else ""), num_node=N, num_edge=E, B=B, K=K,
                       endpoints=n, yardstick_fanout=fan, steps=args.steps, rounds=args.rounds)
            for mname in args.modes:
                mode = MODES[mname]

                def link():
                    check(lib().ggms_link_seeds(C.byref(graph.c), ptr(t_eids), B, K, mode, 99, ptr(out), ptr(forced),
                                                stream), "link_seeds")
                link()
                khop3()
                us = []
                for _ in range(args.rounds):
                    forced.zero_()
                    us.append((timed(link, args.steps), timed(khop3, args.steps)))
                med = np.median(np.array(us), axis=0)
                rec[mname] = dict(link_seeds_us=round(float(med[0]), 2), khop3_first_layer_us=round(float(med[1]), 2),
                                  forced_per_launch=int(forced.item()) // args.steps)
            assert ops.device_status() == 0
            print(json.dumps(rec), flush=True)


def drop_records(args, g):
    """ggms_drop_pair_edges alone: one khop3 batch over the endpoints of B positives (K negatives each, --fanout), its
    layers restored before every call, the call between two events of its own; median over --steps x --rounds calls.
    Next to the time: the bytes of row + col read and written once (16 per edge, what an in-place pass would move) and
    the bytes the snapshot scheme moves (32 per edge), each divided by the time."""
    import torch
    from xgnn_amd import ops
    from xgnn_amd._lib import COUNT_EDGES, check, lib
    dev = torch.device("cuda", 0)
    to_dev = lambda a: torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(dev)  # noqa: E731
    ip, ix = g["indptr"], g["indices"]
    E = int(ip[-1])
    graph = ops.DeviceGraph(to_dev(ip), to_dev(ix))
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    rng = np.random.RandomState(args.seed)
    L = len(args.fanout)
    for B in args.batch:
        eids = to_dev(rng.randint(0, E, B).astype(np.uint32))
        for K in args.num_negative:
            seeds, _ = ops.link_seeds(graph, eids, K, ops.NEG_EXCLUDE, 99)
            bs = ops.BatchSampler(graph, args.fanout, seeds.numel(), sample_type=ops.KHOP3, seed=7, device=dev)
            bs.sample(seeds.contiguous())
            bs.result()
            ids = bs.seed_ids().clone()
            counts0 = bs.counts.clone()
            n = [int(counts0[COUNT_EDGES(i)]) for i in range(L)]
            saved = [(bs.row[i][:n[i]].clone(), bs.col[i][:n[i]].clone()) for i in range(L)]
            me = (C.c_size_t * L)(*bs.max_edges)
            ws = torch.empty(lib().ggms_drop_pair_edges_workspace_bytes(B, me, L) // 4 + 4, dtype=torch.int32, device=dev)
            rows, cols = (C.c_void_p * L)(*[t.data_ptr() for t in bs.row]), (C.c_void_p * L)(*[t.data_ptr() for t in bs.col])
            dropped = torch.zeros(L, dtype=torch.int64, device=dev)
            rec = dict(graph=args.graph, B=B, K=K, fanouts=args.fanout, edges=n, steps=args.steps, rounds=args.rounds)
            for name, which in (("self", 1), ("both", 3)):
                us = []
                for _ in range(args.rounds):
                    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                           for _ in range(args.steps)]
                    for a, b in evs:
                        for i, (r, c) in enumerate(saved):
                            bs.row[i][:n[i]].copy_(r)
                            bs.col[i][:n[i]].copy_(c)
                        bs.counts.copy_(counts0)
                        dropped.zero_()
                        a.record()
                        check(lib().ggms_drop_pair_edges(ptr(ids), C.c_void_p(ids.data_ptr() + 4 * B), B, which, rows, cols,
                                                         me, L, ptr(bs.counts), ptr(dropped), ptr(ws), ws.numel() * 4,
                                                         stream), "drop_pair_edges")
                        b.record()
                    torch.cuda.synchronize()
                    us += [a.elapsed_time(b) * 1e3 for a, b in evs]
                t = float(np.median(us))
                rec[name] = dict(drop_us=round(t, 2), dropped=dropped.cpu().tolist(),
                                 once_GBps=round(16 * sum(n) / t * 1e-3, 1), moved_GBps=round(32 * sum(n) / t * 1e-3, 1))
            assert ops.device_status() == 0
            print(json.dumps(rec), flush=True)


def engine_child(a):
    import samgraph.torch as sam
    cfg = {"dataset_path": a.engine_child, "_arch": sam.builtin_archs["arch1"]["arch"],
           "_sample_type": sam.sample_types["khop3"], "batch_size": a.child_batch, "num_epoch": 2,
           "_cache_policy": sam.cache_policies["degree"], "cache_percentage": 1.0, "max_sampling_jobs": 10,
           "max_copying_jobs": 1, "omp_thread_num": 16, "num_layer": len(a.fanout), "num_hidden": 256, "lr": 0.003,
           "dropout": 0.5, "num_fanout": len(a.fanout), "fanout": a.fanout, "sampler_ctx": "cuda:0",
           "trainer_ctx": "cuda:0", "seed": a.seed}
    if a.child_task == "link_prediction":
        cfg.update(task="link_prediction", num_negative=a.child_k, negative_mode=a.child_mode)
        if a.child_exclude:
            cfg.update(exclude_seed_edges=a.child_exclude)
    sam.config(cfg)
    sam.init()
    steps = sam.steps_per_epoch()
    out = None
    for e in range(sam.num_epoch()):
        t0 = time.perf_counter()
        rows = excluded = 0
        for _ in range(steps):
            sam.sample_once()
            key = sam.get_next_batch()
            rows += sam.get_graph_num_src(key, 0)
            excluded += sam.get_graph_num_excluded(key)
        wall = time.perf_counter() - t0
        out = dict(steps=steps, ms_per_step=round(wall / steps * 1e3, 4), input_nodes_per_step=rows // steps,
                   excluded_per_step=excluded // steps,
                   sample_ms_per_step=round(sam.get_log_epoch_value(e, sam.kLogEpochSampleTime) / steps * 1e3, 4),
                   edges_per_step=int(sam.get_log_epoch_value(e, sam.kLogEpochNumSample) / steps))
    sam.shutdown()
    print(json.dumps(out), flush=True)


def engine_records(args, g):
    import shutil
    import tempfile
    from xgnn_amd import datagen
    E = int(g["indptr"][-1])
    base = "/dev/shm" if os.path.isdir("/dev/shm") and shutil.disk_usage("/dev/shm").free > 2 * g["indices"].nbytes else None
    d = tempfile.mkdtemp(prefix="ggms_bench_link_", dir=base)
    try:
        for B in args.batch:
            edges = np.random.RandomState(args.seed).randint(0, E, 48 * B).astype(np.uint32)
            datagen.write_dataset(d, g, minimal=True, train_edges=edges)
            for K in args.num_negative:
                # (task, batch, negative_mode, exclude_seed_edges, name); --exclude-ab R: the step with the filter (`both`)
                # next to the same step without it (`none`), R times each, alternating, instead of the runs above
                runs = [("link_prediction", B, m, "", m) for m in args.modes] + \
                       [("node_classification", B * (2 + K), "", "", f"node_classification_{B * (2 + K)}_seeds")]
                if args.exclude_ab:
                    runs = [("link_prediction", B, args.modes[-1], x, f"exclude_seed_edges_{x}")
                            for _ in range(args.exclude_ab) for x in ("none", "both")]
                rec = dict(graph=args.graph, B=B, K=K, fanouts=args.fanout)
                for task, batch, mode, exclude, name in runs:
                    cmd = [sys.executable, os.path.abspath(__file__), "--engine-child", d + "/", "--child-task", task,
                           "--child-batch", str(batch), "--child-k", str(K), "--child-mode", mode or "exclude",
                           "--child-exclude", exclude, "--seed", str(args.seed), "--fanout"] + [str(f) for f in args.fanout]
                    r = subprocess.run(["timeout", "-k", "10", str(args.child_timeout)] + cmd, capture_output=True, text=True)
                    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
                    got = json.loads(lines[-1]) if r.returncode == 0 and lines else dict(error=r.stderr[-300:])
                    if args.exclude_ab:
                        rec.setdefault(name, []).append(got)
                    else:
                        rec[name] = got
                    if r.returncode in (124, 134, 137, 139):  # a time limit or a crash: nothing more on this GPU
                        print(json.dumps(rec), flush=True)
                        sys.exit(r.returncode)
                print(json.dumps(rec), flush=True)
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graph", default="products", choices=["products", "papers100M", "hub", "tiny"])
    ap.add_argument("--batch", type=int, nargs="+", default=[1000, 8000], help="positive edges per batch")
    ap.add_argument("--num-negative", type=int, nargs="+", default=[1, 5])
    ap.add_argument("--modes", nargs="+", default=list(MODES), choices=list(MODES))
    ap.add_argument("--fanout", type=int, nargs="+", default=[25, 10])
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--engine", action="store_true", help="also the whole arch1 step, every configuration in a child")
    ap.add_argument("--no-leaf", action="store_true")
    ap.add_argument("--child-timeout", type=int, default=300)
    ap.add_argument("--engine-child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--child-task", default="link_prediction", help=argparse.SUPPRESS)
    ap.add_argument("--child-batch", type=int, default=1000, help=argparse.SUPPRESS)
    ap.add_argument("--child-k", type=int, default=1, help=argparse.SUPPRESS)
    ap.add_argument("--child-mode", default="exclude", help=argparse.SUPPRESS)
    ap.add_argument("--child-exclude", default="", help=argparse.SUPPRESS)
    ap.add_argument("--drop", action="store_true", help="the edge filter (ggms_drop_pair_edges) alone, on a khop3 batch")
    ap.add_argument("--exclude-ab", type=int, default=0, metavar="R",
                    help="with --engine: exclude_seed_edges = none / both, R runs each, alternating")
    args = ap.parse_args()
    if args.engine_child:
        return engine_child(args)
    import torch
    assert torch.cuda.is_available(), "bench_link needs a GPU"
    g = make_graph(args.graph, args.seed)
    if not args.no_leaf:
        leaf_records(args, g)
    if args.drop:
        drop_records(args, g)
    if args.engine:
        # the leaf part's context must not sit beside the engine children's on the device's memory
        torch.cuda.empty_cache()
        engine_records(args, g)


if __name__ == "__main__":
    main()
