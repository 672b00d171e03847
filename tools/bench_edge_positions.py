"""ggms_edge_positions alone, on sampled batches: the call's time beside the sampler chain that produced the batch
(ggms_sample_batch, khop3) and beside khop_labor's layer time on the same frontiers -- the leaf that reads the same
lists -- with the call's algorithmic bytes: every frontier node's list read once, 8 bytes of list bounds per frontier
node, 12 bytes per edge (row, col, eid).

    python tools/bench_edge_positions.py --graph products --fanout 25,10
    python tools/bench_edge_positions.py --graph papers100M --fanout 5,10,15
    python tools/bench_edge_positions.py --graph papers100M --fanout 5,10,15 --skew 0.5   # hubs turn up in many lists

One JSON line per run on stdout; times are medians over --rounds of the mean of --steps back-to-back calls.

    python tools/bench_edge_positions.py --engine 3 [--parent-root <a built checkout of the parent commit>]

The arch1 step (products, khop3, batch 8000, fanout 25 10; tools/bench_update_rows.py's child loop) without the keys, with
edge_ids = on and with edge_feat = on (a one-column F32 edge table), every configuration in a child process, R runs each
in alternating order; ms per step.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from xgnn_amd import datagen, ops  # noqa: E402
from xgnn_amd._lib import COUNT_DST, COUNT_EDGES, COUNT_INPUT, COUNT_STATUS  # noqa: E402


def to_dev(a, dev):
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(dev)


def timed(fn, steps):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1000.0 / steps  # us


CONFIGS = {"plain": {}, "edge_ids": {"edge_ids": "on"}, "edge_feat": {"edge_feat": "on"}}


def run_engine(args):
    import shutil
    import subprocess
    import tempfile
    g = datagen.make_graph("products", seed=42)
    base = "/dev/shm" if os.path.isdir("/dev/shm") and shutil.disk_usage("/dev/shm").free > 3 * g["indices"].nbytes else None
    d = tempfile.mkdtemp(prefix="ggms_bench_edge_", dir=base)
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "bench_update_rows.py")
    runs = [(name, os.path.abspath(ROOT), keys) for name, keys in CONFIGS.items()]
    if args.parent_root:
        runs.insert(0, ("parent_plain", os.path.abspath(args.parent_root), {}))
    rec = {name: [] for name, _, _ in runs}
    try:
        datagen.write_dataset(d, g, minimal=True, edge_feat=np.ones(g["indices"].size, np.float32))
        if args.parent_root:  # the parent's meta parser knows numbers only
            lines = [ln for ln in open(d + "/meta.txt") if not ln.startswith("EDGE_FEAT")]
            open(d + "/meta_parent.txt", "w").write("".join(lines))
        for rnd in range(args.engine):
            for name, root, keys in (runs if rnd % 2 == 0 else runs[::-1]):
                if args.parent_root:  # swap the meta file in for the parent's run, back for ours
                    want = "meta_parent.txt" if name == "parent_plain" else "meta_full.txt"
                    if not os.path.exists(d + "/meta_full.txt"):
                        shutil.copy(d + "/meta.txt", d + "/meta_full.txt")
                    shutil.copy(d + "/" + want, d + "/meta.txt")
                cmd = [sys.executable, child, "--engine-child", d + "/", "--root", root, "--child-keys", json.dumps(keys),
                       "--epochs", str(args.epochs)]
                r = subprocess.run(["timeout", "-k", "10", "300"] + cmd, capture_output=True, text=True)
                lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
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
    ap.add_argument("--graph", default="products", choices=["products", "papers100M", "tiny"])
    ap.add_argument("--fanout", default="25,10")
    ap.add_argument("--batch", type=int, default=8000)
    ap.add_argument("--skew", type=float, default=0.0, help="datagen.make_graph's neighbour_skew")
    ap.add_argument("--num-batches", type=int, default=4)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--engine", type=int, default=0, metavar="R", help="the arch1 step, R runs per configuration")
    ap.add_argument("--parent-root", help="--engine: a built checkout of another commit, timed as parent_plain")
    ap.add_argument("--epochs", type=int, default=8)
    args = ap.parse_args()
    if args.engine:
        return run_engine(args)
    assert torch.cuda.is_available(), "bench_edge_positions needs a GPU"
    dev = torch.device("cuda", 0)
    gr = datagen.make_graph(args.graph, seed=args.seed, neighbour_skew=args.skew)
    ip, train = gr["indptr"], gr["train_set"]
    g = ops.DeviceGraph(to_dev(ip, dev), to_dev(gr["indices"], dev))
    num_edge = int(gr["indices"].size)
    del gr
    fanouts = [int(x) for x in args.fanout.split(",")]
    L = len(fanouts)
    bs = ops.BatchSampler(g, fanouts, args.batch, sample_type=ops.KHOP3, seed=7, device=dev, num_slots=args.num_batches)
    seeds = [to_dev(train[i * args.batch:(i + 1) * args.batch], dev) for i in range(args.num_batches)]
    deg = g.indptr[1:].long() - g.indptr[:-1].long()
    deg = torch.where(deg < 0, deg + (1 << 32), deg)  # (indptr holds uint32 bits)
    # the batches stay in their slots: the positions are timed on exactly what the chain left
    eids, info = [], []
    for s in range(args.num_batches):
        bs.sample(seeds[s], slot=s, copy_input_nodes=True, distinct=True)
        c = bs.counts_slots[s].cpu().tolist()
        assert c[COUNT_STATUS(L)] == 0
        eids.append([torch.empty(m, dtype=torch.int32, device=dev) for m in bs.max_edges])
        nodes = bs.input_nodes[s]
        fr = [int(c[COUNT_DST(i)]) for i in range(L)]
        list_bytes = sum(4 * int(deg[nodes[:n].long()].sum()) + 8 * n for n in fr)
        edges = sum(int(c[COUNT_EDGES(i)]) for i in range(L))
        longest = max(int(deg[nodes[:n].long()].max()) for n in fr)
        info.append(dict(edges=edges, input_nodes=int(c[COUNT_INPUT(L)]), frontier=fr, bytes=list_bytes + 12 * edges,
                         longest_list=longest))

    def positions(s):
        ops.edge_positions(g, bs.rows[s], bs.cols[s], bs.counts_slots[s], id_map=bs.input_nodes[s], max_edges=bs.max_edges,
                           eids=eids[s], num_edge=num_edge)

    # correct before fast: every id names its edge
    positions(0)
    for i in range(L):
        n = int(bs.counts_slots[0][COUNT_EDGES(i)])
        e = eids[0][i][:n].long()
        e = torch.where(e < 0, e + (1 << 32), e)
        assert bool((g.indices[e] == bs.input_nodes[0][bs.rows[0][i][:n].long()]).all()), "an edge id does not name its edge"

    scratch = ops.BatchSampler(g, fanouts, args.batch, sample_type=ops.KHOP3, seed=7, device=dev)
    got = {"positions_us": [], "chain_us": [], "labor_layers_us": []}
    for _ in range(args.rounds + 1):  # the first round warms up
        per = {k: [] for k in got}
        for s in range(args.num_batches):
            per["positions_us"].append(timed(lambda: positions(s), args.steps))
            per["chain_us"].append(timed(lambda: scratch.sample(seeds[s], distinct=True), args.steps))
            fr = info[s]["frontier"]
            nodes = bs.input_nodes[s]
            # layer i of the batch samples from the first num_dst(i) input nodes; the last entry of `fanouts` is layer 0's
            per["labor_layers_us"].append(sum(
                timed(lambda: ops.sample_khop_labor(g, nodes[:fr[i]], fanouts[L - 1 - i], 99), args.steps) for i in range(L)))
        for k in got:
            got[k].append(float(np.mean(per[k])))
    rec = dict(graph=args.graph, skew=args.skew, fanouts=fanouts, batch=args.batch, rounds=args.rounds, steps=args.steps,
               edges=float(np.mean([x["edges"] for x in info])), input_nodes=float(np.mean([x["input_nodes"] for x in info])),
               longest_list=max(x["longest_list"] for x in info),
               algorithmic_MB=round(float(np.mean([x["bytes"] for x in info])) / 1e6, 3))
    for k, v in got.items():
        rec[k] = round(float(np.median(v[1:])), 2)
        rec[k + "_rounds"] = [round(x, 2) for x in v[1:]]
    rec["GBps"] = round(rec["algorithmic_MB"] * 1e3 / rec["positions_us"], 1)
    rec["positions_over_chain"] = round(rec["positions_us"] / rec["chain_us"], 3)
    rec["positions_over_labor_layers"] = round(rec["positions_us"] / rec["labor_layers_us"], 3)
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
