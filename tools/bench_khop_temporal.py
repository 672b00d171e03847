"""khop_temporal's leaf beside khop_labor's, on the frontiers of sampled khop3 batches: the same graph, seeds and
fanouts in one process, alternating.

    python tools/bench_khop_temporal.py --graph products --fanout 25,10
    python tools/bench_khop_temporal.py --graph papers100M --fanout 5,10,15

Per frontier of a batch (layer i samples from the first num_dst(i) input nodes) three chains are timed:
    labor          ggms_sample_khop_labor                                    (the yardstick: the parent's code)
    temporal_inf   ggms_sample_khop_temporal, every cut 0xffffffff           (selects labor's edges: checked)
    temporal_half  ggms_sample_khop_temporal, every cut at its list's median time
    recent_half    the same cuts, GGMS_PICK_RECENT
The times are synthetic and sorted by construction: edge_time[p] = p - indptr[v], the entry's rank in its list, so the
cut deg / 2 makes the first half of every list eligible.  temporal - labor at cut = +inf is the price of the prefix
launch (12 bytes per seed read, 8 written), of the position stream (4 bytes per edge) and of reading e, c and the list
head again in the select launch.  One JSON line on stdout; medians over --rounds of the mean of --steps calls.
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
from xgnn_amd._lib import COUNT_DST, COUNT_STATUS  # noqa: E402

INF = 0xFFFFFFFF


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graph", default="products", choices=["products", "papers100M", "tiny"])
    ap.add_argument("--fanout", default="25,10")
    ap.add_argument("--batch", type=int, default=8000)
    ap.add_argument("--num-batches", type=int, default=4)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seed", type=int, default=42)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_khop_temporal needs a GPU"
    dev = torch.device("cuda", 0)
    gr = datagen.make_graph(args.graph, seed=args.seed)
    train = gr["train_set"]
    g = ops.DeviceGraph(to_dev(gr["indptr"], dev), to_dev(gr["indices"], dev))
    del gr
    ip64 = g.indptr.long()
    ip64 = torch.where(ip64 < 0, ip64 + (1 << 32), ip64)  # (indptr holds uint32 bits)
    deg = ip64[1:] - ip64[:-1]
    E = int(ip64[-1])
    # edge_time[p] = the rank of p in its list, chunk by chunk (no E-sized int64 temporaries)
    edge_time = torch.empty(E, dtype=torch.int32, device=dev)
    N, step = deg.numel(), 1 << 22
    for lo in range(0, N, step):
        hi = min(N, lo + step)
        b, e = int(ip64[lo]), int(ip64[hi])
        if e > b:
            start = torch.repeat_interleave(ip64[lo:hi], deg[lo:hi])
            edge_time[b:e] = (torch.arange(b, e, device=dev) - start).int()
            del start
    fanouts = [int(x) for x in args.fanout.split(",")]
    L = len(fanouts)
    bs = ops.BatchSampler(g, fanouts, args.batch, sample_type=ops.KHOP3, seed=7, device=dev, num_slots=args.num_batches)
    chains = []  # per batch, per layer: (frontier, cut_inf, cut_half, fanout, algorithmic bytes)
    for s in range(args.num_batches):
        bs.sample(to_dev(train[s * args.batch:(s + 1) * args.batch], dev), slot=s, copy_input_nodes=True, distinct=True)
        c = bs.counts_slots[s].cpu().tolist()
        assert c[COUNT_STATUS(L)] == 0
        layers = []
        for i in range(L):
            nodes = bs.input_nodes[s][:int(c[COUNT_DST(i)])].contiguous()
            d = deg[nodes.long()]
            k = fanouts[i]
            half = (d // 2)
            # lists read once (the eligible part), bounds, ids, cuts; src, dst, pos written
            by = dict(labor=int(4 * d.sum() + 12 * nodes.numel() + 8 * torch.clamp(d, max=k).sum()),
                      temporal_inf=int(4 * d.sum() + 20 * nodes.numel() + 12 * torch.clamp(d, max=k).sum()),
                      temporal_half=int(4 * half.sum() + 20 * nodes.numel() + 12 * torch.clamp(half, max=k).sum()))
            layers.append(dict(nodes=nodes, inf=torch.full_like(nodes, -1), half=half.int().contiguous(), k=k, bytes=by,
                               longest=int(d.max())))
        chains.append(layers)

    def run(kind, s):
        for lay in chains[s]:
            if kind == "labor":
                ops.sample_khop_labor(g, lay["nodes"], lay["k"], 99)
            elif kind == "temporal_inf":
                ops.sample_khop_temporal(g, edge_time, lay["nodes"], lay["inf"], lay["k"], 99)
            elif kind == "temporal_half":
                ops.sample_khop_temporal(g, edge_time, lay["nodes"], lay["half"], lay["k"], 99)
            else:
                ops.sample_khop_temporal(g, edge_time, lay["nodes"], lay["half"], lay["k"], 99, ops.PICK_RECENT)

    # correct before fast: without a cut the temporal leaf selects khop_labor's edges, and its positions name them
    for lay in chains[0]:
        a = ops.sample_khop_labor(g, lay["nodes"], lay["k"], 99)
        b = ops.sample_khop_temporal(g, edge_time, lay["nodes"], lay["inf"], lay["k"], 99)
        n = int(a[2].item())
        assert n == int(b[3].item()) and torch.equal(a[0][:n], b[0][:n]) and torch.equal(a[1][:n], b[1][:n])
        p = b[2][:n].long()
        p = torch.where(p < 0, p + (1 << 32), p)
        assert torch.equal(g.indices[p], b[1][:n]), "a position does not name its edge"

    kinds = ["labor", "temporal_inf", "temporal_half", "recent_half"]
    got = {k: [] for k in kinds}
    for rnd in range(args.rounds + 1):  # the first round warms up
        per = {k: [] for k in kinds}
        for s in range(args.num_batches):
            for k in (kinds if rnd % 2 == 0 else kinds[::-1]):
                per[k].append(timed(lambda: run(k, s), args.steps))
        for k in kinds:
            got[k].append(float(np.mean(per[k])))
    rec = dict(graph=args.graph, fanouts=fanouts, batch=args.batch, rounds=args.rounds, steps=args.steps,
               frontier=[int(np.mean([ch[i]["nodes"].numel() for ch in chains])) for i in range(L)],
               longest_list=max(lay["longest"] for ch in chains for lay in ch))
    for k in ("labor", "temporal_inf", "temporal_half"):
        rec[k + "_MB"] = round(float(np.mean([sum(lay["bytes"][k] for lay in ch) for ch in chains])) / 1e6, 3)
    for k in kinds:
        rec[k + "_us"] = round(float(np.median(got[k][1:])), 2)
        rec[k + "_us_rounds"] = [round(x, 2) for x in got[k][1:]]
    rec["temporal_inf_over_labor"] = round(rec["temporal_inf_us"] / rec["labor_us"], 3)
    rec["temporal_half_over_labor"] = round(rec["temporal_half_us"] / rec["labor_us"], 3)
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
