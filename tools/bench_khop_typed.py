"""khop_typed's leaf beside khop_labor's, on the frontiers of sampled khop3 batches: the same graph, seeds and fanouts in
one process, alternating.

    python tools/bench_khop_typed.py --graph products --fanout 25,10
    python tools/bench_khop_typed.py --graph papers100M --fanout 5,10,15

Per frontier of a batch (layer i samples from the first num_dst(i) input nodes) four chains are timed:
    labor        ggms_sample_khop_labor                                   (the yardstick: the parent's code)
    typed_r1     ggms_sample_khop_typed, one type, fanout k               (selects labor's edges: checked)
    typed_even   four types, every list cut into quarters, the same K split evenly over them
    typed_rare   four types, the last one holding the last deg / 32 (at least one) entries of a list, the same split
The types are synthetic and sorted by construction (a function of the entry's rank in its list).  typed_r1 - labor is the
price of the boundary launch (12 bytes per seed read, 8 written), of the position and type streams (5 bytes per edge) and
of reading the count, the boundary and the list head again in the select launch.  Bytes: lists read once, 12 bytes per
seed for labor and 40 + 8 R for typed (id, bounds, count, offset and R boundary words written and read), 8 / 13 bytes per
edge.  One JSON line on stdout; medians over --rounds of the mean of --steps calls.
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


def split(k, R):
    """K split evenly over R types (the remainder to the first ones); a type may get 0."""
    return [k // R + (1 if r < k % R else 0) for r in range(R)]


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
    assert torch.cuda.is_available(), "bench_khop_typed needs a GPU"
    dev = torch.device("cuda", 0)
    gr = datagen.make_graph(args.graph, seed=args.seed)
    train = gr["train_set"]
    g = ops.DeviceGraph(to_dev(gr["indptr"], dev), to_dev(gr["indices"], dev))
    del gr
    ip64 = g.indptr.long()
    ip64 = torch.where(ip64 < 0, ip64 + (1 << 32), ip64)  # (indptr holds uint32 bits)
    deg = ip64[1:] - ip64[:-1]
    E = int(ip64[-1])
    # the types, chunk by chunk (no E-sized int64 temporaries): rank = the entry's position in its list
    types = dict(r1=torch.zeros(E, dtype=torch.uint8, device=dev), even=torch.empty(E, dtype=torch.uint8, device=dev),
                 rare=torch.empty(E, dtype=torch.uint8, device=dev))
    N, step = deg.numel(), 1 << 22
    for lo in range(0, N, step):
        hi = min(N, lo + step)
        b, e = int(ip64[lo]), int(ip64[hi])
        if e > b:
            d = torch.repeat_interleave(deg[lo:hi], deg[lo:hi])
            rank = torch.arange(b, e, device=dev) - torch.repeat_interleave(ip64[lo:hi], deg[lo:hi])
            types["even"][b:e] = (rank * 4 // d).to(torch.uint8)
            common = d - torch.clamp(d // 32, min=1)  # entries of the three common types
            types["rare"][b:e] = torch.where(rank >= common, torch.full_like(rank, 3),
                                             rank * 3 // torch.clamp(common, min=1)).to(torch.uint8)
            del d, rank, common
    fanouts = [int(x) for x in args.fanout.split(",")]
    L = len(fanouts)
    bs = ops.BatchSampler(g, fanouts, args.batch, sample_type=ops.KHOP3, seed=7, device=dev, num_slots=args.num_batches)
    kinds = ["labor", "typed_r1", "typed_even", "typed_rare"]
    chains = []  # per batch, per layer: frontier, fanout, list bytes
    for s in range(args.num_batches):
        bs.sample(to_dev(train[s * args.batch:(s + 1) * args.batch], dev), slot=s, copy_input_nodes=True, distinct=True)
        c = bs.counts_slots[s].cpu().tolist()
        assert c[COUNT_STATUS(L)] == 0
        layers = []
        for i in range(L):
            nodes = bs.input_nodes[s][:int(c[COUNT_DST(i)])].contiguous()
            d = deg[nodes.long()]
            layers.append(dict(nodes=nodes, k=fanouts[i], list_bytes=int(4 * d.sum()), longest=int(d.max())))
        chains.append(layers)

    def call(kind, lay):
        if kind == "labor":
            return ops.sample_khop_labor(g, lay["nodes"], lay["k"], 99)
        name = kind[len("typed_"):]
        return ops.sample_khop_typed(g, types[name], split(lay["k"], 1 if name == "r1" else 4), lay["nodes"], 99)

    # correct before fast: with one type the typed leaf selects khop_labor's edges, and its positions name them; every
    # chain's edge count (the bytes below)
    edges = {k: [] for k in kinds}
    for s, ch in enumerate(chains):
        for lay in ch:
            for k in kinds:
                edges[k].append((s, int(call(k, lay)[-1].item())))
    for lay in chains[0]:
        a, b = call("labor", lay), call("typed_r1", lay)
        n = int(a[2].item())
        assert n == int(b[4].item()) and torch.equal(a[0][:n], b[0][:n]) and torch.equal(a[1][:n], b[1][:n])
        p = b[2][:n].long()
        p = torch.where(p < 0, p + (1 << 32), p)
        assert torch.equal(g.indices[p], b[1][:n]), "a position does not name its edge"
        assert int(b[3][:n].max()) == 0
        for name in ("even", "rare"):
            o = call("typed_" + name, lay)
            n = int(o[4].item())
            p = o[2][:n].long()
            p = torch.where(p < 0, p + (1 << 32), p)
            assert torch.equal(types[name][p], o[3][:n]) and torch.equal(g.indices[p], o[1][:n])

    got = {k: [] for k in kinds}
    for rnd in range(args.rounds + 1):  # the first round warms up
        per = {k: [] for k in kinds}
        for s in range(args.num_batches):
            for k in (kinds if rnd % 2 == 0 else kinds[::-1]):
                per[k].append(timed(lambda: [call(k, lay) for lay in chains[s]], args.steps))
        for k in kinds:
            got[k].append(float(np.mean(per[k])))
    rec = dict(graph=args.graph, fanouts=fanouts, batch=args.batch, rounds=args.rounds, steps=args.steps,
               frontier=[int(np.mean([ch[i]["nodes"].numel() for ch in chains])) for i in range(L)],
               longest_list=max(lay["longest"] for ch in chains for lay in ch))
    seeds = float(np.mean([sum(lay["nodes"].numel() for lay in ch) for ch in chains]))
    lists = float(np.mean([sum(lay["list_bytes"] for lay in ch) for ch in chains]))
    for k in kinds:
        e = sum(n for _, n in edges[k]) / len(chains)
        per_seed, per_edge = (12, 8) if k == "labor" else (40 + 8 * (1 if k == "typed_r1" else 4), 13)
        rec[k + "_edges"] = int(e)
        rec[k + "_MB"] = round((lists + per_seed * seeds + per_edge * e) / 1e6, 3)
        rec[k + "_us"] = round(float(np.median(got[k][1:])), 2)
        rec[k + "_us_rounds"] = [round(x, 2) for x in got[k][1:]]
    for k in kinds[1:]:
        rec[k + "_over_labor"] = round(rec[k + "_us"] / rec["labor_us"], 3)
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
