"""khop_typed_temporal's leaf beside its two parents, on the frontiers of sampled khop3 batches: the same graph, seeds
and fanouts in one process, alternating.

    python tools/bench_khop_typed_temporal.py --graph products --fanout 25,10

Per frontier of a batch (layer i samples from the first num_dst(i) input nodes) four chains are timed:
    typed        ggms_sample_khop_typed, four types (every list cut into quarters), K split evenly     (yardstick)
    tt_typed     ggms_sample_khop_typed_temporal on the SAME types, every cut 0xffffffff: the same edges (checked)
    temporal     ggms_sample_khop_temporal, fanout K, every cut 0xffffffff                               (yardstick)
    tt_r1        ggms_sample_khop_typed_temporal with one type, fanout K: the same edges (checked)
The types and times are synthetic and sorted by construction (the time of an entry is its rank in its list).  With no cut
the new leaf does its parent's selection work; the difference is the search (one more array probed in the same rounds,
four end loads instead of two), the record (2 R words per seed instead of R) and the cut word per seed.
One JSON line on stdout; medians and the min .. max spread over --rounds of the mean of --steps calls.
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
    assert torch.cuda.is_available(), "bench_khop_typed_temporal needs a GPU"
    dev = torch.device("cuda", 0)
    gr = datagen.make_graph(args.graph, seed=args.seed)
    train = gr["train_set"]
    g = ops.DeviceGraph(to_dev(gr["indptr"], dev), to_dev(gr["indices"], dev))
    del gr
    ip64 = g.indptr.long()
    ip64 = torch.where(ip64 < 0, ip64 + (1 << 32), ip64)  # (indptr holds uint32 bits)
    deg = ip64[1:] - ip64[:-1]
    E = int(ip64[-1])
    # chunk by chunk (no E-sized int64 temporaries): time = the entry's rank in its list, type = its quarter
    one, four = torch.zeros(E, dtype=torch.uint8, device=dev), torch.empty(E, dtype=torch.uint8, device=dev)
    time = torch.empty(E, dtype=torch.int32, device=dev)
    N, step = deg.numel(), 1 << 22
    for lo in range(0, N, step):
        hi = min(N, lo + step)
        b, e = int(ip64[lo]), int(ip64[hi])
        if e > b:
            d = torch.repeat_interleave(deg[lo:hi], deg[lo:hi])
            rank = torch.arange(b, e, device=dev) - torch.repeat_interleave(ip64[lo:hi], deg[lo:hi])
            four[b:e] = (rank * 4 // d).to(torch.uint8)
            time[b:e] = rank.to(torch.int32)
            del d, rank
    fanouts = [int(x) for x in args.fanout.split(",")]
    L = len(fanouts)
    bs = ops.BatchSampler(g, fanouts, args.batch, sample_type=ops.KHOP3, seed=7, device=dev, num_slots=args.num_batches)
    chains = []  # per batch, per layer: frontier, its cuts, fanout
    for s in range(args.num_batches):
        bs.sample(to_dev(train[s * args.batch:(s + 1) * args.batch], dev), slot=s, copy_input_nodes=True, distinct=True)
        c = bs.counts_slots[s].cpu().tolist()
        assert c[COUNT_STATUS(L)] == 0
        layers = []
        for i in range(L):
            nodes = bs.input_nodes[s][:int(c[COUNT_DST(i)])].contiguous()
            layers.append(dict(nodes=nodes, cut=torch.full_like(nodes, -1), k=fanouts[i]))  # -1: the bits of 0xffffffff
        chains.append(layers)

    def split(k):
        return [k // 4 + (1 if r < k % 4 else 0) for r in range(4)]

    def call(kind, lay):
        if kind == "typed":
            return ops.sample_khop_typed(g, four, split(lay["k"]), lay["nodes"], 99)
        if kind == "tt_typed":
            return ops.sample_khop_typed_temporal(g, four, time, split(lay["k"]), lay["nodes"], lay["cut"], 99)
        if kind == "temporal":
            return ops.sample_khop_temporal(g, time, lay["nodes"], lay["cut"], lay["k"], 99)
        return ops.sample_khop_typed_temporal(g, one, time, [lay["k"]], lay["nodes"], lay["cut"], 99)

    # correct before fast: each pair emits the same edges
    for lay in chains[0]:
        for old, new, arrays in (("typed", "tt_typed", 4), ("temporal", "tt_r1", 3)):
            a, b = call(old, lay), call(new, lay)
            n = int(a[arrays].item())
            assert n == int(b[4].item()) and all(torch.equal(a[j][:n], b[j][:n]) for j in range(arrays)), (old, new)

    kinds = ["typed", "tt_typed", "temporal", "tt_r1"]
    got = {k: [] for k in kinds}
    for rnd in range(args.rounds + 1):  # the first round warms up
        per = {k: [] for k in kinds}
        for s in range(args.num_batches):
            for k in (kinds if rnd % 2 == 0 else kinds[::-1]):
                per[k].append(timed(lambda: [call(k, lay) for lay in chains[s]], args.steps))
        for k in kinds:
            got[k].append(float(np.mean(per[k])))
    rec = dict(graph=args.graph, fanouts=fanouts, batch=args.batch, rounds=args.rounds, steps=args.steps,
               frontier=[int(np.mean([ch[i]["nodes"].numel() for ch in chains])) for i in range(L)])
    for k in kinds:
        rec[k + "_us"] = round(float(np.median(got[k][1:])), 2)
        rec[k + "_us_min_max"] = [round(min(got[k][1:]), 2), round(max(got[k][1:]), 2)]
    rec["tt_typed_over_typed"] = round(rec["tt_typed_us"] / rec["typed_us"], 3)
    rec["tt_r1_over_temporal"] = round(rec["tt_r1_us"] / rec["temporal_us"], 3)
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
