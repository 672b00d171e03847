"""random_walk_metapath's leaf beside random_walk's, on the same graph, seeds and walk shape in one process, alternating.

    python tools/bench_walk_metapath.py --graph products --seeds 8000,48000

Three chains per seed count:
    walk         ggms_sample_random_walk, walk_length = T                        (the yardstick: the parent's code)
    metapath_r1  ggms_sample_walk_metapath, one relation, metapath [0], T traversals: the same T x W visits per seed
    bipartite    two relations, the first half of every list relation 0 and the rest relation 1, metapath [0, 1]:
                 T x W visits of two steps each, every step a segment search
The types are synthetic and sorted by construction.  Both samplers share the top-K launch; metapath_r1 - walk is the
price of the type bytes (two loads per step) against the XORWOW state traffic (48 bytes per walk lane).  One JSON line
on stdout; medians over --rounds of the mean of --steps calls, with every round's figure.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from xgnn_amd import datagen, lib, ops  # noqa: E402


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
    ap.add_argument("--seeds", default="8000,48000")
    ap.add_argument("--traversals", type=int, default=3)
    ap.add_argument("--walks", type=int, default=4)
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--restart", type=float, default=0.5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seed", type=int, default=42)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_walk_metapath needs a GPU"
    dev = torch.device("cuda", 0)
    gr = datagen.make_graph(args.graph, seed=args.seed)
    num_node = gr["indptr"].size - 1
    g = ops.DeviceGraph(to_dev(gr["indptr"], dev), to_dev(gr["indices"], dev))
    del gr
    ip64 = g.indptr.long()
    ip64 = torch.where(ip64 < 0, ip64 + (1 << 32), ip64)  # (indptr holds uint32 bits)
    deg = ip64[1:] - ip64[:-1]
    E = int(ip64[-1])
    one = torch.zeros(E, dtype=torch.uint8, device=dev)
    two = torch.empty(E, dtype=torch.uint8, device=dev)
    step = 1 << 22
    for lo in range(0, num_node, step):  # chunk by chunk: no E-sized int64 temporaries
        hi = min(num_node, lo + step)
        b, e = int(ip64[lo]), int(ip64[hi])
        if e > b:
            d = torch.repeat_interleave(deg[lo:hi], deg[lo:hi])
            rank = torch.arange(b, e, device=dev) - torch.repeat_interleave(ip64[lo:hi], deg[lo:hi])
            two[b:e] = (rank * 2 >= d).to(torch.uint8)
            del d, rank
    T, W, K, p = args.traversals, args.walks, args.k, args.restart
    rng = np.random.RandomState(args.seed)
    kinds = ["walk", "metapath_r1", "bipartite"]
    rec = dict(graph=args.graph, traversals=T, walks=W, K=K, restart=p, rounds=args.rounds, steps=args.steps,
               longest_list=int(deg.max()))
    for n in [int(x) for x in args.seeds.split(",")]:
        inp = to_dev(rng.randint(0, num_node, n).astype(np.uint32), dev)
        states = ops.random_states(lib().ggms_random_walk_num_states(n, W), 7, dev)
        calls = dict(walk=lambda: ops.sample_random_walk(g, inp, T, p, W, K, states),
                     metapath_r1=lambda: ops.sample_walk_metapath(g, one, 1, [0], inp, T, p, W, K, 99),
                     bipartite=lambda: ops.sample_walk_metapath(g, two, 2, [0, 1], inp, T, p, W, K, 99))
        # correct before fast: every output edge of the one-relation walk joins a seed and a node, counts within T x W
        src, dst, data, num = calls["metapath_r1"]()
        m = int(num.item())
        assert 0 < m <= n * K and int(data[:m].max()) <= T * W and int(data[:m].min()) >= 1
        got = {k: [] for k in kinds}
        for rnd in range(args.rounds + 1):  # the first round warms up
            for k in (kinds if rnd % 2 == 0 else kinds[::-1]):
                got[k].append(timed(calls[k], args.steps))
        for k in kinds:
            rec[f"{k}_{n}_edges"] = int(calls[k]()[-1].item())
            rec[f"{k}_{n}_us"] = round(float(np.median(got[k][1:])), 2)
            rec[f"{k}_{n}_us_rounds"] = [round(x, 2) for x in got[k][1:]]
        for k in kinds[1:]:
            rec[f"{k}_{n}_over_walk"] = round(rec[f"{k}_{n}_us"] / rec[f"walk_{n}_us"], 3)
    assert ops.device_status() == 0
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
