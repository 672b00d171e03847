"""ppr_topk's leaf beside random_walk's, on the same graph and seeds in one process, alternating.

    python tools/bench_ppr.py --graph products --seeds 8000

Two chains:
    walk   ggms_sample_random_walk at PinSAGE's defaults (walk_length 3, 4 walks, restart 0.5): ~12 visits per seed
    ppr    ggms_sample_ppr (alpha 0.15, eps 1e-4, max_nodes 1024, max_rounds 32 unless given), the same K
They compute different things -- a 12-sample Monte Carlo estimate against the pushed vector itself -- so the ratio is a
price, not a race.  One JSON line on stdout; medians over --rounds of the mean of --steps calls, with every round's
figure, and what the push did: rounds per seed, the share of truncated seeds, the mass that reached p.
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
    ap.add_argument("--seeds", default="8000")
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--alpha", type=float, default=0.15)
    ap.add_argument("--eps", type=float, default=1e-4)
    ap.add_argument("--max-nodes", type=int, default=1024)
    ap.add_argument("--max-rounds", type=int, default=32)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seed", type=int, default=42)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_ppr needs a GPU"
    dev = torch.device("cuda", 0)
    gr = datagen.make_graph(args.graph, seed=args.seed)
    num_node = gr["indptr"].size - 1
    g = ops.DeviceGraph(to_dev(gr["indptr"], dev), to_dev(gr["indices"], dev))
    del gr
    T, W, p, K = 3, 4, 0.5, args.k
    rng = np.random.RandomState(args.seed)
    kinds = ["walk", "ppr"]
    rec = dict(graph=args.graph, K=K, alpha=args.alpha, eps=args.eps, max_nodes=args.max_nodes, max_rounds=args.max_rounds,
               rounds=args.rounds, steps=args.steps)
    for n in [int(x) for x in args.seeds.split(",")]:
        inp = to_dev(rng.randint(0, num_node, n).astype(np.uint32), dev)
        states = ops.random_states(lib().ggms_random_walk_num_states(n, W), 7, dev)
        calls = dict(walk=lambda: ops.sample_random_walk(g, inp, T, p, W, K, states),
                     ppr=lambda: ops.sample_ppr(g, inp, args.alpha, args.eps, args.max_nodes, args.max_rounds, K))
        # correct before fast: the scores of a seed never exceed its pushed mass, which never exceeds 2^30
        src, dst, data, num, stat = calls["ppr"]()
        m, st = int(num.item()), stat.cpu().numpy().view(np.uint32)
        assert 0 < m <= n * K and int(st[:, 1].max()) <= 1 << 30 and int(data[:m].min()) >= 1
        rec[f"ppr_{n}_rounds_mean"] = round(float((st[:, 0] & 0xFF).mean()), 2)
        rec[f"ppr_{n}_truncated_share"] = round(float((st[:, 0] >> 31).mean()), 4)
        rec[f"ppr_{n}_mass_mean"] = round(float(st[:, 1].mean() / (1 << 30)), 4)
        got = {k: [] for k in kinds}
        for rnd in range(args.rounds + 1):  # the first round warms up
            for k in (kinds if rnd % 2 == 0 else kinds[::-1]):
                got[k].append(timed(calls[k], args.steps))
        for k in kinds:
            rec[f"{k}_{n}_edges"] = int(calls[k]()[3].item())
            rec[f"{k}_{n}_us"] = round(float(np.median(got[k][1:])), 2)
            rec[f"{k}_{n}_us_rounds"] = [round(x, 2) for x in got[k][1:]]
        rec[f"ppr_{n}_over_walk"] = round(rec[f"ppr_{n}_us"] / rec[f"walk_{n}_us"], 3)
    assert ops.device_status() == 0
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
