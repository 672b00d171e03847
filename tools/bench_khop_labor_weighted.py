"""khop_labor_weighted's batch chain beside khop_labor's and weighted_khop's: the same graph, seeds and fanouts in one
process, alternating.

    python tools/bench_khop_labor_weighted.py --graph products --fanout 25,10
    python tools/bench_khop_labor_weighted.py --graph papers100M --fanout 5,10,15

Three sampling chains (seeds -> every layer -> dedup -> local ids), one enqueue each, timed with events around --steps
batches of --batch distinct train seeds:
    labor_weighted  ggms_sample_batch_labor_weighted, weights = datagen.edge_weights('default') (integers 1 .. 10)
    labor           ggms_sample_batch(GGMS_KHOP_LABOR)            (reads half the list bytes: ids without weights)
    weighted_khop   ggms_sample_batch(GGMS_WEIGHTED_KHOP) on the alias tables of the same weights (WITH replacement)
The weighted sampler is reported against khop_labor, not gated on it.  One JSON line on stdout; medians over --rounds
of the mean time per batch, and the rounds themselves (their spread is the box's run-to-run noise).
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


def to_dev(a, dev):
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graph", default="products", choices=["products", "papers100M", "tiny"])
    ap.add_argument("--fanout", default="25,10")
    ap.add_argument("--batch", type=int, default=8000)
    ap.add_argument("--steps", type=int, default=800)  # a round of a few hundred ms: short windows time the clock
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--skip-weighted-khop", action="store_true", help="no alias tables (minutes of host time at papers100M size)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_khop_labor_weighted needs a GPU"
    dev = torch.device("cuda", 0)
    gr = datagen.make_graph(args.graph, seed=args.seed)
    train = gr["train_set"]
    w = datagen.edge_weights(gr, "default", seed=args.seed)
    g = ops.DeviceGraph(to_dev(gr["indptr"], dev), to_dev(gr["indices"], dev))
    fanouts = [int(x) for x in args.fanout.split(",")]
    samplers = {"labor_weighted": ops.LaborWeightedBatchSampler(g, to_dev(w, dev), fanouts, args.batch, device=dev),
                "labor": ops.BatchSampler(g, fanouts, args.batch, sample_type=ops.KHOP_LABOR, device=dev)}
    if not args.skip_weighted_khop:
        prob, alias = datagen.build_alias_tables(gr["indptr"], gr["indices"], w)
        samplers["weighted_khop"] = ops.BatchSampler(g, fanouts, args.batch, sample_type=ops.WEIGHTED_KHOP, seed=7, device=dev,
                                                     prob_table=to_dev(prob, dev), alias_table=to_dev(alias, dev))
    del gr
    nb = max(1, min(args.steps, 24, train.size // args.batch))
    seeds = [to_dev(train[s * args.batch:(s + 1) * args.batch], dev) for s in range(nb)]

    def run(kind, s):
        bs = samplers[kind]
        if kind == "labor_weighted":
            bs.sample(seeds[s % nb], salt=s, distinct=True)
        else:
            bs.sample(seeds[s % nb], distinct=True, labor_salt=s)

    def timed(kind):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for s in range(args.steps):
            run(kind, s)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1000.0 / args.steps  # us per batch

    kinds = list(samplers)
    rec = dict(graph=args.graph, fanouts=fanouts, batch=args.batch, rounds=args.rounds, steps=args.steps)
    for k in kinds:  # correct before fast: every chain ends with a clean status; the edge counts
        run(k, 0)
        rec[k + "_edges"] = [lay["row"].numel() for lay in samplers[k].result()["layers"]]
    got = {k: [] for k in kinds}
    for rnd in range(args.rounds + 1):  # the first round warms up
        for k in (kinds if rnd % 2 == 0 else kinds[::-1]):
            got[k].append(timed(k))
    for k in kinds:
        rec[k + "_us"] = round(float(np.median(got[k][1:])), 2)
        rec[k + "_us_rounds"] = [round(x, 2) for x in got[k][1:]]
    for k in kinds:
        if k != "labor":
            rec[k + "_over_labor"] = round(rec[k + "_us"] / rec["labor_us"], 3)
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
