"""khop_budget's leaf beside khop_labor's, on the same graph and seeds in one process, alternating.

    python tools/bench_khop_budget.py --graph products --seeds 8000 --k 10

Chains, all with the per-seed cap / fanout k:
    labor          ggms_sample_khop_labor
    budget_<mode>_<x>  ggms_sample_khop_budget, mode uniform | ladies, node budget S = x times the frontier size
They compute different things -- a node-wise draw against a layer-wise one under a node budget -- so the ratio is a
price, not a race.  One JSON line on stdout: medians over --rounds of the mean of --steps calls with every round's
figure, each chain's edges, M and the number chosen, and the figure the sampler exists for: the distinct nodes of a
3-layer batch (fanouts k, k, k; budget S per layer) for both samplers.
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

MODES = dict(uniform=ops.BUDGET_UNIFORM, ladies=ops.BUDGET_LADIES)


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
    ap.add_argument("--seeds", type=int, default=8000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--budgets", default="1,4", help="node budgets, in multiples of the frontier size")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seed", type=int, default=42)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_khop_budget needs a GPU"
    dev = torch.device("cuda", 0)
    gr = datagen.make_graph(args.graph, seed=args.seed)
    num_node = gr["indptr"].size - 1
    g = ops.DeviceGraph(to_dev(gr["indptr"], dev), to_dev(gr["indices"], dev))
    del gr
    n, k = args.seeds, args.k
    inp = to_dev(np.random.RandomState(args.seed).permutation(num_node)[:n].astype(np.uint32), dev)
    bmap = ops.budget_map(num_node, dev)
    mults = [int(x) for x in args.budgets.split(",")]
    calls = dict(labor=lambda: ops.sample_khop_labor(g, inp, k, 77))
    for name, mode in MODES.items():
        for x in mults:
            calls[f"budget_{name}_{x}"] = (lambda mode=mode, x=x: ops.sample_khop_budget(
                g, inp, x * n, k, 77, mode=mode, map=bmap, num_edge=num_node))
    kinds = list(calls)
    rec = dict(graph=args.graph, seeds=n, k=k, rounds=args.rounds, steps=args.steps)
    for kind in kinds[1:]:  # correct before fast: the budget holds, the map is clean again
        src, dst, pos, num, stat = calls[kind]()
        m, (M, chosen) = int(num.item()), stat.tolist()
        assert 0 < m <= n * k and torch.unique(dst[:m]).numel() <= chosen <= M and not bmap.any().item()
        rec[f"{kind}_M"], rec[f"{kind}_chosen"] = M, chosen
    got = {kind: [] for kind in kinds}
    for rnd in range(args.rounds + 1):  # the first round warms up
        for kind in (kinds if rnd % 2 == 0 else kinds[::-1]):
            got[kind].append(timed(calls[kind], args.steps))
    for kind in kinds:
        rec[f"{kind}_edges"] = int(calls[kind]()[-2 if kind != "labor" else -1].item())
        rec[f"{kind}_us"] = round(float(np.median(got[kind][1:])), 2)
        rec[f"{kind}_us_rounds"] = [round(v, 2) for v in got[kind][1:]]
    # the distinct nodes of a 3-layer batch
    bs = ops.BatchSampler(g, [k] * 3, n, sample_type=ops.KHOP_LABOR, device=dev)
    bs.sample(inp, distinct=True, labor_salt=5)
    rec["labor_batch_nodes"] = int(bs.result()["input_nodes"].numel())
    for name, mode in MODES.items():
        for x in mults:
            bb = ops.BudgetBatchSampler(g, [k] * 3, [x * n] * 3, n, mode=mode, device=dev, num_edge=num_node)
            bb.sample(inp, salt=5, distinct=True)
            res = bb.result()
            rec[f"budget_{name}_{x}_batch_nodes"] = int(res["input_nodes"].numel())
            rec[f"budget_{name}_{x}_batch_edges"] = [int(l["row"].numel()) for l in res["layers"]]
            del bb
    assert ops.device_status() == 0
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
