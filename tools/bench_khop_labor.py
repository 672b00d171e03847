"""khop_labor against khop3 (the default sampler): the same seeds, fanouts and graph in one process, through
ggms_sample_batch and the row gather.  Per step and sampler: input nodes, edges, sampling ms, gather ms, and the step
with the two overlapped as the engine overlaps them (batch s + 1 sampled on one stream while batch s is gathered on
another).  The samplers alternate in rounds; the figures are medians over the rounds.

    python tools/bench_khop_labor.py --graph products --fanout 25,10
    python tools/bench_khop_labor.py --graph papers100M --fanout 5,10,15
    python tools/bench_khop_labor.py --graph community --fanout 15,10,5 --batch 1000
    python tools/bench_khop_labor.py --graph hub --fanout 25,10      # a 10^6-neighbour hub among degree-50 seeds

--graph: products / papers100M (the graphs bench.py builds), community (tests/khop_labor_ref.py's generator at 2.4 M
nodes), hub (1 M nodes of degree 50, node 0 with 10^6 neighbours; timed with and without node 0 among the seeds).
One JSON line per (graph, fanout) on stdout.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from xgnn_amd import datagen, ops  # noqa: E402
from xgnn_amd._lib import COUNT_EDGES, COUNT_INPUT, COUNT_STATUS  # noqa: E402
import khop_labor_ref as ref  # noqa: E402


def make_graph(name, seed):
    if name in ("products", "papers100M", "tiny"):
        g = datagen.make_graph(name, seed=seed)
        return g["indptr"], g["indices"], g["train_set"], g["meta"]["feat_dim"]
    rng = np.random.RandomState(seed)
    if name == "community":
        ip, ix = ref.community_graph(num_node=2_400_000, seed=seed)
    else:  # hub
        N, hub = 1_000_000, 1_000_000
        deg = np.full(N, 50, np.int64)
        deg[0] = hub
        ip = np.zeros(N + 1, np.uint32)
        ip[1:] = np.cumsum(deg)
        ix = rng.randint(0, N, int(ip[-1])).astype(np.uint32)
    N = ip.size - 1
    return ip, ix, rng.permutation(N)[: N // 10].astype(np.uint32), 100


def to_dev(a, dev):
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(dev)


class Run:
    """One sampler's buffers: the batch sampler (two output slots) and two gather outputs."""

    def __init__(self, g, fanouts, batch, code, feat, dev):
        self.bs = ops.BatchSampler(g, fanouts, batch, sample_type=code, seed=7, device=dev, num_slots=2)
        self.L, self.feat = len(fanouts), feat
        self.out = [torch.empty((self.bs.max_unique, feat.shape[1]), dtype=feat.dtype, device=dev) for _ in range(2)]
        self.s_sample, self.s_gather = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)

    def sample(self, seeds, step, slot):
        self.bs.sample(seeds, slot=slot, copy_input_nodes=True, distinct=True, labor_salt=ref.batch_salt(42, 0, step))

    def gather(self, slot):
        c = self.bs.counts_slots[slot]
        ops.gather_scatter(self.out[slot], self.feat, self.bs.input_nodes[slot], None, num=self.bs.max_unique,
                           num_dev=c[COUNT_INPUT(self.L):COUNT_INPUT(self.L) + 1])

    def counts(self, slot):
        c = self.bs.counts_slots[slot].cpu().tolist()
        assert c[COUNT_STATUS(self.L)] == 0, "batch status word"
        return c[COUNT_INPUT(self.L)], sum(c[COUNT_EDGES(i)] for i in range(self.L))

    def timed(self, fn, steps):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(steps)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / steps

    def round(self, batches, steps):
        """(input nodes, edges, sampling ms, gather ms, overlapped step ms) of one round over `batches`."""
        nb = len(batches)

        def sampling(n):
            for s in range(n):
                self.sample(batches[s % nb], s % nb, s & 1)

        def gathering(n):
            for s in range(n):
                self.gather(0)

        def overlapped(n):  # batch s + 1 is sampled while batch s is gathered; a slot is reused once its gather is done
            done = [None, None]
            for s in range(n):
                slot = s & 1
                with torch.cuda.stream(self.s_sample):
                    if done[slot] is not None:
                        self.s_sample.wait_event(done[slot])
                    self.sample(batches[s % nb], s % nb, slot)
                    sampled = torch.cuda.Event()
                    sampled.record()
                with torch.cuda.stream(self.s_gather):
                    self.s_gather.wait_event(sampled)
                    self.gather(slot)
                    done[slot] = torch.cuda.Event()
                    done[slot].record()
            torch.cuda.current_stream().wait_stream(self.s_sample)
            torch.cuda.current_stream().wait_stream(self.s_gather)

        nodes, edges = [], []
        for s in range(nb):
            self.sample(batches[s], s, 0)
            n, e = self.counts(0)
            nodes.append(n)
            edges.append(e)
        ms_s = self.timed(sampling, steps)
        self.sample(batches[0], 0, 0)
        ms_g = self.timed(gathering, steps)
        ms_o = self.timed(overlapped, steps)
        return float(np.mean(nodes)), float(np.mean(edges)), ms_s, ms_g, ms_o


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graph", default="products", choices=["products", "papers100M", "community", "hub", "tiny"])
    ap.add_argument("--fanout", default="25,10", help="one or more fanout lists, ';'-separated: 25,10;5,10,15")
    ap.add_argument("--batch", type=int, default=8000)
    ap.add_argument("--num-batches", type=int, default=8)
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seed", type=int, default=42)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_khop_labor needs a GPU"
    dev = torch.device("cuda", 0)
    ip, ix, train, dim = make_graph(args.graph, args.seed)
    g = ops.DeviceGraph(to_dev(ip, dev), to_dev(ix, dev))
    feat = torch.zeros((ip.size - 1, dim), dtype=torch.float32, device=dev)  # the gather's time does not depend on the values
    batches = [to_dev(train[i * args.batch:(i + 1) * args.batch], dev) for i in range(args.num_batches)]
    variants = {"": batches}
    if args.graph == "hub":  # the same batches, node 0 (the hub) in place of each batch's first seed
        train = train[train != 0]
        batches = [to_dev(train[i * args.batch:(i + 1) * args.batch], dev) for i in range(args.num_batches)]
        with_hub = [b.clone() for b in batches]
        for b in with_hub:
            b[0] = 0
        variants = {"without_hub": batches, "with_hub": with_hub}
    for fan in args.fanout.split(";"):
        fanouts = [int(x) for x in fan.split(",")]
        runs = {"khop3": Run(g, fanouts, args.batch, ops.KHOP3, feat, dev),
                "khop_labor": Run(g, fanouts, args.batch, ops.KHOP_LABOR, feat, dev)}
        for vname, vb in variants.items():
            for r in runs.values():  # warm-up: every kernel of every shape once
                r.round(vb, 2)
            got = {k: [] for k in runs}
            for _ in range(args.rounds):  # alternate the samplers
                for k, r in runs.items():
                    got[k].append(r.round(vb, args.steps))
            rec = {"graph": args.graph + ("/" + vname if vname else ""), "fanouts": fanouts, "batch": args.batch,
                   "rounds": args.rounds, "steps": args.steps}
            for k, v in got.items():
                med = np.median(np.array(v), axis=0)
                rec[k] = dict(input_nodes=round(med[0], 1), edges=round(med[1], 1), sample_ms=round(med[2], 4),
                              gather_ms=round(med[3], 4), sum_ms=round(med[2] + med[3], 4), overlapped_ms=round(med[4], 4),
                              overlapped_ms_rounds=[round(x[4], 4) for x in v])
            a, b = rec["khop_labor"], rec["khop3"]
            rec["labor_over_khop3"] = dict(input_nodes=round(a["input_nodes"] / b["input_nodes"], 4),
                                           sample_ms=round(a["sample_ms"] / b["sample_ms"], 4),
                                           gather_ms=round(a["gather_ms"] / b["gather_ms"], 4),
                                           overlapped_ms=round(a["overlapped_ms"] / b["overlapped_ms"], 4))
            print(json.dumps(rec), flush=True)
        del runs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
