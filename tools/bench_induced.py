"""ggms_induced_edges alone, on the input-node lists of sampled khop3 batches, beside its yardstick: one hop of
ggms_khop_closure over the same lists -- the same lists through the same edge tiles (edge_tiles.h), one random 4-byte
access per entry.  The leaf walks the lists twice, so the expectation is at most 2 x the closure hop's time (+ 10 % for
session drift).  The two alternate, batch by batch, inside every round of one session.

    python tools/bench_induced.py --graph products --fanout 25,10 --batch 8000
    python tools/bench_induced.py --graph products --fanout 25,10 --batch 1024     # ShaDow's usual size
    python tools/bench_induced.py --graph papers100M --fanout 5,10,15 --batch 8000
    python tools/bench_induced.py --graph papers100M --fanout 5,10,15 --batch 1024

One JSON line per run on stdout; times are medians over --rounds of the mean of --steps back-to-back calls (buffers and
workspaces allocated once, outside the timed region; no host synchronisation inside it).  Algorithmic bytes:
  leaf     2 walks x (4 B list entry + 4 B map word) per walked entry, 3 x 8 B of list bounds and 4 x 4 B of id / map word
           per node (mark, degree scan, unmark), 12 B per induced edge (row, col, eid)
  closure  (4 B list entry + 4 B stamp word) per walked entry, 8 B of list bounds per node, 8 B per claimed node
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from xgnn_amd import datagen, ops  # noqa: E402
from xgnn_amd._lib import COUNT_INPUT, COUNT_STATUS, check, lib  # noqa: E402


def to_dev(a, dev):
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(dev)


def ptr(t):
    return C.c_void_p(t.data_ptr())


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
    assert torch.cuda.is_available(), "bench_induced needs a GPU"
    dev = torch.device("cuda", 0)
    gr = datagen.make_graph(args.graph, seed=args.seed)
    ip, train = gr["indptr"], gr["train_set"]
    g = ops.DeviceGraph(to_dev(ip, dev), to_dev(gr["indices"], dev))
    num_edge, num_node = int(gr["indices"].size), int(ip.size - 1)
    del gr
    fanouts = [int(x) for x in args.fanout.split(",")]
    L = len(fanouts)
    bs = ops.BatchSampler(g, fanouts, args.batch, sample_type=ops.KHOP3, seed=7, device=dev)
    deg = g.indptr[1:].long() - g.indptr[:-1].long()
    deg = torch.where(deg < 0, deg + (1 << 32), deg)  # (indptr holds uint32 bits)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    # the node lists, as the batches left them
    lists = []
    for s in range(args.num_batches):
        bs.sample(to_dev(train[s * args.batch:(s + 1) * args.batch], dev), distinct=True)
        c = bs.counts.cpu().tolist()
        assert c[COUNT_STATUS(L)] == 0
        lists.append(bs.result()["input_nodes"].clone())
    max_nodes = max(t.numel() for t in lists)
    walked = [int(deg[t.long()].sum()) for t in lists]
    cap = max(walked)  # no batch induces more edges than it walks

    local_of = ops.induced_map(num_node, dev)
    row, col, eid = (torch.empty(max(cap, 4), dtype=torch.int32, device=dev) for _ in range(3))
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    ws_bytes = lib().ggms_induced_edges_workspace_bytes(max_nodes, num_edge)
    ws = torch.empty((ws_bytes + 3) // 4, dtype=torch.int32, device=dev)

    def induced(s):
        t = lists[s]
        check(lib().ggms_induced_edges(C.byref(g.c), num_edge, ptr(t), t.numel(), None, ptr(local_of), ptr(row), ptr(col),
                                       ptr(eid), cap, ptr(counts), ptr(ws), ws_bytes, stream), "ggms_induced_edges")

    visit = torch.zeros(num_node, dtype=torch.int32, device=dev)
    closure = torch.empty(num_node, dtype=torch.int32, device=dev)
    hops = torch.zeros(3, dtype=torch.int64, device=dev)
    cws_bytes = lib().ggms_khop_closure_workspace_bytes(num_node)
    cws = torch.empty((cws_bytes + 3) // 4, dtype=torch.int32, device=dev)
    stamp = [0]

    def closure_hop(s):
        t = lists[s]
        stamp[0] += 1
        check(lib().ggms_khop_closure(C.byref(g.c), ptr(t), t.numel(), 1, ptr(visit), stamp[0], None, ptr(closure),
                                      ptr(hops), ptr(cws), cws_bytes, stream), "ggms_khop_closure")

    # correct before fast: every induced edge names an edge of the graph between two nodes of the list, the walked total
    # is the lists' length, and the map is clean again
    info = []
    for s in range(args.num_batches):
        induced(s)
        closure_hop(s)
        torch.cuda.synchronize()
        m, w = counts.cpu().tolist()
        assert w == walked[s] and m <= cap
        e = eid[:m].long()
        e = torch.where(e < 0, e + (1 << 32), e)
        t = lists[s]
        assert bool((g.indices[e] == t[row[:m].long()]).all()), "an induced edge does not name its edge"
        assert bool((g.indptr[t[col[:m].long()].long()].long() <= e).all())
        claimed = int(hops[2].item())
        n = t.numel()
        info.append(dict(nodes=n, walked=w, induced=m, claimed=claimed,
                         leaf_bytes=2 * 8 * w + (3 * 8 + 4 * 4) * n + 12 * m, closure_bytes=8 * w + 8 * n + 8 * claimed))
    assert not bool((local_of != -1).any()), "the map is not clean"

    got = {"induced_us": [], "closure_us": []}
    for _ in range(args.rounds + 1):  # the first round warms up
        per = {k: [] for k in got}
        for s in range(args.num_batches):  # alternating, batch by batch
            per["induced_us"].append(timed(lambda: induced(s), args.steps))
            per["closure_us"].append(timed(lambda: closure_hop(s), args.steps))
        for k in got:
            got[k].append(float(np.mean(per[k])))
    mean = lambda k: float(np.mean([x[k] for x in info]))  # noqa: E731
    rec = dict(graph=args.graph, fanouts=fanouts, batch=args.batch, rounds=args.rounds, steps=args.steps,
               nodes=mean("nodes"), walked=mean("walked"), induced=mean("induced"), claimed=mean("claimed"),
               leaf_MB=round(mean("leaf_bytes") / 1e6, 3), closure_MB=round(mean("closure_bytes") / 1e6, 3))
    for k, v in got.items():
        rec[k] = round(float(np.median(v[1:])), 2)
        rec[k + "_rounds"] = [round(x, 2) for x in v[1:]]
    rec["leaf_GBps"] = round(rec["leaf_MB"] * 1e3 / rec["induced_us"], 1)
    rec["closure_GBps"] = round(rec["closure_MB"] * 1e3 / rec["closure_us"], 1)
    rec["induced_over_closure"] = round(rec["induced_us"] / rec["closure_us"], 3)
    rec["expectation"] = 2.2
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
