"""ggms_hetero_nodes + ggms_hetero_edges on sampled khop_typed batches, beside the torch formulation of the same outputs on
the same GPU -- what a user runs above the engine today: the type look-up, torch.sort(stable=True) of the nodes and of every
layer's edges, bincounts, and the index_selects through the rank map.  The yardstick shares no code with the leaves.  The
two alternate, batch by batch, inside every round of one session.

    python tools/bench_hetero.py --graph products --fanout 25,10
    python tools/bench_hetero.py --graph papers100M --fanout 5,10,15

R = 4 relations (a list's quarters: sorted by construction, a function of the entry's rank in its list), T = 3 node types
(a hash of the id).  The leaves do not look at whether relations and node types agree, so neither does this tool.
The engine's step with and without the key, and what the key adds to the load (each run its own process):

    python tools/bench_hetero.py --make-dataset DIR       # products-sized, T = 3, the 9 relations of the node types
    python tools/bench_hetero.py --engine DIR --key on    # (and --key off): ms per step of sample_once + get_next_batch

One JSON line on stdout; times are medians over --rounds of the mean of --steps back-to-back calls (buffers and workspaces
allocated once, outside the timed region; the torch side allocates its results as torch does; the leaf side has no host
synchronisation inside the timed region, the torch side none either -- the cuts are host integers, as a user has them).
Algorithmic bytes of the leaves: 23 B per node (id and type read, type written and read again, id read again, local / slot /
typed id written), 34 B per edge (row, col, eid and the type twice read, two 4-byte look-ups, three words written).
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
from xgnn_amd._lib import COUNT_DST, COUNT_EDGES, COUNT_INPUT, COUNT_SRC, COUNT_STATUS, COUNTS_WORDS  # noqa: E402

R, T = 4, 3


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


def split(k, r):
    return [k // r + (1 if i < k % r else 0) for i in range(r)]


def quarter_types(g, dev):
    """type = 4 * rank / degree of every list entry, chunk by chunk (no E-sized int64 temporaries)"""
    ip64 = g.indptr.long()
    ip64 = torch.where(ip64 < 0, ip64 + (1 << 32), ip64)  # (indptr holds uint32 bits)
    deg = ip64[1:] - ip64[:-1]
    et = torch.empty(int(ip64[-1]), dtype=torch.uint8, device=dev)
    n, step = deg.numel(), 1 << 22
    for lo in range(0, n, step):
        hi = min(n, lo + step)
        b, e = int(ip64[lo]), int(ip64[hi])
        if e > b:
            d = torch.repeat_interleave(deg[lo:hi], deg[lo:hi])
            rank = torch.arange(b, e, device=dev) - torch.repeat_interleave(ip64[lo:hi], deg[lo:hi])
            et[b:e] = (rank * R // d).to(torch.uint8)
            del d, rank
    return et


def torch_hetero(node_type, batch):
    """The same outputs with torch operators (what a trainer does above the engine today)."""
    nodes, L = batch["nodes"], len(batch["rows"])
    nt = node_type[nodes.long()]
    _, order = torch.sort(nt, stable=True)
    typed_nodes = nodes[order]
    base = torch.cumsum(torch.bincount(nt, minlength=T), 0) - torch.bincount(nt, minlength=T)
    slot = torch.empty_like(order)
    slot[order] = torch.arange(order.numel(), device=order.device)
    local = slot - base[nt.long()]
    cut_counts = torch.stack([torch.bincount(nt[:c], minlength=T) for c in batch["cuts"]])
    out = []
    for i in range(L):
        et = batch["etypes"][i]
        _, idx = torch.sort(et, stable=True)
        off = torch.cumsum(torch.bincount(et, minlength=R), 0)
        out.append((torch.index_select(local, 0, torch.index_select(batch["rows"][i], 0, idx).long()),
                    torch.index_select(local, 0, torch.index_select(batch["cols"][i], 0, idx).long()),
                    torch.index_select(batch["eids"][i], 0, idx), off))
    return dict(ntype=nt, local=local, slot=slot, typed_nodes=typed_nodes, base=base, cut_counts=cut_counts, layers=out)


ENGINE_TYPE_FANOUT = [[3, 3, 3, 3, 3, 3, 3, 2, 2], [2, 1, 1, 1, 1, 1, 1, 1, 1]]  # by layer id: 25 and 10


def make_dataset(path, preset, seed):
    """A typed dataset without a sort: node type = id % 3; an entry of rank j in a list of degree d gets the source type
    3 j / d -- its id is moved to the nearest id of that type -- so every list is sorted by relation as it is drawn."""
    gr = datagen.make_graph(preset, seed=seed)
    ip, ix = gr["indptr"].astype(np.int64), gr["indices"]
    n = ip.size - 1
    deg = np.diff(ip)
    et = np.empty(ix.size, np.uint8)
    step = 1 << 20
    for lo in range(0, n, step):  # chunked: no E-sized int64 temporaries
        hi = min(n, lo + step)
        b, e = int(ip[lo]), int(ip[hi])
        if e > b:
            d = np.repeat(deg[lo:hi], deg[lo:hi])
            rank = np.arange(b, e) - np.repeat(ip[lo:hi], deg[lo:hi])
            src_t = rank * T // d
            ids = ix[b:e].astype(np.int64)
            ids = np.minimum(ids - ids % T + src_t, n - 1 - (n - 1 - src_t) % T)  # the same type, below n
            ix[b:e] = ids.astype(np.uint32)
            et[b:e] = ((np.repeat(np.arange(lo, hi), deg[lo:hi]) % T) * T + src_t).astype(np.uint8)
    nt = (np.arange(n) % T).astype(np.uint8)
    dim = 32
    gr["meta"] = dict(gr["meta"], feat_dim=dim, num_class=47)
    feat = (np.arange(n, dtype=np.int64)[:, None] * dim + np.arange(dim)[None, :]).astype(np.float32)
    datagen.write_dataset(path, gr, feat=feat, label=np.arange(n) % 47, minimal=True, edge_type=et, num_edge_type=T * T,
                          node_type=nt, num_node_type=T)
    print(json.dumps(dict(dataset=path, num_node=int(n), num_edge=int(ix.size))), flush=True)


def engine_run(path, key, batch, steps, warmup):
    import time
    import samgraph.torch as sam
    cfg = {"dataset_path": path, "_arch": sam.builtin_archs["arch1"]["arch"], "_sample_type": sam.sample_types["khop_typed"],
           "type_fanout": ENGINE_TYPE_FANOUT, "batch_size": batch, "num_epoch": 1, "_cache_policy": sam.cache_policies["degree"],
           "cache_percentage": 0.0, "max_sampling_jobs": 10, "max_copying_jobs": 1, "omp_thread_num": 4, "num_layer": 2,
           "num_hidden": 64, "lr": 0.003, "dropout": 0.0, "sampler_ctx": "cuda:0", "trainer_ctx": "cuda:0", "seed": 1}
    if key == "on":
        cfg["hetero_batch"] = "on"
    sam.config(cfg)
    t0 = time.time()
    sam.data_init()
    load_s = time.time() - t0
    sam.sample_init(0, "cuda:0")
    sam.train_init(0, "cuda:0")
    assert sam.steps_per_epoch() >= warmup + steps
    times = []
    for i in range(warmup + steps):
        torch.cuda.synchronize()
        t0 = time.time()
        sam.sample_once()
        k = sam.get_next_batch()
        rows = sam.get_graph_feat(k)
        torch.cuda.synchronize()
        times.append((time.time() - t0) * 1e3)
    rec = dict(engine=path, key=key, batch=batch, steps=steps, load_s=round(load_s, 3),
               step_ms=round(float(np.median(times[warmup:])), 4), step_ms_mean=round(float(np.mean(times[warmup:])), 4),
               rows=int(rows.shape[0]))
    print(json.dumps(rec), flush=True)
    sam.shutdown()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--make-dataset", default=None, metavar="DIR")
    ap.add_argument("--engine", default=None, metavar="DIR")
    ap.add_argument("--key", default="on", choices=["on", "off"])
    ap.add_argument("--graph", default="products", choices=["products", "papers100M", "tiny"])
    ap.add_argument("--fanout", default="25,10")
    ap.add_argument("--batch", type=int, default=8000)
    ap.add_argument("--num-batches", type=int, default=4)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seed", type=int, default=42)
    args = ap.parse_args()
    if args.make_dataset:
        return make_dataset(args.make_dataset, args.graph, args.seed)
    assert torch.cuda.is_available(), "bench_hetero needs a GPU"
    if args.engine:
        return engine_run(args.engine, args.key, args.batch, 16, 4)
    dev = torch.device("cuda", 0)
    gr = datagen.make_graph(args.graph, seed=args.seed)
    train = gr["train_set"]
    g = ops.DeviceGraph(to_dev(gr["indptr"], dev), to_dev(gr["indices"], dev), inline_heads=False)
    num_node = int(gr["indptr"].size - 1)
    del gr
    et = quarter_types(g, dev)
    ids = torch.arange(num_node, device=dev)
    node_type = ((ids * 2654435761) >> 7).remainder(T).to(torch.uint8)
    del ids
    fanouts = [int(x) for x in args.fanout.split(",")]
    L = len(fanouts)
    bs = ops.TypedBatchSampler(g, et, [split(k, R) for k in fanouts], args.batch, device=dev)
    batches = []
    for s in range(args.num_batches):
        bs.sample(to_dev(train[s * args.batch:(s + 1) * args.batch], dev), salt=1000 + s)
        res = bs.result()
        c = bs.counts.cpu().tolist()
        assert c[COUNT_STATUS(L)] == 0
        counts = torch.zeros(COUNTS_WORDS(L), dtype=torch.int64, device=dev)
        counts[:bs.counts.numel()] = bs.counts
        batches.append(dict(nodes=res["input_nodes"].clone(), counts=counts,
                            rows=[lay["row"].clone() for lay in res["layers"]],
                            cols=[lay["col"].clone() for lay in res["layers"]],
                            eids=[lay["eid"].clone() for lay in res["layers"]],
                            etypes=[lay["etype"].clone() for lay in res["layers"]],
                            cuts=[int(c[COUNT_SRC(i)]) for i in range(L)] + [int(c[COUNT_DST(L - 1)])],
                            cut_words=[COUNT_SRC(i) for i in range(L)] + [COUNT_DST(L - 1)],
                            edges=[int(c[COUNT_EDGES(i)]) for i in range(L)]))
    max_nodes = max(b["nodes"].numel() for b in batches)
    max_edges = [max(b["edges"][i] for b in batches) for i in range(L)]
    # the leaves' buffers and their one workspace, allocated once
    node_out = dict(ntype=torch.empty(max_nodes, dtype=torch.uint8, device=dev),
                    base=torch.empty(T + 1, dtype=torch.int32, device=dev),
                    cut_counts=torch.empty((L + 1, T), dtype=torch.int32, device=dev))
    for name in ("local", "slot", "typed_nodes"):
        node_out[name] = torch.empty(max_nodes, dtype=torch.int32, device=dev)
    edge_out = tuple([torch.empty(max(m, 4), dtype=torch.int32, device=dev) for m in max_edges] for _ in range(3))
    rel_off = torch.empty((L, R + 1), dtype=torch.int32, device=dev)
    from xgnn_amd._lib import lib
    import ctypes as C
    need = max(lib().ggms_hetero_nodes_workspace_bytes(max_nodes, T),
               lib().ggms_hetero_edges_workspace_bytes((C.c_size_t * L)(*max_edges), L, R))
    ws = torch.empty(need // 4 + 4, dtype=torch.int32, device=dev)

    def leaf(b):
        n = b["nodes"].numel()
        ops.hetero_nodes(node_type, T, b["nodes"], num_nodes_dev=b["counts"][COUNT_INPUT(L):COUNT_INPUT(L) + 1],
                         cut_base=b["counts"], cut_words=b["cut_words"], max_nodes=n, out=node_out, workspace=ws)
        ops.hetero_edges(b["rows"], b["cols"], b["etypes"], R, b["counts"], node_out["local"][:n], eids=b["eids"],
                         max_edges=b["edges"], out=edge_out, rel_offsets=rel_off, workspace=ws)

    # correct before fast: the two formulations agree, array for array
    for b in batches:
        leaf(b)
        want = torch_hetero(node_type, b)
        torch.cuda.synchronize()
        n = b["nodes"].numel()
        for name in ("ntype", "local", "slot", "typed_nodes"):
            assert torch.equal(node_out[name][:n].long(), want[name].long()), name
        assert torch.equal(node_out["base"][:T].long(), want["base"]) and torch.equal(node_out["cut_counts"].long(), want["cut_counts"])
        for i, (w_row, w_col, w_eid, w_off) in enumerate(want["layers"]):
            m = b["edges"][i]
            assert torch.equal(edge_out[0][i][:m], w_row.int()) and torch.equal(edge_out[1][i][:m], w_col.int())
            assert torch.equal(edge_out[2][i][:m], w_eid) and torch.equal(rel_off[i, 1:].long(), w_off)

    got = {"leaf_us": [], "leaf_nodes_us": [], "torch_us": []}
    for _ in range(args.rounds + 1):  # the first round warms up
        per = {k: [] for k in got}
        for b in batches:  # alternating, batch by batch
            per["leaf_us"].append(timed(lambda: leaf(b), args.steps))
            per["torch_us"].append(timed(lambda: torch_hetero(node_type, b), args.steps))
            n = b["nodes"].numel()
            per["leaf_nodes_us"].append(timed(lambda: ops.hetero_nodes(
                node_type, T, b["nodes"], num_nodes_dev=b["counts"][COUNT_INPUT(L):COUNT_INPUT(L) + 1], cut_base=b["counts"],
                cut_words=b["cut_words"], max_nodes=n, out=node_out, workspace=ws), args.steps))
        for k in got:
            got[k].append(float(np.mean(per[k])))
    nodes = float(np.mean([b["nodes"].numel() for b in batches]))
    edges = float(np.mean([sum(b["edges"]) for b in batches]))
    rec = dict(graph=args.graph, fanouts=fanouts, batch=args.batch, rounds=args.rounds, steps=args.steps, R=R, T=T,
               nodes=int(nodes), edges=int(edges), leaf_MB=round((23 * nodes + 34 * edges) / 1e6, 3))
    for k, v in got.items():
        rec[k] = round(float(np.median(v[1:])), 2)
        rec[k + "_rounds"] = [round(x, 2) for x in v[1:]]
    rec["leaf_GBps"] = round(rec["leaf_MB"] * 1e3 / rec["leaf_us"], 1)
    rec["torch_over_leaf"] = round(rec["torch_us"] / rec["leaf_us"], 3)
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
