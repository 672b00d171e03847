"""ggms_gather_typed on sampled khop_typed + ggms_hetero_nodes batches, beside two yardsticks on the same GPU:
  (a) the torch formulation -- per type a slice of typed_nodes, the rank look-up and index_select on the type's table (what
      a user does above the engine when the typed tables live in torch);
  (b) the existing one-table gather over a table padded to the widest row (what a user of the one-table store does today).
Leaf and yardsticks alternate, batch by batch, inside every round of one session; medians of --rounds rounds.  The run first
checks that (a) and the leaf give the same bytes.

    python tools/bench_typed_feat.py --graph products --fanout 25,10 --tables mag240m
    python tools/bench_typed_feat.py --graph papers100M --fanout 5,10,15 --tables igb

T = 3 node types (a hash of the id).  Table sets: mag240m = one wide F16 type (768), two types without a table; igb = three
widths with mixed dtypes (1024 x F16, 128 x F32, 64 x BF16).  Tables hold random bits (never NaN-checked: rows are copied).
(b) is skipped, and reported as null, where the padded table does not fit beside the typed ones.

The engine's step with and without the key (each run its own process, on a dataset of tools/bench_hetero.py --make-dataset
to which --add-tables adds the typed tables):

    python tools/bench_typed_feat.py --add-tables DIR --tables mag240m
    python tools/bench_typed_feat.py --engine DIR --key on      # (and --key off)

One JSON line on stdout.  Algorithmic bytes of the leaf per row: 4 (id) + 4 (rank) + the table row + the output row; of (b):
4 + twice the padded row.  HBM peak taken as 8 TB/s (MI355X).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from xgnn_amd import datagen, ops  # noqa: E402
from xgnn_amd._lib import COUNT_INPUT, COUNT_STATUS  # noqa: E402
from bench_hetero import ENGINE_TYPE_FANOUT, quarter_types, split, timed, to_dev  # noqa: E402

R, T = 4, 3
HBM_PEAK_GBPS = 8000.0
TABLE_SETS = {"mag240m": [(768, torch.float16), None, None],
              "igb": [(1024, torch.float16), (128, torch.float32), (64, torch.bfloat16)]}
NP_OF = {torch.float16: np.float16, torch.float32: np.float32}


def add_tables(path, which):
    """node_feat_<t>.bin and the meta keys for a dataset that has node types already (bfloat16 written as float16 bits)."""
    meta = dict(line.rstrip("\n").split("\t") for line in open(os.path.join(path, "meta.txt")))
    nt = np.fromfile(os.path.join(path, "node_type.bin"), np.uint8)
    assert int(meta["NUM_NODE_TYPE"]) == T
    with open(os.path.join(path, "meta.txt"), "a") as f:
        for t, spec in enumerate(TABLE_SETS[which]):
            rows = int((nt == t).sum())
            if spec is not None:
                bits = np.random.RandomState(t).randint(0, 1 << 15, (rows, spec[0] * spec[1].itemsize // 2)).astype(np.uint16)
                bits.tofile(os.path.join(path, f"node_feat_{t}.bin"))
            f.write(f"NODE_FEAT_DIM_{t}\t{spec[0] if spec else 0}\n")
            name = {torch.float16: "F16", torch.float32: "F32", torch.bfloat16: "BF16"}[spec[1]] if spec else "F32"
            f.write(f"NODE_FEAT_DATA_TYPE_{t}\t{name}\n")
    print(json.dumps(dict(dataset=path, tables=which)), flush=True)


def engine_run(path, key, batch, steps, warmup):
    import time
    import samgraph.torch as sam
    cfg = {"dataset_path": path, "_arch": sam.builtin_archs["arch1"]["arch"], "_sample_type": sam.sample_types["khop_typed"],
           "type_fanout": ENGINE_TYPE_FANOUT, "batch_size": batch, "num_epoch": 1, "_cache_policy": sam.cache_policies["degree"],
           "cache_percentage": 0.0, "max_sampling_jobs": 10, "max_copying_jobs": 1, "omp_thread_num": 4, "num_layer": 2,
           "num_hidden": 64, "lr": 0.003, "dropout": 0.0, "sampler_ctx": "cuda:0", "trainer_ctx": "cuda:0", "seed": 1,
           "hetero_batch": "on", "typed_feat": key}
    sam.config(cfg)
    sam.init()
    times = []
    for i in range(warmup + steps):
        torch.cuda.synchronize()
        t0 = time.time()
        sam.sample_once()
        k = sam.get_next_batch()
        rows = [sam.get_graph_feat_of_type(k, t) for t in range(T)]
        torch.cuda.synchronize()
        times.append((time.time() - t0) * 1e3)
    print(json.dumps(dict(engine=path, typed_feat=key, batch=batch, steps=steps,
                          step_ms=round(float(np.median(times[warmup:])), 4), rows=[int(r.shape[0]) for r in rows],
                          dims=[int(r.shape[1]) for r in rows])), flush=True)
    sam.shutdown()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--add-tables", default=None, metavar="DIR")
    ap.add_argument("--engine", default=None, metavar="DIR")
    ap.add_argument("--key", default="on", choices=["on", "off"])
    ap.add_argument("--tables", default="mag240m", choices=sorted(TABLE_SETS))
    ap.add_argument("--graph", default="products", choices=["products", "papers100M", "tiny"])
    ap.add_argument("--fanout", default="25,10")
    ap.add_argument("--batch", type=int, default=8000)
    ap.add_argument("--num-batches", type=int, default=4)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seed", type=int, default=42)
    args = ap.parse_args()
    if args.add_tables:
        return add_tables(args.add_tables, args.tables)
    assert torch.cuda.is_available(), "bench_typed_feat needs a GPU"
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
    # a node's rank inside its type, and the tables (random bits)
    rank = torch.empty(num_node, dtype=torch.int32, device=dev)
    specs, tables, rows_of = TABLE_SETS[args.tables], [], []
    for t in range(T):
        at = (node_type == t).nonzero().squeeze(1)
        rank[at] = torch.arange(at.numel(), dtype=torch.int32, device=dev)
        rows_of.append(at.numel())
        if specs[t] is None:
            tables.append(None)
        else:
            dim, dt = specs[t]
            tables.append(torch.randint(0, 1 << 15, (at.numel(), dim * dt.itemsize // 2), dtype=torch.int16, device=dev).view(dt))
        del at
    del ids
    c_tables = ops.typed_tables(tables)
    widest = max(s[0] * s[1].itemsize for s in specs if s is not None)
    padded = None
    if torch.cuda.mem_get_info()[0] > num_node * widest + (8 << 30):
        padded = torch.empty((num_node, widest // 4), dtype=torch.float32, device=dev)
    fanouts = [int(x) for x in args.fanout.split(",")]
    L = len(fanouts)
    bs = ops.TypedBatchSampler(g, et, [split(k, R) for k in fanouts], args.batch, device=dev)
    batches = []
    for s in range(args.num_batches):
        bs.sample(to_dev(train[s * args.batch:(s + 1) * args.batch], dev), salt=1000 + s)
        res = bs.result()
        assert bs.counts.cpu().tolist()[COUNT_STATUS(L)] == 0
        nodes = res["input_nodes"].clone()
        het = ops.hetero_nodes(node_type, T, nodes)
        torch.cuda.synchronize()
        batches.append(dict(nodes=nodes, typed=het["typed_nodes"], base=het["base"], base_host=het["base"].cpu().tolist()))
    max_nodes = max(b["nodes"].numel() for b in batches)
    out = torch.empty(ops.gather_typed_out_bytes(c_tables, T, max_nodes), dtype=torch.uint8, device=dev)
    off = torch.empty(T + 1, dtype=torch.int64, device=dev)
    out_b = torch.empty((max_nodes, widest // 4), dtype=torch.float32, device=dev)

    def leaf(b):
        ops.gather_typed(c_tables, T, b["typed"], b["base"], row_of_node=rank, num_node=num_node,
                         max_nodes=b["nodes"].numel(), out=out, offsets=off)

    def torch_typed(b):  # (a): the slices' bounds are host integers, as a user has them
        res = []
        for t in range(T):
            if tables[t] is not None:
                sl = b["typed"][b["base_host"][t]:b["base_host"][t + 1]].long()
                res.append(torch.index_select(tables[t], 0, rank[sl].long()))
        return res

    def one_table(b):  # (b)
        ops.extract(padded, b["typed"][:b["nodes"].numel()], out=out_b[:b["nodes"].numel()])

    for b in batches:  # correct before fast
        leaf(b)
        want = torch_typed(b)
        torch.cuda.synchronize()
        o, k = off.cpu().tolist(), 0
        for t in range(T):
            if tables[t] is not None:
                nb = want[k].numel() * want[k].element_size()
                assert torch.equal(out[o[t]:o[t] + nb], want[k].contiguous().view(torch.uint8).reshape(-1)), f"type {t}"
                k += 1

    got = {"leaf_us": [], "torch_us": [], "one_table_us": []}
    for _ in range(args.rounds + 1):  # the first round warms up
        per = {k: [] for k in got}
        for b in batches:  # alternating, batch by batch
            per["leaf_us"].append(timed(lambda: leaf(b), args.steps))
            per["torch_us"].append(timed(lambda: torch_typed(b), args.steps))
            if padded is not None:
                per["one_table_us"].append(timed(lambda: one_table(b), args.steps))
        for k in got:
            got[k].append(float(np.mean(per[k])) if per[k] else None)
    cnt = np.mean([[b["base_host"][t + 1] - b["base_host"][t] for t in range(T)] for b in batches], axis=0)
    rb = [0 if s is None else s[0] * s[1].itemsize for s in specs]
    leaf_bytes = float(sum(c * (8 + 2 * r) for c, r in zip(cnt, rb) if r))
    nodes = float(np.mean([b["nodes"].numel() for b in batches]))
    rec = dict(graph=args.graph, fanouts=fanouts, batch=args.batch, tables=args.tables, rounds=args.rounds, steps=args.steps,
               nodes=int(nodes), per_type=[int(c) for c in cnt], row_bytes=rb, leaf_MB=round(leaf_bytes / 1e6, 3),
               one_table_MB=round(nodes * (4 + 2 * widest) / 1e6, 3))
    for k, v in got.items():
        rec[k] = None if v[1] is None else round(float(np.median(v[1:])), 2)
        rec[k + "_rounds"] = None if v[1] is None else [round(x, 2) for x in v[1:]]
    rec["leaf_GBps"] = round(rec["leaf_MB"] * 1e3 / rec["leaf_us"], 1)
    rec["leaf_share_of_peak"] = round(rec["leaf_GBps"] / HBM_PEAK_GBPS, 3)
    rec["torch_over_leaf"] = round(rec["torch_us"] / rec["leaf_us"], 3)
    rec["one_table_over_leaf"] = None if rec["one_table_us"] is None else round(rec["one_table_us"] / rec["leaf_us"], 3)
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
