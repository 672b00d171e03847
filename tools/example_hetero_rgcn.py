"""A DGL-free R-GCN on heterogeneous batches, in plain torch, from the accessors of config key hetero_batch alone.

    python tools/example_hetero_rgcn.py [--dataset DIR] [--epochs 2] [--batch-size 256]

Without --dataset a typed dataset is generated first (datagen's `tiny` graph: 20 000 nodes of T = 3 types, the R = 9
relations of datagen.relation_types, lists sorted by relation, a label that depends on a node's type and on its own and
its neighbours' features).  The model keeps one hidden state per NODE TYPE; a layer has one weight per relation and one
self weight per type, and a relation's block is one gather, one matmul and one index_add_:

    out[dst_type(r)].index_add_(0, rel_col, (h[src_type(r)][rel_row] @ W_r) / degree)

The engine hands over everything the layer needs, already on the GPU: the rows grouped by type (get_graph_feat_of_type,
views of one buffer), the blocks with ids local to their types (get_graph_rel_row / _rel_col), and the per-type source /
destination counts of every layer.  A layer's destination nodes are the first num_dst_of_type nodes of each type's
group, so the next layer's input is the head of this layer's output -- no re-indexing between layers.  The seeds' logits
are read back through get_graph_node_type / get_graph_node_local of the first num_seeds input nodes.
--typed-feat: the dataset gets one feature table PER NODE TYPE (config key typed_feat): type 0 keeps the 16 float32
columns, type 1 gets 8 of them as float16, type 2 has no features at all.  The model then starts with a linear input
projection per type that has features -- get_graph_feat_of_type(key, t) is (nodes of the type, feat_dim_of_type(t)) in
feat_dtype_of_type(t) -- and an nn.Embedding indexed by typed_nodes for the type that has none.
Prints the loss of every epoch; it falls.
"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import samgraph.torch as sam  # noqa: E402
from xgnn_amd import datagen  # noqa: E402

T = 3
TYPE_FANOUT = [[2] * 9, [2] * 9]  # by layer id: every relation, two neighbours each


def make_dataset(path, seed=5, typed_feat=False):
    g = datagen.make_graph("tiny", seed=seed)
    ip, ix, n = g["indptr"], g["indices"], g["meta"]["num_node"]
    rng = np.random.RandomState(seed)
    nt = rng.choice(T, n, p=[0.5, 0.3, 0.2]).astype(np.uint8)
    ix, et, _ = datagen.sort_lists_by_type(ip, ix, datagen.relation_types(ip, ix, nt, T))
    g["indices"] = ix
    dim = 16
    feat = rng.random_sample((n, dim)).astype(np.float32)
    # the label: the node's type, one bit of its own features, one bit of its neighbourhood's mean
    owner = np.repeat(np.arange(n), np.diff(ip.astype(np.int64)))
    mean = np.bincount(owner, weights=feat[ix, 1], minlength=n) / np.maximum(np.diff(ip.astype(np.int64)), 1)
    label = nt.astype(np.int64) * 4 + (feat[:, 0] > 0.5) * 2 + (mean > 0.5)
    g["meta"] = dict(g["meta"], feat_dim=dim, num_class=4 * T)
    node_feat = [feat[nt == 0], feat[nt == 1][:, :8].astype(np.float16), None] if typed_feat else None
    datagen.write_dataset(path, g, feat=feat, label=label, minimal=True, edge_type=et, num_edge_type=T * T, node_type=nt,
                          num_node_type=T, node_feat=node_feat)
    return path


class TypedInput(torch.nn.Module):
    """typed_feat: a linear projection per type that has features, an embedding per node for a type that has none."""

    def __init__(self, dims, num_nodes, d_out):
        super().__init__()
        self.proj = torch.nn.ModuleList([torch.nn.Linear(d, d_out) if d else torch.nn.Embedding(num_nodes, d_out) for d in dims])
        self.dims = dims

    def forward(self, rows, typed_nodes):
        return [self.proj[t](rows[t].float()) if d else self.proj[t](typed_nodes[t].long()) for t, d in enumerate(self.dims)]


class RelLayer(torch.nn.Module):
    """One weight per relation, one self weight per node type; mean over a node's sampled in-edges of all relations."""

    def __init__(self, d_in, d_out, num_rel, num_type):
        super().__init__()
        self.rel = torch.nn.ParameterList([torch.nn.Parameter(torch.randn(d_in, d_out) * d_in ** -0.5) for _ in range(num_rel)])
        self.own = torch.nn.ModuleList([torch.nn.Linear(d_in, d_out) for _ in range(num_type)])

    def forward(self, h, blocks, num_dst):
        """h[t]: the layer's source rows of type t; blocks: (r, src_type, dst_type, rel_row, rel_col); num_dst[t]."""
        out = [self.own[t](h[t][:num_dst[t]]) for t in range(len(h))]
        deg = [torch.zeros(num_dst[t], device=h[t].device) for t in range(len(h))]
        for _, _, d, _, col in blocks:
            deg[d].index_add_(0, col, torch.ones(col.numel(), device=col.device))
        for r, s, d, row, col in blocks:
            msg = h[s][row] @ self.rel[r]
            out[d] = out[d].index_add(0, col, msg / deg[d][col].unsqueeze(1))
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dataset", default=None)
    ap.add_argument("--epochs", type=int, default=2)
    ap.add_argument("--batch-size", type=int, default=256)
    ap.add_argument("--hidden", type=int, default=64)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--typed-feat", action="store_true")
    args = ap.parse_args()
    tmp = None
    if args.dataset is None:
        tmp = tempfile.TemporaryDirectory()
        args.dataset = make_dataset(tmp.name, typed_feat=args.typed_feat)
    L, R = len(TYPE_FANOUT), len(TYPE_FANOUT[0])
    sam.config({"dataset_path": args.dataset, "_arch": sam.builtin_archs["arch1"]["arch"],
                "_sample_type": sam.sample_types["khop_typed"], "type_fanout": TYPE_FANOUT, "hetero_batch": "on",
                "batch_size": args.batch_size, "num_epoch": args.epochs, "_cache_policy": sam.cache_policies["degree"],
                "cache_percentage": 0.0, "max_sampling_jobs": 10, "max_copying_jobs": 1, "omp_thread_num": 4,
                "num_layer": L, "num_hidden": args.hidden, "lr": 0.003, "dropout": 0.0, "sampler_ctx": "cuda:0",
                "trainer_ctx": "cuda:0", "seed": args.seed, **({"typed_feat": "on"} if args.typed_feat else {})})
    sam.init()
    dev = torch.device("cuda", 0)
    torch.manual_seed(args.seed)
    num_type = sam.num_node_type()
    rel = [(r, sam.relation_src_type(r), sam.relation_dst_type(r)) for r in range(R)]
    rel = [x for x in rel if x[1] != 255]  # a relation without an edge has no signature
    dims = [args.hidden if args.typed_feat else sam.feat_dim()] + [args.hidden] * (L - 1) + [sam.num_class()]
    layers = torch.nn.ModuleList([RelLayer(dims[i], dims[i + 1], R, num_type) for i in range(L)]).to(dev)
    params = list(layers.parameters())
    if args.typed_feat:
        num_node = sam.get_dataset_label().numel()
        inp = TypedInput([sam.feat_dim_of_type(t) for t in range(num_type)], num_node, args.hidden).to(dev)
        params += list(inp.parameters())
    opt = torch.optim.Adam(params, lr=0.01)
    steps = sam.steps_per_epoch()
    losses = []
    for epoch in range(args.epochs):
        t0, total, correct, loss_sum = time.time(), 0, 0, 0.0
        for step in range(steps):
            sam.sample_once()
            key = sam.get_next_batch()
            h = [sam.get_graph_feat_of_type(key, t) for t in range(num_type)]  # views: a type's rows are one slice
            if args.typed_feat:
                h = [torch.relu(x) for x in inp(h, [sam.get_graph_typed_nodes(key, t) for t in range(num_type)])]
            for i in range(L):  # layer 0 = the outermost hop
                assert all(h[t].shape[0] >= sam.get_graph_num_src_of_type(key, i, t) for t in range(num_type))
                blocks = [(r, s, d, sam.get_graph_rel_row(key, i, r).long(), sam.get_graph_rel_col(key, i, r).long())
                          for r, s, d in rel if sam.get_graph_rel_num_edges(key, i, r)]
                h = layers[i](h, blocks, [sam.get_graph_num_dst_of_type(key, i, t) for t in range(num_type)])
                if i + 1 < L:
                    h = [torch.relu(x) for x in h]
            # the seeds are the first input nodes; their logits lie in their types' outputs at their ranks
            label = sam.get_graph_label(key)
            n = label.numel()
            ntype, local = sam.get_graph_node_type(key)[:n].long(), sam.get_graph_node_local(key)[:n].long()
            start = torch.tensor([0] + [x.shape[0] for x in h[:-1]], device=dev).cumsum(0)
            logits = torch.cat(h)[start[ntype] + local]
            loss = torch.nn.functional.cross_entropy(logits, label)
            opt.zero_grad()
            loss.backward()
            opt.step()
            total += n
            correct += int((logits.argmax(1) == label).sum())
            loss_sum += float(loss.detach()) * n
        losses.append(loss_sum / total)
        print(f"epoch {epoch}: {steps} steps, loss {losses[-1]:.4f}, train acc {correct / total:.3f}, "
              f"{time.time() - t0:.2f} s", flush=True)
    sam.shutdown()
    if tmp is not None:
        tmp.cleanup()
    if len(losses) > 1 and not losses[-1] < losses[0]:
        sys.exit(f"the loss did not fall: {losses}")


if __name__ == "__main__":
    main()
