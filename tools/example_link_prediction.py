"""Link prediction with GraphSAGE on batches from the samgraph_* engine (task = link_prediction), in plain PyTorch-ROCm.

tools/example_train_sage.py's DGL-free model; the head is a dot product of the two endpoints' embeddings, trained with
binary cross-entropy over the batch's positive pairs (label 1) and negative pairs (label 0).  A usage example of the
pair interface, not a tuned model:

    sam.config({..., "task": "link_prediction", "num_negative": K, "negative_mode": "exclude",
                "exclude_seed_edges": "both"})   # the positives and their mirrors leave the sampled layers
    pos_src, pos_dst, neg_src, neg_dst = sam.get_graph_link_pairs(key)   # local ids: rows of the model's output

batch_size counts positive EDGES; the batch's seed list is their B (2 + K) endpoints, so the first sampled layer's
num_dst is B (2 + K) while the distinct endpoints are the first max(id) + 1 nodes of the batch.

    python tools/example_link_prediction.py <dataset_dir> [--epochs 2] [--batch-size 512] [--num-negative 3]
        [--exclude-seed-edges none|self|both] [--learn-features sgd|adagrad --feat-lr 0.05] [--edge-weight]
        [--temporal [--temporal-pick uniform|recent]]

--learn-features makes the engine's feature table the model's trainable input embedding (config keys feat_learnable,
feat_lr): the batch's rows become a leaf that requires grad, and after backward() their gradient goes back with
sam.update_graph_feat(key, h.grad) -- the table moves on the device, no copy of it lives in torch.  The rows are used
as they are (no 1 / 65536): give such a dataset a feat.bin that is an embedding's initial value, small random numbers.

--edge-weight reads the dataset's edge table (config key edge_feat; datagen.write_dataset(..., edge_feat=...)): column 0
of sam.get_graph_edge_feat(key, i), the row of every sampled edge of layer i, scales that edge's message, and the mean
becomes the weighted mean.  sam.get_graph_edge_ids(key, i) are the ids the rows were gathered under -- what a model with
its own per-edge parameters would index them with -- and sam.get_graph_link_edge_ids(key) those of the positives.

--temporal samples with sample_type khop_temporal on a dataset that carries edge_time.bin (datagen.write_dataset(...,
edge_time=...)): every endpoint of a positive is sampled strictly before the positive's time, so exclude_seed_edges is
none.  The age of every sampled edge, dt = sam.get_graph_node_cut(key)[col] - sam.get_graph_edge_time(key, i), is the
model's edge input: a message is scaled by 1 / (1 + log(1 + dt)), recent interactions count more.
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import samgraph.torch as sam  # noqa: E402
from example_train_sage import SageLayer  # noqa: E402


class WeightedSageLayer(SageLayer):
    """SageLayer whose neighbour term is the mean weighted by a scalar per edge."""

    def forward(self, h, row, col, num_dst, weight):
        agg = torch.zeros((num_dst, h.shape[1]), dtype=h.dtype, device=h.device)
        total = torch.zeros(num_dst, dtype=h.dtype, device=h.device)
        agg.index_add_(0, col, h[row] * weight.unsqueeze(1))
        total.index_add_(0, col, weight)
        return self.w_self(h[:num_dst]) + self.w_nbr(agg / total.clamp(min=1e-12).unsqueeze(1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("dataset")
    ap.add_argument("--epochs", type=int, default=2)
    ap.add_argument("--batch-size", type=int, default=512, help="positive edges per batch")
    ap.add_argument("--num-negative", type=int, default=3)
    ap.add_argument("--negative-mode", default="exclude", choices=["uniform", "exclude"])
    ap.add_argument("--exclude-seed-edges", default="both", choices=["none", "self", "both"],
                    help="take the batch's positive edges (self), and their mirrors (both), out of the sampled layers")
    ap.add_argument("--fanout", type=int, nargs="+", default=[10, 5])
    ap.add_argument("--sample-type", default="khop3")
    ap.add_argument("--hidden", type=int, default=64)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--learn-features", choices=["sgd", "adagrad"],
                    help="train the feature table itself with this rule (config key feat_learnable)")
    ap.add_argument("--feat-lr", type=float, default=0.05, help="learning rate of the feature table (feat_lr)")
    ap.add_argument("--edge-weight", action="store_true",
                    help="scale every message by column 0 of the edge's row of the dataset's edge table (edge_feat)")
    ap.add_argument("--temporal", action="store_true",
                    help="sample_type khop_temporal: neighbours from strictly before each positive's time (edge_time.bin)")
    ap.add_argument("--temporal-pick", default="uniform", choices=["uniform", "recent"])
    args = ap.parse_args()
    L = len(args.fanout)
    edge = {"edge_feat": "on"} if args.edge_weight else {}
    if args.temporal:  # strictly-before already removes the positive, its mirror at the same time, and everything later
        args.sample_type, args.exclude_seed_edges = "khop_temporal", "none"
        edge["temporal_pick"] = args.temporal_pick
    learn = {"feat_learnable": args.learn_features, "feat_lr": args.feat_lr} if args.learn_features else {}
    sam.config({**learn, **edge, "dataset_path": args.dataset, "_arch": sam.builtin_archs["arch1"]["arch"],
                "_sample_type": sam.sample_types[args.sample_type], "batch_size": args.batch_size,
                "num_epoch": args.epochs, "_cache_policy": sam.cache_policies["degree"], "cache_percentage": 0.0,
                "max_sampling_jobs": 10, "max_copying_jobs": 1, "omp_thread_num": 4, "num_layer": L,
                "num_hidden": args.hidden, "lr": 0.003, "dropout": 0.0, "num_fanout": L, "fanout": args.fanout,
                "sampler_ctx": "cuda:0", "trainer_ctx": "cuda:0", "seed": args.seed,
                "task": "link_prediction", "num_negative": args.num_negative, "negative_mode": args.negative_mode,
                "exclude_seed_edges": args.exclude_seed_edges})
    sam.init()
    dev = torch.device("cuda", 0)
    torch.manual_seed(args.seed)
    dims = [sam.feat_dim()] + [args.hidden] * L
    layers = torch.nn.ModuleList([(WeightedSageLayer if edge else SageLayer)(dims[i], dims[i + 1]) for i in range(L)]).to(dev)
    opt = torch.optim.Adam(layers.parameters(), lr=0.003)
    steps = sam.steps_per_epoch()
    for epoch in range(args.epochs):
        t0, pairs, loss_sum, hits, excluded = time.time(), 0, 0.0, 0, 0
        for step in range(steps):
            sam.sample_once()
            key = sam.get_next_batch()
            pos_src, pos_dst, neg_src, neg_dst = (t.long() for t in sam.get_graph_link_pairs(key))
            num_out = int(sam.get_graph_seed_ids(key).max()) + 1  # distinct endpoints: the first nodes of the batch
            if learn:  # the rows as they are: a leaf whose gradient goes back to the table
                h = feat = sam.get_graph_feat(key).requires_grad_()
            else:
                h = sam.get_graph_feat(key) / 65536.0  # the synthetic features are integers in [0, 65535]
            coo = sam.get_graph_coo(key, L)  # layer 0 = outermost hop (largest frontier)
            for i in range(L):
                row, col, num_src, num_dst = coo[i]
                assert h.shape[0] == num_src
                # (edge k of the layer is CSR position sam.get_graph_edge_ids(key, i)[k]; its row was gathered under that id)
                w = ()
                if args.edge_weight:
                    w = (sam.get_graph_edge_feat(key, i)[:, 0].float().abs(),)
                if args.temporal:  # the edge's age against the cut-off of the node it was sampled for (uint32 bits)
                    cut = sam.get_graph_node_cut(key).long() & 0xFFFFFFFF
                    dt = (cut[col.long()] - (sam.get_graph_edge_time(key, i).long() & 0xFFFFFFFF)).clamp(min=0).float()
                    decay = 1.0 / (1.0 + torch.log1p(dt))
                    w = (w[0] * decay if w else decay,)
                h = layers[i](h, row.long(), col.long(), num_dst if i + 1 < L else num_out, *w)
                if i + 1 < L:
                    h = torch.relu(h)
            pos = (h[pos_src] * h[pos_dst]).sum(1)
            neg = (h[neg_src] * h[neg_dst]).sum(2).flatten()
            score = torch.cat([pos, neg])
            target = torch.cat([torch.ones_like(pos), torch.zeros_like(neg)])
            loss = torch.nn.functional.binary_cross_entropy_with_logits(score, target)
            opt.zero_grad()
            loss.backward()
            opt.step()
            if learn:
                sam.update_graph_feat(key, feat.grad)
            pairs += score.numel()
            excluded += sam.get_graph_num_excluded(key)
            loss_sum += float(loss) * score.numel()
            hits += int(((score > 0) == (target > 0)).sum())
        print(f"epoch {epoch}: {steps} steps, loss {loss_sum / pairs:.4f}, pair acc {hits / pairs:.3f}, "
              f"{time.time() - t0:.2f} s, sampled {sam.get_log_epoch_value(epoch, sam.kLogEpochNumSample):.0f} edges, "
              f"{excluded} more excluded", flush=True)
    sam.shutdown()


if __name__ == "__main__":
    main()
