"""The typed link front (ggms_link_seeds_typed) next to the untyped one (ggms_link_seeds), timed on one GPU.

    python tools/bench_link_typed.py --graph products [--baseline-lib PATH/libggms_hip.so]
    python tools/bench_link_typed.py --graph hub      # 10^6 nodes of degree 50, node 0 with 10^6 neighbours, 40 of them of
                                                      # the last type: one positive of the batch lies in that segment

The node types are ranges of the node id (T = 3; hub: the last 40 ids are type 2) and every list is sorted by id, so it is
sorted by relation = type(owner) * T + type(entry) as well.  Both leaves run over the SAME positives, in alternation
inside every round: `--steps` launches back to back between two events, `--rounds` rounds, median [min, max] in us
(host issue time included).  --baseline-lib: take ggms_link_seeds from another build of the library (the parent
commit's); without it, from this build.  One JSON line per (B, K) on stdout.
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
T = 3


def typed_graph(name, seed):
    from bench_link import make_graph
    g = make_graph(name, seed)
    ip, ix = g["indptr"], g["indices"]
    N = ip.size - 1
    cuts = np.array([0, N // 2, N - 40, N] if name == "hub" else [0, N // 2, N * 4 // 5, N])
    owner = np.repeat(np.arange(N, dtype=np.uint64), np.diff(ip.astype(np.int64)))
    ix = (np.sort((owner << np.uint64(32)) | ix) & np.uint64(0xFFFFFFFF)).astype(np.uint32)  # every list ascending
    nt = (np.searchsorted(cuts, np.arange(N), side="right") - 1).astype(np.uint8)
    et = (nt[owner.astype(np.int64)] * T + nt[ix]).astype(np.uint8)
    return ip, ix, et, nt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graph", default="products", choices=["tiny", "products", "hub"])
    ap.add_argument("--batch", type=int, nargs="+", default=[1000, 8000])
    ap.add_argument("--num-negative", type=int, nargs="+", default=[1, 5])
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--baseline-lib", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import torch
    from bench_link import timed
    from xgnn_amd import ops
    from xgnn_amd._lib import SYMBOLS, check, lib
    ip, ix, et, nt = typed_graph(args.graph, args.seed)
    dev = torch.device("cuda", 0)
    to_dev = lambda a: torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(dev)  # noqa: E731
    graph = ops.DeviceGraph(to_dev(ip), to_dev(ix))
    d_et, d_nt = to_dev(et), to_dev(nt)
    nodes, base = ops.type_lists(d_nt, T)
    untyped = lib().ggms_link_seeds
    if args.baseline_lib:
        untyped = C.CDLL(args.baseline_lib).ggms_link_seeds
        untyped.restype, untyped.argtypes = SYMBOLS["ggms_link_seeds"]
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    rng = np.random.RandomState(args.seed)
    E = int(ip[-1])
    for B in args.batch:
        eids = rng.randint(int(ip[1]) if args.graph == "hub" else 0, E, B).astype(np.uint32)
        if args.graph == "hub":  # a position of node 0's segment of the last type: its last entry
            eids[B // 2] = int(ip[1]) - 1
        t_eids = to_dev(eids)
        for K in args.num_negative:
            out = torch.empty(B * (2 + K), dtype=torch.int32, device=dev)
            rel = torch.empty(B, dtype=torch.uint8, device=dev)
            forced = torch.zeros(1, dtype=torch.int64, device=dev)
            rec = dict(graph=args.graph, num_node=ip.size - 1, num_edge=E, B=B, K=K, steps=args.steps, rounds=args.rounds,
                       baseline=args.baseline_lib or "this build")
            for mname, mode in (("uniform", 0), ("exclude", 1)):
                def plain():
                    check(untyped(C.byref(graph.c), ptr(t_eids), B, K, mode, 99, ptr(out), ptr(forced), stream), "link_seeds")

                def typed():
                    check(lib().ggms_link_seeds_typed(C.byref(graph.c), ptr(d_et), ptr(d_nt), ptr(nodes), ptr(base), T,
                                                      ptr(t_eids), B, K, mode + 2, 99, ptr(out), ptr(rel), ptr(forced),
                                                      stream), "link_seeds_typed")
                plain(), typed()
                us = np.array([(timed(plain, args.steps), timed(typed, args.steps)) for _ in range(args.rounds)])
                stat = lambda c: [round(float(x), 2) for x in (np.median(us[:, c]), us[:, c].min(), us[:, c].max())]  # noqa: E731
                rec[mname] = dict(link_seeds_us=stat(0), link_seeds_typed_us=stat(1))
            assert ops.device_status() == 0
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
