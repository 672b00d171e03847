"""tests/typed_driver.py's run (link_driver.py's batches with edge ids, edge rows and edge types), with what
induced_subgraph = on adds to a batch: the induced COO, its edge ids and -- with edge_feat = on -- its edge rows.

    python tests/induced_driver.py <dataset_dir> <out_prefix> [probe=<accessor>] [extra k=v ...]

probe=<accessor>: the named accessor of samgraph.torch is called on the first batch whatever the configuration says (a
run without the key must die there, by name); the argument does not reach the configuration.
"""
import sys

PROBE = [a.split("=", 1)[1] for a in sys.argv[3:] if a.startswith("probe=")]
sys.argv = [a for a in sys.argv if not a.startswith("probe=")]

import link_driver  # noqa: E402
import typed_driver  # noqa: E402

ARGS = dict(a.split("=", 1) for a in sys.argv[3:])
INDUCED = ARGS.get("induced_subgraph") == "on"
FEAT = ARGS.get("edge_feat") == "on"


def record_batch(sam, key, num_layers, link):
    rec = typed_driver.record_batch(sam, key, num_layers, link)
    for name in PROBE:
        getattr(sam, name)(key)
    if INDUCED:
        m = sam.get_graph_num_induced(key)
        row, col, eid = sam.get_graph_induced_row(key), sam.get_graph_induced_col(key), sam.get_graph_induced_edge_ids(key)
        assert row.numel() == col.numel() == eid.numel() == m and row.device == sam.get_graph_row(key, 0).device
        assert row.dtype == col.dtype == eid.dtype == sam.get_graph_row(key, 0).dtype
        rec.update(ind_row=row.cpu().numpy(), ind_col=col.cpu().numpy(), ind_eid=eid.cpu().numpy(), num_induced=m)
        if FEAT:
            rows = sam.get_graph_induced_edge_feat(key)
            assert rows.shape[0] == m and rows.dim() == 2
            rec["ind_efeat"] = rows.cpu().numpy()
    return rec


if __name__ == "__main__":
    link_driver.base_config = typed_driver.base_config
    link_driver.record_batch = record_batch
    link_driver.main()
