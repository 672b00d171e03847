"""tests/link_driver.py's run, with every layer's edge ids and edge-table rows and the positives' edge ids next to a
batch's arrays:

    python tests/edge_driver.py <dataset_dir> <out_prefix> [extra k=v ...]

link_driver.py itself is used as it is: its record of a batch gets `eid{i}` (edge_ids = on or edge_feat = on), `efeat{i}`
(edge_feat = on) and `link_edge_ids` (task = link_prediction), and its main() does the rest.
"""
import sys

import link_driver

_record_batch = link_driver.record_batch
ARGS = dict(a.split("=", 1) for a in sys.argv[3:])
FEAT = ARGS.get("edge_feat") == "on"
IDS = FEAT or ARGS.get("edge_ids") == "on"


def record_batch(sam, key, num_layers, link):
    rec = _record_batch(sam, key, num_layers, link)
    for i in range(num_layers):
        if IDS:
            eid = sam.get_graph_edge_ids(key, i)
            assert eid.numel() == sam.get_graph_num_edge(key, i) and eid.device == sam.get_graph_row(key, i).device
            rec[f"eid{i}"] = eid.cpu().numpy()
        if FEAT:
            rows = sam.get_graph_edge_feat(key, i)
            assert rows.shape[0] == sam.get_graph_num_edge(key, i) and rows.dim() == 2
            rec[f"efeat{i}"] = rows.cpu().numpy()
    if link:
        rec["link_edge_ids"] = sam.get_graph_link_edge_ids(key).cpu().numpy()
    return rec


if __name__ == "__main__":
    link_driver.record_batch = record_batch
    link_driver.main()
