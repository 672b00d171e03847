"""tests/link_driver.py's run, with every batch's excluded-edge count next to its arrays:

    python tests/link_exclude_driver.py <dataset_dir> <out_prefix> [extra k=v ...]

link_driver.py itself is used as it is: its record of a batch gets one more entry, `num_excluded`
(sam.get_graph_num_excluded), and its main() does the rest.
"""
import link_driver

_record_batch = link_driver.record_batch


def record_batch(sam, key, num_layers, link):
    rec = _record_batch(sam, key, num_layers, link)
    rec["num_excluded"] = sam.get_graph_num_excluded(key)
    return rec


if __name__ == "__main__":
    link_driver.record_batch = record_batch
    link_driver.main()
