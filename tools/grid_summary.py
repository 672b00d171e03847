"""Summarise the launch shapes of a rocprofv3 --kernel-trace CSV: for every ggms kernel the number of launches and the
largest grid seen, in workgroups and in 256-thread units (what GGMS_DEBUG_GRID_CAP counts).  Usage:
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python -m pytest -m gpu tests/test_gpu_grid_rounds.py -k "not natural"
    python tools/grid_summary.py DIR [cap]
With `cap`, every kernel whose largest grid has more workgroups than the cap allows is marked: `cap` workgroups, or
cap x (256 / block) for blocks narrower than 256 threads (the one-wave workgroups of k_weighted_hash_dedup come four to a
unit).  A marked kernel must be on the list of launches the cap leaves alone ("Test aid: the grid cap")."""
import collections
import csv
import glob
import re
import sys


def _dims(r, what):
    if what + "_X" in r:
        return [int(r[what + a]) for a in ("_X", "_Y", "_Z")]
    return [int(r[what]), 1, 1]


def main():
    d = sys.argv[1]
    cap = int(sys.argv[2]) if len(sys.argv) > 2 else None
    seen = collections.OrderedDict()
    for f in sorted(glob.glob(d + "/**/*kernel_trace.csv", recursive=True)):
        with open(f, newline="") as fh:
            rows = list(csv.DictReader(fh))
        for r in rows:
            name = r["Kernel_Name"]
            if "ggms" not in name:
                continue
            name = name.replace("(anonymous namespace)::", "").replace("void ", "")
            name = re.sub(r"<.*", "<>", name)  # one line per kernel template
            name = re.sub(r"\(.*", "", name)   # the argument list
            wg, grid = _dims(r, "Workgroup_Size"), _dims(r, "Grid_Size")
            groups = [max(g // max(w, 1), 1) for g, w in zip(grid, wg)]
            threads = grid[0] * grid[1] * grid[2]
            e = seen.setdefault(name, dict(n=0, groups=[0, 0, 0], threads=0, wg=wg))
            e["n"] += 1
            e["threads"] = max(e["threads"], threads)
            if groups[0] * groups[1] * groups[2] > e["groups"][0] * e["groups"][1] * e["groups"][2]:
                e["groups"], e["wg"] = groups, wg
    print(f"{'kernel':58s} {'launches':>8s} {'max grid':>12s} {'block':>6s} {'x256 threads':>12s}")
    for name, e in sorted(seen.items()):
        g = "x".join(str(v) for v in e["groups"] if v > 1) or "1"
        units = e["threads"] / 256.0
        num_groups = e["groups"][0] * e["groups"][1] * e["groups"][2]
        block = e["wg"][0] * e["wg"][1] * e["wg"][2]
        over = "   ABOVE THE CAP" if cap is not None and num_groups > cap * max(256 // max(block, 1), 1) else ""
        print(f"{name[:58]:58s} {e['n']:8d} {g:>12s} {e['wg'][0] * e['wg'][1] * e['wg'][2]:6d} {units:12.2f}{over}")


if __name__ == "__main__":
    main()
