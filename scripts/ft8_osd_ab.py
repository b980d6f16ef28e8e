"""Does another form of osd_decode_kernel slow FT8 OSD down?  scripts/ft8_osd_cost.py (OSD off / order 1 / order 2 / off again at 1024 FT8 channels)
in four child processes in a row on one box -- the parent commit's library, this tree's, the parent's, this tree's -- and one record of the four
results: the tree's order-1 and order-2 medians are read against the parent's own boundary spread of the same legs.  This process opens no
context itself.

    python scripts/ft8_osd_ab.py --parent-tree <checkout of the parent commit, built> [--out profiles/ft8_osd_cost_after_ft4.json]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--parent-tree", required=True)
ap.add_argument("--channels", type=int, default=1024)
ap.add_argument("--boundaries", type=int, default=7)
ap.add_argument("--child-timeout", type=float, default=420.0, help="seconds one child process may take: a child that hangs must not hold the card")
ap.add_argument("--out", default=os.path.join(HERE, "profiles", "ft8_osd_cost_after_ft4.json"))
args = ap.parse_args()
order = ["parent", "tree", "parent", "tree"]
runs = []
with tempfile.TemporaryDirectory() as tmp:
    for k, which in enumerate(order):
        print("child %d: %s" % (k, which), file=sys.stderr, flush=True)
        path = os.path.join(tmp, "run%d.json" % k)
        subprocess.run([sys.executable, os.path.join(HERE, "scripts", "ft8_osd_cost.py"), "--tree", args.parent_tree if which == "parent" else HERE,
                        "--channels", str(args.channels), "--boundaries", str(args.boundaries), "--out", path], check=True, stdout=subprocess.DEVNULL, timeout=args.child_timeout)
        runs.append(dict(json.load(open(path)), which=which))
par = [r for r in runs if r["which"] == "parent"]
tree = [r for r in runs if r["which"] == "tree"]
out = dict(what="scripts/ft8_osd_cost.py on the parent commit's library and this tree's, four processes in a row on one box", order=order)
for leg in ("off", "order1", "order2", "off_again"):
    lo = min(p[leg]["sync_ms_min"] for p in par)
    hi = max(p[leg]["sync_ms_max"] for p in par)
    out[leg] = dict(parent_sync_ms_medians=[p[leg]["sync_ms_median"] for p in par], parent_sync_ms_range=[lo, hi],
                    tree_sync_ms_medians=[t[leg]["sync_ms_median"] for t in tree],
                    tree_inside_parent_range=bool(all(lo <= t[leg]["sync_ms_median"] <= hi for t in tree)))
out["runs"] = runs
print(json.dumps({k: v for k, v in out.items() if k != "runs"}))
with open(args.out, "w") as fh:
    json.dump(out, fh, indent=1)
    fh.write("\n")
