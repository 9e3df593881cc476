"""Per-kernel means of the counters in a rocprofv3 --pmc CSV directory (full launches of the CG apply)."""
import csv
import glob
import json
import sys
from collections import defaultdict

d = sys.argv[1]
rows = defaultdict(lambda: defaultdict(list))
for f in glob.glob(d + "/**/*counter_collection.csv", recursive=True):
    for r in csv.DictReader(open(f)):
        k = r["Kernel_Name"]
        if "k_hobrick" not in k:
            continue
        name = "k_hobrick_um" if "k_hobrick_um" in k else "k_hobrick_cg"
        rows[name][r["Counter_Name"]].append(float(r["Counter_Value"]))
out = {}
for k, cs in rows.items():
    out[k] = {}
    for c, v in cs.items():
        v = sorted(v)
        full = [x for x in v if x >= 0.5 * v[len(v) // 2]]  # (each solve's last apply returns at once)
        out[k][c] = {"mean_full": sum(full) / max(len(full), 1), "launches": len(v), "full": len(full)}
print(json.dumps(out, indent=1))
json.dump(out, open(d + "/summary.json", "w"), indent=1)
