"""Dev tool: HBM traffic per launch from two rocprofv3 PMC passes (FETCH_SIZE, WRITE_SIZE) -> profiles/*.json.

usage: python tools/pmc_traffic.py <dir with fetch/ and write/ sub-dirs> <out.json> <frames>
Correction per MI355X_MICROARCH.md (HBM section): on gfx950 FETCH_SIZE tallies 64 B per 128-B request of a
wide coalesced read -> x2; WRITE_SIZE exact; both counters report KiB.
"""
import csv, glob, json, os, sys
from collections import defaultdict
root, out, frames = sys.argv[1], sys.argv[2], int(sys.argv[3])
def per_kernel(sub, counter):
    tot, n = defaultdict(float), defaultdict(set)
    for f in glob.glob(os.path.join(root, sub, "**", "*counter_collection.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            if r["Counter_Name"] == counter and "hicom::" in r["Kernel_Name"]:
                k = r["Kernel_Name"].split("hicom::")[1].split("<")[0].split("(")[0]
                tot[k] += float(r["Counter_Value"]); n[k].add(r["Dispatch_Id"])
    return {k: (tot[k] / len(n[k]), len(n[k])) for k in tot}
fe, wr = per_kernel("fetch", "FETCH_SIZE"), per_kernel("write", "WRITE_SIZE")
res = {"command": "rocprofv3 --kernel-trace --pmc <FETCH_SIZE|WRITE_SIZE> --output-format csv -- python3 bench.py --full --steps 10 --warmup 3 "
                  "--no-cpu-baseline --no-graph  (one counter per pass; includes the roofline loop of bench.py)",
       "correction": "MI355X_MICROARCH.md HBM section: on gfx950 FETCH_SIZE tallies 64 B per 128-B request of a wide coalesced "
                     "read -> x2; WRITE_SIZE exact; both reported in KiB",
       "frames": frames, "workload": "%d x 729 x 1152 bf16, direct, hidden 896 (BASELINE configs[1])" % frames, "kernels": {}}
for k in sorted(set(fe) | set(wr)):
    f, nf = fe.get(k, (0.0, 0)); w, nw = wr.get(k, (0.0, 0))
    res["kernels"][k] = {"FETCH_SIZE_KiB_mean": f, "WRITE_SIZE_KiB_mean": w, "launches": max(nf, nw),
                         "hbm_bytes_per_launch_corrected": (2 * f + w) * 1024}
json.dump(res, open(out, "w"), indent=1)
for k, v in res["kernels"].items():
    print("%-28s launches %3d  fetch %.1f KiB  write %.1f KiB  -> %.2f MB" % (k, v["launches"], v["FETCH_SIZE_KiB_mean"], v["WRITE_SIZE_KiB_mean"],
                                                                             v["hbm_bytes_per_launch_corrected"] / 1e6))
