"""scratch/profile/pmc_forward.py <counter_collection.csv>: mean counter values per launch of the two forward blend kernels
(k_blend_fwd_head, k_blend_fwd_parts) of a `rocprofv3 --pmc ... --output-format csv` run."""
import collections
import csv
import sys

acc = collections.defaultdict(lambda: [0.0, 0])
for r in csv.DictReader(open(sys.argv[1])):
    name = r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
    if "k_blend_fwd" in name:
        a = acc[(name, r["Counter_Name"])]
        a[0] += float(r["Counter_Value"])
        a[1] += 1
for (name, ctr), (total, n) in sorted(acc.items()):
    print("%-34s %-16s %12.3f M over %d launches" % (name, ctr, total / n / 1e6, n))
