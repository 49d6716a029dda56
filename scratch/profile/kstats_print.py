"""scratch/profile/kstats_print.py <kernel_stats.csv> [min total us]: the kernels of a `rocprofv3 --kernel-trace --stats --output-format csv`
run whose summed time reaches the threshold (default 150 us): calls, average, minimum and maximum per launch in microseconds."""
import csv
import sys

floor = float(sys.argv[2]) if len(sys.argv) > 2 else 150.0
for r in csv.DictReader(open(sys.argv[1])):
    name = r["Name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0].split("::")[-1][:44]
    if float(r["AverageNs"]) * int(r["Calls"]) >= floor * 1e3:
        print("%-46s calls %5s avg %9.2f us min %9.2f max %9.2f" % (name, r["Calls"], float(r["AverageNs"]) / 1e3, float(r["MinNs"]) / 1e3,
                                                                     float(r["MaxNs"]) / 1e3))
