"""conv_x3r_kernel rows of the kernel_stats.csv files under a rocprofv3 --kernel-trace --stats output directory: calls, total ms and
average us per symbol (profiles/x3r_finish/):  python tools/x3r_trace_rows.py <directory>"""
import csv, glob, sys
d = sys.argv[1]
for f in sorted(glob.glob(d + "/**/*kernel_stats.csv", recursive=True)):
    tot = 0.0
    for r in csv.DictReader(open(f)):
        if "conv_x3r_kernel" in r["Name"]:
            n = r["Name"]; n = n[n.index("conv_x3r_kernel"):].split("(")[0]
            print(f"{n:40s} calls {int(r['Calls']):6d}  total {float(r['TotalDurationNs']) / 1e6:9.3f} ms  avg {float(r['AverageNs']) / 1e3:8.3f} us")
            tot += float(r["TotalDurationNs"])
    print(f"all conv_x3r_kernel rows: {tot / 1e6:.3f} ms")
