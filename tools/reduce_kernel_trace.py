"""Reduce a rocprofv3 kernel trace of a bench.py run to the two tables kept under profiles/:
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python bench.py --steps 20 --warmup 5
    python tools/reduce_kernel_trace.py OUT stats.csv chain.txt
stats.csv: calls, total, average, share and launch shapes (workgroups x threads) per kernel; chain.txt: the kernels between
consecutive rdetr::decoder_reference_kernel launches (one per decoder layer and image group), by calls per window."""
import csv
import glob
import sys
from collections import defaultdict

rows = []
for path in glob.glob(sys.argv[1] + "/**/*kernel_trace.csv", recursive=True):
    rows += list(csv.DictReader(open(path)))
rows.sort(key=lambda r: int(r["Start_Timestamp"]))


def shape(r):
    wg = int(r["Workgroup_Size_X"]) * int(r.get("Workgroup_Size_Y", 1) or 1) * int(r.get("Workgroup_Size_Z", 1) or 1)
    grid = int(r["Grid_Size_X"]) * int(r.get("Grid_Size_Y", 1) or 1) * int(r.get("Grid_Size_Z", 1) or 1)
    return f"{grid // wg}x{wg}"


def table(sel):
    by = defaultdict(lambda: [0, 0.0, set()])
    for r in sel:
        e = by[r["Kernel_Name"]]
        e[0] += 1
        e[1] += (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
        e[2].add(shape(r))
    return sorted(by.items(), key=lambda kv: -kv[1][1])


total = sum(e[1] for _, e in table(rows))
with open(sys.argv[2], "w", newline="") as f:
    w = csv.writer(f)
    w.writerow(["kernel", "calls", "total_us", "avg_us", "percent", "workgroups x threads"])
    for name, (n, us, shapes) in table(rows):
        w.writerow([name[:150], n, f"{us:.1f}", f"{us / n:.2f}", f"{100 * us / total:.2f}", " ".join(sorted(shapes, key=lambda s: int(s.split("x")[0])))])

marks = [i for i, r in enumerate(rows) if "decoder_reference_kernel" in r["Kernel_Name"]]
windows = [(a, b) for a, b in zip(marks, marks[1:]) if b - a < 120]
if not windows:
    sys.exit("no decoder_reference_kernel windows in the trace")
inside = [r for a, b in windows for r in rows[a:b]]
with open(sys.argv[3], "w") as f:
    f.write(f"kernels between consecutive decoder_reference_kernel launches (graph replay, both image groups interleaved in time), "
            f"{len(windows)} windows, {len(rows)} launches in the trace\n")
    f.write("calls/window   avg us     workgroups x threads  kernel\n")
    for name, (n, us, shapes) in table(inside):
        f.write(f"{n / len(windows):12.2f} {us / n:8.2f} {' '.join(sorted(shapes, key=lambda s: int(s.split('x')[0]))):>24s}  {name[:130]}\n")
    f.write(f"launches per window: {len(inside) / len(windows):.2f}\n")
