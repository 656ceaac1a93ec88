"""Timeline of one steady-state push from a rocprofv3 kernel trace, for pushes whose kernels run on two
streams: python3 scripts/push_timeline.py <dir with run_kernel_trace.csv> [first-kernel-substring]

A push is the kernels from the k_zero2 in front of one `first` kernel (default k_boundaries<false, 0, true>,
the single-pass form) up to the next push's k_zero2. Of the pushes that are followed by another within 3 ms (the benchmark's
timed steps; the last push of a --full run is followed by its digest copies) the middle one is printed:
start offset, gap since the latest end so far (negative: the kernel started while an earlier one was
still running, i.e. it overlaps), duration, hardware queue, name. The last line gives the push's span
from its first kernel's start to its last kernel's end and the sum of the durations."""
import csv
import glob
import sys

d = sys.argv[1]
first = sys.argv[2] if len(sys.argv) > 2 else "k_boundaries<false, 0, true>"
f = glob.glob(d + "/**/run_kernel_trace.csv", recursive=True) + glob.glob(d + "/run_kernel_trace.csv")
rows = sorted(csv.DictReader(open(f[0])), key=lambda r: int(r["Start_Timestamp"]))
start = [int(r["Start_Timestamp"]) for r in rows]
idx = [i for i, r in enumerate(rows) if first in r["Kernel_Name"]]
steady = [(a, b) for a, b in zip(idx[:-1], idx[1:]) if start[b] - start[a] < 3_000_000]
if not steady:
    steady = list(zip(idx[:-1], idx[1:]))
a, b = steady[len(steady) // 2]
while b > a and "k_zero2" not in rows[b]["Kernel_Name"]:
    b -= 1
if b == a:
    b = steady[len(steady) // 2][1]
# (the push's k_zero2, and whatever the side stream starts beside it, come just before `first`)
for k in range(a - 1, max(a - 6, -1), -1):
    if "k_zero2" in rows[k]["Kernel_Name"]:
        a = k
        break
t0 = start[a]
latest = t0
busy = 0
for r in rows[a:b]:
    s, e = int(r["Start_Timestamp"]), int(r["End_Timestamp"])
    busy += e - s
    over = " ||" if s < latest else "   "
    print(f"{(s - t0) / 1e3:8.1f} gap {(s - latest) / 1e3:7.1f} dur {(e - s) / 1e3:6.1f} q{r.get('Queue_Id', '?'):>2}{over} "
          f"{r['Kernel_Name'][:70]}")
    latest = max(latest, e)
print(f"push span {(latest - t0) / 1e3:.1f} us (first kernel start to last kernel end), kernels busy {busy / 1e3:.1f} us, "
      f"next push starts at {(start[steady[len(steady) // 2][1]] - t0) / 1e3:.1f} us; {len(steady)} steady pushes in the trace")
