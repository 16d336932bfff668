"""Kernel time per HMC step from two rocprofv3 --kernel-trace --stats passes of bench.py that differ only in --steps:
the difference of the two kernel_stats.csv leaves the timed region's launches (set-up, warm-up and calibration cancel).

Usage: python profiles/kstats_per_step.py <kernel_stats.csv of the short run> <of the long run> <steps difference> [top]
"""
import csv
import re
import sys


def load(path):
    d = {}
    with open(path) as f:
        for r in csv.DictReader(f):
            name = re.sub(r"\(.*", "", r["Name"]).replace("vihmc::", "").replace("void ", "")
            d[name] = (int(r["Calls"]), float(r["TotalDurationNs"]) / 1e3)
    return d


def main():
    a, b, steps = load(sys.argv[1]), load(sys.argv[2]), int(sys.argv[3])
    top = int(sys.argv[4]) if len(sys.argv) > 4 else 14
    rows = []
    for n, (c1, t1) in b.items():
        c0, t0 = a.get(n, (0, 0.0))
        if c1 > c0:
            rows.append((n, (c1 - c0) / steps, (t1 - t0) / steps, (t1 - t0) / (c1 - c0)))
    rows.sort(key=lambda r: -r[2])
    tot = sum(r[2] for r in rows)
    print(f"kernel time per HMC step {tot:.1f} us in {sum(r[1] for r in rows):.1f} launches")
    print(f"{'kernel':44s} {'per step':>9s} {'us/step':>10s} {'avg_us':>9s} {'pct':>6s}")
    for n, c, t, avg in rows[:top]:
        print(f"{n[:44]:44s} {c:9.2f} {t:10.1f} {avg:9.2f} {100 * t / tot:6.2f}")


if __name__ == "__main__":
    main()
