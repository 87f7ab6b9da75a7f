"""Per-phase kernel totals of a `rocprofv3 --kernel-trace` run of tools/time_bidirectional.py on ONE workload (developer tool).
usage: python tools/bidirectional_trace_summary.py <rocprofv3 results .db> [width height]

Phases, in launch order: (a) the two-call pairs (packed resampling: resample_x_levels*), (b)+(c) the bidirectional calls (the
sequence cache's per-level resample_x_lds_kernel marks their start), (d) the lock-step group (its first copy_planes_kernel)."""
import collections
import re
import sqlite3
import statistics
import sys


def name_of(n):
    return re.match(r"(?:void )?(?:\(anonymous namespace\)::)?([\w:]+(?:<[^>]*>)?)", n).group(1)


def main():
    db = sqlite3.connect(sys.argv[1])
    w, h = (int(a) for a in sys.argv[2:4]) if len(sys.argv) > 3 else (4096, 4096)
    rows = db.execute("select name, start, end from kernels order by start").fetchall()
    names = [name_of(r[0]) for r in rows]
    first_bc, first_d = names.index("resample_x_lds_kernel"), names.index("copy_planes_kernel")
    stats = collections.defaultdict(list)
    for i, ((_, s, e), k) in enumerate(zip(rows, names)):
        phase = "d" if i >= first_d else "b/c" if i >= first_bc else "a"
        stats[(phase, k)].append((e - s) / 1e3)
    print("%-5s %-48s %6s %11s %9s" % ("phase", "kernel", "count", "total_us", "avg_us"))
    for phase in ("a", "b/c", "d"):
        items = sorted(((k, d) for (p, k), d in stats.items() if p == phase), key=lambda kv: -sum(kv[1]))
        for k, d in items:
            print("%-5s %-48s %6d %11.1f %9.2f" % (phase, k, len(d), sum(d), sum(d) / len(d)))
        print("%-5s %-48s %6d %11.1f" % (phase, "ALL", sum(len(d) for _, d in items), sum(sum(d) for _, d in items)))
    cons = [(e - s) / 1e3 for (_, s, e), k in zip(rows, names) if k.startswith("consistency_kernel")]
    mb = w * h * 20 / 1e6  # 8 B/px coalesced flow reads, 8 B/px gathered backward flow, 4 B/px mask
    med = statistics.median(cons)
    print("\nconsistency_kernel %dx%d: %d launches, median %.1f us, min %.1f, max %.1f; %.1f MB algorithmic -> %.2f TB/s at the "
          "median" % (w, h, len(cons), med, min(cons), max(cons), mb, mb / med))


if __name__ == "__main__":
    main()
