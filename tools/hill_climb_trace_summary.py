"""the kernel trace of a tools/hill_climb_timing.py run (rocprofv3 --kernel-trace --output-format csv), split by call:
per (call, kernel) the number of launches and the min / median / max duration in microseconds, as CSV on stdout.
the tool's calls alternate highest, nearest, deep, components at 1.5 edges and then at 3; a call is the launches from
the k_nbr_addresses in front of k_hc_parent or k_cc_init to the next k_hc_peaks or, for components, k_cc_label.
warm-up repetitions are counted too.
    python tools/hill_climb_trace_summary.py <kernel_trace.csv> > profiles/r11_hill_climb_c2_kernel_stats.csv"""
import csv
import re
import sys
from collections import defaultdict

CASES = ["highest_r1.5", "nearest_r1.5", "deep_r1.5", "components_r1.5",
         "highest_r3", "nearest_r3", "deep_r3", "components_r3"]
LAST = {"k_hc_parent": "k_hc_peaks", "k_cc_init": "k_cc_label"}


def main():
    rows = list(csv.DictReader(open(sys.argv[1])))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    names = [re.sub(r"[(<].*", "", r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("void ", ""))
             for r in rows]
    calls = []
    i = 0
    while i < len(rows):
        if names[i] == "k_nbr_addresses" and i + 1 < len(rows) and names[i + 1] in LAST:
            j = i
            while names[j] != LAST[names[i + 1]]:
                j += 1
            calls.append((i, j))
            i = j + 1
        else:
            i += 1
    stats = defaultdict(list)
    span = defaultdict(list)
    for n, (a, b) in enumerate(calls):
        case = CASES[n % len(CASES)]
        assert case.startswith("components") == (names[a + 1] == "k_cc_init"), (n, case, names[a + 1])
        for k in range(a, b + 1):
            stats[(case, names[k])].append((int(rows[k]["End_Timestamp"]) - int(rows[k]["Start_Timestamp"])) / 1e3)
        span[case].append((int(rows[b]["End_Timestamp"]) - int(rows[a]["Start_Timestamp"])) / 1e3)
    out = csv.writer(sys.stdout)
    out.writerow(["call", "kernel", "launches", "min_us", "median_us", "max_us"])
    for case in CASES:
        for (c, k), v in stats.items():
            if c == case:
                v = sorted(v)
                out.writerow([case, k, len(v), round(v[0], 1), round(v[len(v) // 2], 1), round(v[-1], 1)])
        v = sorted(span[case])
        out.writerow([case, "first kernel's start to last kernel's end", len(v), round(v[0], 1),
                      round(v[len(v) // 2], 1), round(v[-1], 1)])


if __name__ == "__main__":
    main()
