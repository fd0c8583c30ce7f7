"""Per-kernel medians of the grouping launches in a rocprofv3 kernel trace of scripts/grouping_calls.py (the first two calls
are dropped; k_union is split into its two passes).  usage: grouping_trace_summary.py <kernel_trace.csv>"""
import csv, sys, collections, re
rows = list(csv.DictReader(open(sys.argv[1])))
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
per = collections.defaultdict(list)
for r in rows:
    m = re.search(r"::(k_\w+)(?:<\d+>)?\(", r["Kernel_Name"])
    if m and "cluster" not in r["Kernel_Name"] and m.group(1) in ("k_union", "k_count", "k_centers", "k_border", "k_tag_hp", "k_noise_nn",
                                                                    "k_cell_insert", "k_cell_scatter", "k_compress", "k_flatten", "k_relabel",
                                                                    "k_sizes", "k_keep", "k_copy_i32", "k_member_tail", "k_compact_noise",
                                                                    "k_cluster_num", "k_seg_offsets"):
        per[m.group(1)].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
tot = 0.0
for k, v in per.items():
    if k == "k_union":
        p0, p1 = v[0::2][2:], v[1::2][2:]
        a, b = sorted(p0)[len(p0) // 2], sorted(p1)[len(p1) // 2]
        print("k_union pass0 med %.1f  pass1 med %.1f  (n=%d)" % (a, b, len(p0)))
        tot += a + b
    else:
        w = v[2:]
        md = sorted(w)[len(w) // 2]
        tot += md
        print("%s med %.1f (n=%d)" % (k, md, len(w)))
print("sum of the listed kernels, medians: %.1f us" % tot)
