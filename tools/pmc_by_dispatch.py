#!/usr/bin/env python3
"""rocprofv3 --pmc counter_collection.csv -> counter values per DISPATCH of the kernels whose name contains <substring>, in dispatch order
(for programs that launch a known sequence of kernels, such as tools/probes/fetch_calib.hip).
usage: tools/pmc_by_dispatch.py <substring> <csv> [<csv> ...]"""
import collections, csv, json, sys

sub, paths = sys.argv[1], sys.argv[2:]
per = collections.OrderedDict()
for path in paths:
    rows = collections.defaultdict(dict)
    for r in csv.DictReader(open(path)):
        if sub in r["Kernel_Name"]:
            rows[int(r["Dispatch_Id"])][r["Counter_Name"]] = float(r["Counter_Value"])
            rows[int(r["Dispatch_Id"])]["_ns"] = float(r["End_Timestamp"]) - float(r["Start_Timestamp"])
    for k, (d, cs) in enumerate(sorted(rows.items())):
        per.setdefault(k, {}).update(cs)
for k in sorted(per):
    print(k, json.dumps(per[k]))
