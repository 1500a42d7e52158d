#!/usr/bin/env python3
"""Average duration of the WaveNet layer launches in a rocprofv3 --kernel-trace run (rocpd SQLite output), by the layer's
place in its flow: the launches of a layer kernel (default: k_wn_layer_mixed, the streamed batch-1 utterance) in start
order; a launch of the <true, ...> instantiation is a flow's LAST layer, the launch behind a last layer (or the very first
one) is a flow's FIRST layer, every other one a middle layer.

  python tools/wn_launch_trace.py <results.db> [kernel name part] [label]
"""
import sqlite3
import sys


def main():
    db = sys.argv[1]
    part = sys.argv[2] if len(sys.argv) > 2 else "k_wn_layer_mixed"
    label = sys.argv[3] if len(sys.argv) > 3 else db
    c = sqlite3.connect(db)
    rows = c.execute("select name, end - start from kernels where name like ? order by start", ("%" + part + "%",)).fetchall()
    sums = {"first": [0, 0.0], "middle": [0, 0.0], "last": [0, 0.0]}
    after_last = True
    for name, dur in rows:
        last = (part + "<true") in name
        kind = "last" if last else "first" if after_last else "middle"
        after_last = last
        sums[kind][0] += 1
        sums[kind][1] += dur / 1e3
    print("%-28s %s" % (label, "  ".join("%s %7.2f us (%d)" % (k, v[1] / max(v[0], 1), v[0]) for k, v in sums.items())))


if __name__ == "__main__":
    main()
