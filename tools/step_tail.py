"""Per-step table of the mapper step from a rocprofv3 trace: mean us of every kernel of one phz_map_reads_batch submission, of the
device-to-host copy that ends it (if the trace has one) and of the gaps between them, from the start / end stamps.

usage: python tools/step_tail.py <dir with *_kernel_trace.csv [and *_memory_copy_trace.csv]> [steps to keep, from the end: default 50]

A step is the run of dispatches from one k_tile_window to the next; the last N steps are averaged (the earlier ones are set-up and warm-up).
"""
import csv
import glob
import os
import sys


def short(name):
    name = name.replace("(anonymous namespace)::", "").replace("void ", "")
    return name.split("(")[0][:40]


def main():
    d = sys.argv[1]
    keep = int(sys.argv[2]) if len(sys.argv) > 2 else 50
    kf = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if not kf:
        sys.exit("no *kernel_trace.csv under " + d)
    ev = []
    for r in csv.DictReader(open(kf[0])):
        ev.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short(r["Kernel_Name"])))
    for f in glob.glob(os.path.join(d, "**", "*memory_copy_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            direction = r.get("Direction", r.get("Name", "copy"))
            if "DEVICE_TO_HOST" in direction.upper().replace(" ", "_") or "DTOH" in direction.upper():
                ev.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), "copy D2H"))
    ev.sort()
    steps = []
    for e in ev:
        if e[2].startswith("k_tile_window"):
            steps.append([e])
        elif steps and (e[2].startswith("k_") or e[2] == "copy D2H"):
            steps[-1].append(e)
    # a step ends with its last mapper event: k_compact, or the copy right behind it
    for s in steps:
        last = max((i for i, e in enumerate(s) if e[2].startswith("k_compact")), default=len(s) - 1)
        if last + 1 < len(s) and s[last + 1][2] == "copy D2H":
            last += 1
        del s[last + 1:]
    steps = [s for s in steps if any(e[2].startswith("k_map") for e in s)][-keep:]
    if not steps:
        sys.exit("no mapper step in the trace")
    shape = [e[2] for e in steps[-1]]
    steps = [s for s in steps if [e[2] for e in s] == shape]
    n = len(steps)
    print("%d steps of %d events each; mean us per step" % (n, len(shape)))
    total = 0.0
    for i, name in enumerate(shape):
        dur = sum(s[i][1] - s[i][0] for s in steps) / n / 1e3
        if i:
            gap = sum(s[i][0] - s[i - 1][1] for s in steps) / n / 1e3
            print("  %-42s %9.2f" % ("(gap)", gap))
            total += gap
        print("  %-42s %9.2f" % (name, dur))
        total += dur
    span = sum(s[-1][1] - s[0][0] for s in steps) / n / 1e3
    kmap = sum(e[1] - e[0] for s in steps for e in s if e[2].startswith("k_map")) / n / 1e3
    print("  %-42s %9.2f" % ("first start -> last end", span))
    print("  %-42s %9.2f" % ("of it not k_map", span - kmap))
    period = (steps[-1][0][0] - steps[0][0][0]) / max(1, n - 1) / 1e3
    print("  %-42s %9.2f" % ("step period (start to next start)", period))


if __name__ == "__main__":
    main()
