"""The last two-lane step of a plain bench run from a rocprofv3 kernel trace, per hardware queue (the format of r06_timeline.txt):
   cd /tmp && rocprofv3 --kernel-trace --output-format csv -d $OUT -- python bench.py --steps 3 --warmup 1
   python profiles/timeline_lanes.py $OUT
Every kernel > 0.08 ms with its start and duration (ms from the step's first kernel), then the figures the schedule is judged by:
where the two k_mme3 launches end and start, when the ground truth's cell tables are complete, the second lane's k_nn_grid."""
import csv
import glob
import re
import sys

rows = []
for f in glob.glob(sys.argv[1] + "/**/*kernel_trace.csv", recursive=True):
    with open(f) as fh:
        for r in csv.DictReader(fh):
            n = re.sub(r"\(.*", "", r["Kernel_Name"])
            n = re.sub(r"<.*", "", n).split("::")[-1].split(" ")[-1]
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r.get("Queue_Id", "?"), n))
rows.sort()
mort = [i for i, r in enumerate(rows) if r[3] == "k_morton"]
step = rows[mort[-2]:]  # a step starts with two k_morton, one per cloud; a plain run ends with its last timed step
t0 = step[0][0]
ms = lambda t: (t - t0) / 1e6
print("two-lane step: %.2f ms wall, %d kernels" % (ms(max(r[1] for r in step)), len(step)))
queues = sorted({r[2] for r in step}, key=lambda q: min(r[0] for r in step if r[2] == q))
for q in queues:
    ks = [r for r in step if r[2] == q]
    print("--- queue %s: %d kernels, busy %.2f ms; kernels > 0.08 ms (start, duration)" % (q, len(ks), sum(r[1] - r[0] for r in ks) / 1e6))
    for r in ks:
        if r[1] - r[0] > 80_000:
            print("  %7.3f  dur %7.3f  %s" % (ms(r[0]), (r[1] - r[0]) / 1e6, r[3]))
mme = [r for r in step if r[3] == "k_mme3"]
fill = [r for r in step if r[3] == "k_cell_fill"]
gath = [r for r in step if r[3] == "k_gather"]
grid = [r for r in step if r[3] == "k_nn_grid"]
main_q = mme[0][2]
print("--- figures (ms)")
print("map k_mme3: %.3f -> %.3f (%.3f)" % (ms(mme[0][0]), ms(mme[0][1]), (mme[0][1] - mme[0][0]) / 1e6))
print("ground truth k_mme3: %.3f -> %.3f (%.3f); hole between the two: %.3f" % (ms(mme[1][0]), ms(mme[1][1]), (mme[1][1] - mme[1][0]) / 1e6, (mme[1][0] - mme[0][1]) / 1e6))
print("  kernels on the main queue inside the hole: %d" % sum(1 for r in step if r[2] == main_q and mme[0][1] <= r[0] < mme[1][0]))
g = [r for r in gath if r[2] != main_q][-1]
print("ground truth k_gather: %.3f -> %.3f (%.3f)" % (ms(g[0]), ms(g[1]), (g[1] - g[0]) / 1e6))
print("ground truth's last k_cell_fill ends: %.3f" % ms(max(r[1] for r in fill if r[2] != main_q)))
for r in grid:
    print("k_nn_grid on queue %s (%s lane): %.3f -> %.3f (%.3f)" % (r[2], "main" if r[2] == main_q else "second", ms(r[0]), ms(r[1]), (r[1] - r[0]) / 1e6))
print("end of the step: %.3f" % ms(max(r[1] for r in step)))
