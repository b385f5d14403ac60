"""Developer tool: per-kernel start/end times of a few frames from a rocprofv3 --kernel-trace database, as a
text timeline (who overlaps whom).   python tools/timeline.py gpurun_out/tl/x_results.db [first_frame n_frames]"""
import sqlite3
import sys

db = sqlite3.connect(sys.argv[1])
gaps_mode = len(sys.argv) > 2 and sys.argv[2] == "--gaps"
first = int(sys.argv[2]) if len(sys.argv) > 2 and not gaps_mode else 6
count = int(sys.argv[3]) if len(sys.argv) > 3 and not gaps_mode else 2
tabs = [r[0] for r in db.execute("select name from sqlite_master where type='table' or type='view'")]
kd = [t for t in tabs if t.startswith("kernels")] or [t for t in tabs if "kernel_dispatch" in t]
rows = None
for t in ("kernels",) + tuple(kd):
    try:
        rows = db.execute(f"select name, start, end, queue_id from {t} order by start").fetchall()
        break
    except sqlite3.Error:
        continue
if rows is None:
    print("tables:", tabs)
    sys.exit(1)
rows = [(n.split("(")[0].replace("void svr::", "").replace("svr::", "")[:34], s, e, q) for n, s, e, q in rows]
if gaps_mode:
    # python tools/timeline.py x_results.db --gaps [last_n]: idle time between consecutive tile kernels (end -> next
    # start) and their durations over the last last_n launches (bench.py's timed window: its --steps)
    import statistics
    last = int(sys.argv[3]) if len(sys.argv) > 3 else 60
    tk = [r for r in rows if r[0].startswith("tile_")][-last:]
    gaps = [(b[1] - a[2]) / 1e3 for a, b in zip(tk, tk[1:])]
    durs = [(r[2] - r[1]) / 1e3 for r in tk]
    period = [(b[1] - a[1]) / 1e3 for a, b in zip(tk, tk[1:])]
    for what, v in (("gap between tile kernels", gaps), ("tile kernel duration", durs), ("start to start", period)):
        q = statistics.quantiles(v, n=10)
        print(f"{what:26s} n {len(v):4d}  mean {statistics.fmean(v):8.2f}  median {statistics.median(v):8.2f}  p10 {q[0]:8.2f}  p90 {q[-1]:8.2f} us")
    print("queues of the tile kernels:", sorted({r[3] for r in tk}))
    sys.exit(0)
tiles = [i for i, r in enumerate(rows) if r[0].startswith("prologue")]
if len(tiles) <= first + count:
    first, count = max(0, len(tiles) - 3), 2
t0 = rows[tiles[first]][1]
for n, s, e, q in rows[tiles[first]:tiles[first + count]]:
    print(f"{(s - t0) / 1e3:9.1f} .. {(e - t0) / 1e3:9.1f} us  ({(e - s) / 1e3:7.1f})  q{q}  {n}")
