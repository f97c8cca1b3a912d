"""What the dense map's floor plan costs ("Floor plan"): the VLS-128 sequence mapped with "DenseMap" 1 at leaf 0.1 and
0.2 (the two tables of scripts/dense_map_measure.py), then, on that table, the host's clock around the waiting calls, --repeat
single runs each: get_filtered (what a caller pays today before a single cell can be rasterised on the host -- the cost the grid is
read against), the whole grid, the 40 m window around the last pose, and the extent alone; on a DenseMap of its own that holds
the pipeline's table, with dense_map_grid of the pipeline itself timed beside it and checked equal.  Beside the times, the
bytes each launch names.  --trace 1: once more per leaf as a child process under `rocprofv3 --kernel-trace --stats` -- a run of
its own -- for the launches' own times.  Appends to profiles/dense_grid_measure.jsonl."""
import argparse, csv, glob, json, os, shutil, subprocess, sys, tempfile, time
import numpy as np
sys.path.insert(0, os.getcwd())
import lidarslam_amd as L

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=48)
ap.add_argument("--model", type=int, default=128)
ap.add_argument("--leaves", type=float, nargs="*", default=[0.1, 0.2])
ap.add_argument("--repeat", type=int, default=5)
ap.add_argument("--half", type=float, default=20.0)  # the window's half side in metres
ap.add_argument("--trace", type=int, default=0)
ap.add_argument("--child", type=int, default=0)  # the traced child: one leaf, the whole grid and the window once each, nothing written
ap.add_argument("--tag", default="")
ap.add_argument("--out", default="profiles/dense_grid_measure.jsonl")
a = ap.parse_args()
KERNELS = ("k_dense_grid_bounds", "k_dense_grid_columns", "k_dense_grid_rows", "k_dense_grid_ground", "k_dense_grid_band", "k_dense_grid_classify")


def emit(**kw):
    if a.tag:
        kw["tag"] = a.tag
    with open(a.out, "a") as out:
        out.write(json.dumps(kw) + "\n")
    print(kw, flush=True)


def mapped(clouds, leaf):
    s = L.Slam(0, EgoMotion=3)
    s.set_param("DenseMapLeafSize", leaf)
    s.set_param("DenseMap", 1)
    for f, (pts, stamp) in enumerate(clouds):
        if f + 1 < len(clouds):
            s.hint_next_frame(clouds[f + 1][0])
        s.add_frame(pts, stamp, f)
    return s


def copied(ctx, s, leaf):
    """the pipeline's table in a DenseMap of its own: one point a voxel, inserted under the ordinal that measured it"""
    pts, _ = L.dense_map(s, 1)
    src = L.dense_map_sources(s, 1)
    d = L.DenseMap(ctx, leaf)
    for f in np.unique(src):
        d.insert_points(pts[src == f], int(f))
    assert d.size() == pts.size
    return d


def timed(call):
    out = []
    for _ in range(a.repeat):
        t0 = time.perf_counter()
        call()
        out.append(time.perf_counter() - t0)
    return out


def named_bytes(capacity, voxels, info, radius=2, bounds=True):
    """the bytes each launch names, as the ProfScopes of lsa_dense_grid.hip state them"""
    w, h = int(info["width"]), int(info["height"])
    ew, eh, n = w + 2 * radius, h + 2 * radius, w * h
    out = dict(columns=capacity * 64 + voxels * 4, rows_and_ground=(eh * ew + 2 * eh * w + n) * 4, band=capacity * 64 + voxels * 12, classify=n * 41, download=n * 21)
    if bounds:
        out["bounds"] = capacity * 64
    return out


def extent_only(d, window=None):
    import ctypes as C
    p = L.DenseGridParams(min_height=0.2, max_height=2.0, max_miss_ratio=-1.0, cell_leaves=2, ground_radius=2, min_obstacle_voxels=1, min_frames=1)
    if window is not None:
        p.use_window = 1
        p.window[:] = list(window)
    info = L.DenseGridInfo()
    return d.L.lsa_dense_map_get_grid(d.h, C.byref(p), C.byref(info), None, None, 0)


clouds = [L.synth_frame(a.model, 1000, f) for f in range(a.frames)]
for leaf in a.leaves:
    s = mapped(clouds, leaf)
    x, y = s.world_transform()[:2, 3]
    window = (x - a.half, y - a.half, x + a.half, y + a.half)
    ctx = L.Context(0)
    d = copied(ctx, s, leaf)
    if a.child:
        d.grid(), d.grid(window=window)
        d.close(), ctx.close(), s.close()
        sys.exit(0)
    whole, local = d.grid(), d.grid(window=window)  # (the first calls allocate the rasters)
    capacity, voxels = int(d.get_param("Capacity")), d.size()
    case = dict(what="grid", model=a.model, frames=a.frames, leaf=leaf, voxels=voxels, capacity=capacity, repeat=a.repeat, cell_leaves=2, ground_radius=2,
                clock="host, around the waiting call; single runs in order", get_filtered_s=timed(lambda: d.get()),
                whole_cells=[int(whole[0]["width"]), int(whole[0]["height"])], whole_s=timed(lambda: d.grid()),
                window_m=2 * a.half, window_cells=[int(local[0]["width"]), int(local[0]["height"])], window_s=timed(lambda: d.grid(window=window)),
                whole_extent_only_s=timed(lambda: extent_only(d)), window_extent_only_s=timed(lambda: extent_only(d, window)),
                pipeline_whole_s=timed(lambda: L.dense_map_grid(s)), pipeline_window_s=timed(lambda: L.dense_map_grid(s, half_extent=a.half)),
                states_whole=[int((whole[2] == v).sum()) for v in (100, 0, -1)], states_window=[int((local[2] == v).sum()) for v in (100, 0, -1)],
                whole_bytes_named=named_bytes(capacity, voxels, whole[0]), window_bytes_named=named_bytes(capacity, voxels, local[0], bounds=False),
                get_filtered_bytes_downloaded=voxels * 56, get_filtered_again_s=timed(lambda: d.get()))
    for got, want in ((L.dense_map_grid(s), whole), (L.dense_map_grid(s, half_extent=a.half), local)):
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes() and got[2].tobytes() == want[2].tobytes()
    emit(**case)
    d.close(), ctx.close(), s.close()

if a.trace and shutil.which("rocprofv3"):
    for leaf in a.leaves:
        out = tempfile.mkdtemp(prefix="grid_trace_")
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", out, "--output-format", "csv", "--", sys.executable, os.path.abspath(__file__), "--child", "1", "--frames", str(a.frames),
               "--model", str(a.model), "--leaves", str(leaf), "--half", str(a.half)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=500)
        stats, calls = {}, []
        for path in glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                for k in KERNELS:
                    if k in row.get("Name", ""):
                        stats[k] = dict(calls=int(row["Calls"]), total_us=float(row["TotalDurationNs"]) / 1e3, min_us=float(row["MinNs"]) / 1e3, max_us=float(row["MaxNs"]) / 1e3)
        # the launches one by one, in the child's order: the whole grid, then the window
        for path in glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                for k in KERNELS:
                    if k in row.get("Kernel_Name", ""):
                        calls.append((int(row["Start_Timestamp"]), k, (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3))
        seen, ordered = {}, []
        for _, k, us in sorted(calls):
            seen[k] = seen.get(k, 0) + 1
            ordered.append(dict(kernel=k, call="whole" if k == "k_dense_grid_bounds" or seen[k] == 1 else "window", us=us))
        emit(what="kernel_trace", tool="rocprofv3 --kernel-trace --stats, a run of its own", model=a.model, frames=a.frames, leaf=leaf, returncode=r.returncode, kernels=stats,
             calls=ordered, note="" if stats else (r.stderr[-300:] or "no kernel_stats.csv found"))
        shutil.rmtree(out, ignore_errors=True)
