"""What the dense map's normals cost ("Normals"): the VLS-128 sequence mapped with "DenseMap" 1 at leaf 0.1 and 0.2
(the two tables of scripts/dense_map_measure.py), then, on that table, the host's clock around the waiting calls, --repeat single
runs each: get (the export the cost is read against) and normals at radius 1 and 2 (k_dense_normals, a group of 32 lanes a
voxel, and k_dense_normal_records), on a DenseMap of its own that holds the pipeline's table -- its exported points inserted
under their source ordinals --, with dense_map_normals of the pipeline itself timed beside it.  (The one-thread-a-voxel variant
in the profile's lines was measured once from a build that had it behind a knob; it is not kept.)  --trace 1: once more per leaf as a child
process under `rocprofv3 --kernel-trace --stats` -- a run of its own -- for the kernels' own times.  Appends to
profiles/dense_normals_measure.jsonl."""
import argparse, csv, glob, json, os, shutil, subprocess, sys, tempfile, time
import numpy as np
sys.path.insert(0, os.getcwd())
import lidarslam_amd as L

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=48)
ap.add_argument("--model", type=int, default=128)
ap.add_argument("--leaves", type=float, nargs="*", default=[0.1, 0.2])
ap.add_argument("--repeat", type=int, default=5)
ap.add_argument("--trace", type=int, default=0)
ap.add_argument("--child", type=int, default=0)  # the traced child: one leaf, every kernel once, nothing written
ap.add_argument("--tag", default="")
ap.add_argument("--out", default="profiles/dense_normals_measure.jsonl")
a = ap.parse_args()


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


clouds = [L.synth_frame(a.model, 1000, f) for f in range(a.frames)]
for leaf in a.leaves:
    s = mapped(clouds, leaf)
    views, first = L.dense_map_viewpoints(s)
    ctx = L.Context(0)
    d = copied(ctx, s, leaf)
    if a.child:
        for r in (1, 2):
            d.normals(r, 5, viewpoints=views, first_frame=first)
        d.close(), ctx.close(), s.close()
        sys.exit(0)
    case = dict(what="normals", model=a.model, frames=a.frames, leaf=leaf, voxels=d.size(), capacity=int(d.get_param("Capacity")), repeat=a.repeat,
                clock="host, around the waiting call; single runs in order", get_s=timed(lambda: d.get()))
    nan = {}
    for r in (1, 2):
        d.normals(r, 5, viewpoints=views, first_frame=first)  # (the first call allocates the records)
        case[f"normals_r{r}_s"] = timed(lambda: d.normals(r, 5, viewpoints=views, first_frame=first))
        kept = d.normals(r, 5, viewpoints=views, first_frame=first)
        nan[r] = int(np.isnan(kept["normal_x"]).sum())
        case[f"neighbors_mean_r{r}"] = float(kept["neighbors"].mean())
        case[f"pipeline_r{r}_s"] = timed(lambda: L.dense_map_normals(s, 1, -1.0, r, 5, True))
        assert L.dense_map_normals(s, 1, -1.0, r, 5, True).tobytes() == kept.tobytes()
    case.update(without_normal_r1=nan[1], without_normal_r2=nan[2], get_again_s=timed(lambda: d.get()))
    emit(**case)
    d.close(), ctx.close(), s.close()

if a.trace and shutil.which("rocprofv3"):
    for leaf in a.leaves:
        out = tempfile.mkdtemp(prefix="normals_trace_")
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", out, "--output-format", "csv", "--", sys.executable, os.path.abspath(__file__), "--child", "1", "--frames", str(a.frames),
               "--model", str(a.model), "--leaves", str(leaf)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=500)
        stats, calls = {}, []
        for path in glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                name = row.get("Name", "")
                if "k_dense_normal" in name or "k_dense_gather" in name:
                    key = "k_dense_normal_records" if "records" in name else "k_dense_gather" if "gather" in name else "k_dense_normals"
                    stats[key] = dict(calls=int(row["Calls"]), total_us=float(row["TotalDurationNs"]) / 1e3, min_us=float(row["MinNs"]) / 1e3, max_us=float(row["MaxNs"]) / 1e3)
        # the launches one by one, in the child's order: per kernel radius 1, then radius 2
        for path in glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                name = row.get("Kernel_Name", "")
                if "k_dense_normal" in name:
                    kind = "records" if "records" in name else "sums"
                    calls.append((int(row["Start_Timestamp"]), kind, (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3))
        seen = {}
        for i, (_, kind, us) in enumerate(sorted(calls)):
            seen[kind] = seen.get(kind, 0) + 1
            calls[i] = dict(kernel=kind, radius=seen[kind], us=us)
        emit(what="kernel_trace", tool="rocprofv3 --kernel-trace --stats, a run of its own", model=a.model, frames=a.frames, leaf=leaf, returncode=r.returncode, kernels=stats,
             calls=calls, note="" if stats else (r.stderr[-300:] or "no kernel_stats.csv found"))
        shutil.rmtree(out, ignore_errors=True)
