"""What free-space carving costs ("Free space"): the VLS-128 sequence replayed from host clouds, the next cloud
announced as bench.py does, with the dense map on at leaf 0.1 and 0.2 and "DenseMapCarve" 0 against 1 at stride 1 and 4, and on
keyframes only ("DenseMap" 2).  Per case: frames/s over the frames behind --warmup (the carves in flight belong to the drive), the
rays cast and rays/s, the voxels the rays of the last frame visit by the definition's own count (1 + |i1 - i0| summed over the
axes, from lsa_slam_get_registered_frame and ..._origins) and from it the visited voxels/s, the table's voxels, capacity and
bytes, what a filter at ratio 1 leaves and what a prune removes and gives back.  --trace 1: each carve case at stride 1 once
more as a child process under `rocprofv3 --kernel-trace --stats` -- a run of its own, so that the tracer's overhead stays out
of the frames/s -- for the times of k_dense_carve beside k_dense_claim and k_dense_apply.  Appends to
profiles/dense_carve_measure.jsonl."""
import argparse, csv, glob, json, os, shutil, subprocess, sys, tempfile, time
import numpy as np
sys.path.insert(0, os.getcwd())
import lidarslam_amd as L

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=48)
ap.add_argument("--warmup", type=int, default=8)
ap.add_argument("--model", type=int, default=128)
ap.add_argument("--leaves", type=float, nargs="*", default=[0.1, 0.2])
ap.add_argument("--cases", nargs="*", default=["1:0:1", "1:1:1", "1:1:4", "2:0:1", "2:1:1"])  # DenseMap : DenseMapCarve : stride
ap.add_argument("--range", type=float, default=30.0)
ap.add_argument("--trace", type=int, default=0)
ap.add_argument("--child", type=int, default=0)  # the traced child: one case, nothing written
ap.add_argument("--tag", default="")
ap.add_argument("--out", default="profiles/dense_carve_measure.jsonl")
a = ap.parse_args()


def emit(**kw):
    if a.tag:
        kw["tag"] = a.tag
    with open(a.out, "a") as out:
        out.write(json.dumps(kw) + "\n")
    print(kw, flush=True)


def drive(clouds, mode, carve, stride, leaf):
    s = L.Slam(0, EgoMotion=3)
    s.set_param("DenseMapLeafSize", leaf)
    s.set_param("DenseMap", mode)
    s.set_param("DenseMapCarveRange", a.range)
    s.set_param("DenseMapCarveStride", stride)
    s.set_param("DenseMapCarve", carve)
    t0 = None
    for f, (pts, stamp) in enumerate(clouds):
        if f == a.warmup:
            t0 = time.perf_counter()
        if f + 1 < len(clouds):
            s.hint_next_frame(clouds[f + 1][0])
        s.add_frame(pts, stamp, f)
    L.dense_map_size(s)  # the insertions and carves in flight belong to the drive
    wall = time.perf_counter() - t0
    return s, (len(clouds) - a.warmup) / wall


def visited_by_the_last_frame(s, leaf, stride):
    """the voxels the rays of the frame in the pipeline visit, counted as DenseMapHost.carve counts its steps, without walking"""
    pts, org = s.registered_frame()[::stride], L.registered_frame_origins(s)[::stride].astype(np.float64)
    p = np.stack([pts["x"], pts["y"], pts["z"]], axis=1).astype(np.float64)
    d = p - org
    length = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    with np.errstate(all="ignore"):
        t = np.minimum(length - 2.0 * leaf, a.range)
        e = org + d * (t / length)[:, None]
        steps = np.abs(np.floor(e / leaf) - np.floor(org / leaf)).sum(axis=1) + 1
    ok = np.isfinite(steps) & (t > 0)
    return int(ok.sum()), int(steps[ok].sum())


clouds = [L.synth_frame(a.model, 1000, f) for f in range(a.frames)]
cases = [tuple(int(v) for v in c.split(":")) for c in a.cases]
if a.child:
    s, _ = drive(clouds, *cases[0], a.leaves[0])
    s.close()
    sys.exit(0)

for leaf in a.leaves:
    for mode, carve, stride in cases:
        s, fps = drive(clouds, mode, carve, stride, leaf)
        inserted = int(s.get_param("DenseMapFrames"))
        case = dict(what="drive", model=a.model, frames=a.frames, warmup=a.warmup, points_per_frame=int(clouds[0][0].size), dense_map=mode, carve=carve, stride=stride,
                    carve_range=a.range, leaf=leaf, frames_per_s=fps, keyframes=int(s.stats()[13]), inserted_frames=inserted, voxels=int(s.get_param("DenseMapVoxels")),
                    capacity=int(s.get_param("DenseMapCapacity")), bytes=int(s.get_param("DenseMapBytes")), rehashes=int(s.get_param("DenseMapRehashes")))
        if carve:
            rays = int(s.get_param("DenseMapRays"))
            last_rays, last_visited = visited_by_the_last_frame(s, leaf, stride)
            seen = int(L.dense_map_filtered(s, 1, 1.0)[0].size)
            t0 = time.perf_counter()
            removed = L.prune_dense_map(s, 1, 1.0)
            prune_s = time.perf_counter() - t0
            case.update(rays=rays, rays_per_carved_frame=rays / max(inserted, 1), rays_per_s=rays * fps / a.frames,
                        last_frame_rays=last_rays, last_frame_visited_voxels=last_visited, visited_per_ray=last_visited / max(last_rays, 1),
                        visited_voxels_per_s=last_visited * fps * inserted / a.frames, kept_at_ratio_1=seen, pruned=removed, prune_wall_s=prune_s,
                        capacity_after_prune=int(s.get_param("DenseMapCapacity")), bytes_after_prune=int(s.get_param("DenseMapBytes")))
        emit(**case)
        s.close()

if a.trace and shutil.which("rocprofv3"):
    for leaf in a.leaves:
        d = tempfile.mkdtemp(prefix="carve_trace_")
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "--output-format", "csv", "--", sys.executable, os.path.abspath(__file__), "--child", "1", "--frames", str(a.frames),
               "--model", str(a.model), "--cases", "1:1:1", "--leaves", str(leaf), "--range", str(a.range)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=500)
        rows = {}
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                name = row.get("Name", "")
                for k in ("k_dense_carve", "k_dense_claim", "k_dense_apply", "k_dense_rehash"):
                    if k in name:
                        rows[k] = dict(calls=int(row["Calls"]), total_us=float(row["TotalDurationNs"]) / 1e3, average_us=float(row["AverageNs"]) / 1e3,
                                       min_us=float(row["MinNs"]) / 1e3, max_us=float(row["MaxNs"]) / 1e3)
        emit(what="kernel_trace", tool="rocprofv3 --kernel-trace --stats, a run of its own", model=a.model, frames=a.frames, dense_map=1, carve=1, stride=1, leaf=leaf,
             carve_range=a.range, returncode=r.returncode, kernels=rows, note="" if rows else (r.stderr[-300:] or "no kernel_stats.csv found"))
        shutil.rmtree(d, ignore_errors=True)
