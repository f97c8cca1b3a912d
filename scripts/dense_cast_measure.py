"""What a question along a ray costs ("Rays"): the VLS-128 sequence mapped with the dense map on at leaf 0.1 and
0.2, then, on the map as it stands, by the host's clock (the median of --runs calls, each behind a settled map): the compare
of the last frame against the map (dense_map_compare_frame, labels of every point) at tolerances of 1, 2 and 4 leaves with
the label shares -- how much of the static street reads THROUGH_MAP is the honest figure for the grazing limit --, a 128 x 2048
render at 30 m with the voxels visited per ray from the hits' steps, and the download of the whole map (dense_map) beside them:
what a caller paid before these calls to answer the same question on the host.  Then, on a table of its own fed the same frames
under the generator's poses (DenseMap.insert_frame), compare_frame of the last frame beside carve_frame of the same frame on the
same map: by the host's clock, and -- --trace 1 -- once more as a child process under `rocprofv3 --kernel-trace --stats`, a run of
its own, for the times of k_dense_compare and k_dense_carve themselves.  Appends to profiles/dense_cast_measure.jsonl."""
import argparse, csv, glob, json, os, shutil, subprocess, sys, tempfile, time
import numpy as np
sys.path.insert(0, os.getcwd())
import lidarslam_amd as L

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=48)
ap.add_argument("--model", type=int, default=128)
ap.add_argument("--leaves", type=float, nargs="*", default=[0.1, 0.2])
ap.add_argument("--range", type=float, default=30.0)
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--trace", type=int, default=0)
ap.add_argument("--child", type=int, default=0)  # the traced child: the table of its own at one leaf, nothing written
ap.add_argument("--tag", default="")
ap.add_argument("--out", default="profiles/dense_cast_measure.jsonl")
a = ap.parse_args()


def emit(**kw):
    if a.tag:
        kw["tag"] = a.tag
    with open(a.out, "a") as out:
        out.write(json.dumps(kw) + "\n")
    print(kw, flush=True)


def clocked(call):
    """(the last result, the median of the wall times of --runs calls)"""
    times = []
    for _ in range(a.runs):
        t0 = time.perf_counter()
        out = call()
        times.append(time.perf_counter() - t0)
    return out, float(np.median(times))


def own_table(clouds, leaf):
    """compare_frame and carve_frame of the last frame on a table fed every frame under the generator's poses.
    -> (counts, compare seconds, carve seconds (enqueued and waited for), voxels)"""
    ctx = L.Context(0)
    d = L.DenseMap(ctx, leaf, CarveRange=a.range)
    last = len(clouds) - 1
    for f, (pts, _) in enumerate(clouds):
        ctx.upload_frame(pts)
        d.insert_frame(f, L.synth_pose(f), L.synth_pose(f + 1), -0.1, 0.0)
    voxels = d.size()
    pose = (L.synth_pose(last), L.synth_pose(last + 1), -0.1, 0.0)
    (labels, counts), compare_s = clocked(lambda: d.compare_frame(*pose, max_range=a.range, before=last))

    def carve():
        d.carve_frame(last, *pose)
        return d.size()  # waits for it

    carve()  # the first carve of a map makes its miss array
    _, carve_s = clocked(carve)
    d.close()
    ctx.close()
    return counts, compare_s, carve_s, voxels


clouds = [L.synth_frame(a.model, 1000, f) for f in range(a.frames)]
if a.child:
    own_table(clouds, a.leaves[0])
    sys.exit(0)

for leaf in a.leaves:
    s = L.Slam(0, EgoMotion=3, DenseMapLeafSize=leaf, DenseMap=1)
    for f, (pts, stamp) in enumerate(clouds):
        s.add_frame(pts, stamp, f)
    voxels = L.dense_map_size(s)
    base = dict(model=a.model, frames=a.frames, leaf=leaf, voxels=voxels, capacity=int(s.get_param("DenseMapCapacity")), max_range=a.range, runs=a.runs,
                points_in_frame=int(s.registered_frame().size))
    _, export_s = clocked(lambda: L.dense_map(s))
    emit(what="export", wall_s=export_s, **base)
    for leaves in (1, 2, 4):
        (labels, counts), wall = clocked(lambda: L.dense_map_compare_frame(s, tolerance=leaves * leaf, max_range=a.range))
        judged = max(int(counts[1] + counts[2] + counts[3]), 1)
        emit(what="compare_frame", tolerance_leaves=leaves, wall_s=wall, not_judged=int(counts[0]), consistent=int(counts[1]), unmapped=int(counts[2]),
             through_map=int(counts[3]), through_map_share_of_judged=int(counts[3]) / judged, **base)
    el = np.deg2rad(np.linspace(-25.0, 15.0, 128))
    hits, wall = clocked(lambda: L.dense_map_render_scan(s, el, 2048, max_range=a.range))
    cast = hits["status"] >= 0
    emit(what="render_128x2048", wall_s=wall, rays=int(cast.sum()), hits=int((hits["status"] == 1).sum()), visited_voxels=int(hits["steps"].sum()),
         visited_per_ray=float(hits["steps"][cast].mean()), rays_per_s=float(cast.sum() / wall), **base)
    s.close()

for leaf in a.leaves:
    counts, compare_s, carve_s, voxels = own_table(clouds, leaf)
    emit(what="compare_beside_carve", model=a.model, frames=a.frames, leaf=leaf, voxels=voxels, max_range=a.range, runs=a.runs, points_in_frame=int(clouds[-1][0].size),
         compare_frame_wall_s=compare_s, carve_frame_wall_s=carve_s, labels=[int(c) for c in counts],
         note="compare: tolerance one leaf, before = the frame's ordinal, the labels downloaded; carve: margin 2 leaves, stride 1, enqueued and waited for")

if a.trace and shutil.which("rocprofv3"):
    for leaf in a.leaves:
        d = tempfile.mkdtemp(prefix="cast_trace_")
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "--output-format", "csv", "--", sys.executable, os.path.abspath(__file__), "--child", "1", "--frames", str(a.frames),
               "--model", str(a.model), "--leaves", str(leaf), "--range", str(a.range), "--runs", str(a.runs)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=500)
        rows = {}
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                name = row.get("Name", "")
                for k in ("k_dense_compare", "k_dense_carve", "k_dense_claim", "k_dense_apply"):
                    if k in name:
                        rows[k] = dict(calls=int(row["Calls"]), total_us=float(row["TotalDurationNs"]) / 1e3, average_us=float(row["AverageNs"]) / 1e3,
                                       min_us=float(row["MinNs"]) / 1e3, max_us=float(row["MaxNs"]) / 1e3)
        emit(what="kernel_trace", tool="rocprofv3 --kernel-trace --stats, a run of its own", model=a.model, frames=a.frames, leaf=leaf, max_range=a.range,
             compare_calls=a.runs, carve_calls=a.runs + 1, returncode=r.returncode, kernels=rows, note="" if rows else (r.stderr[-300:] or "no kernel_stats.csv found"))
        shutil.rmtree(d, ignore_errors=True)
