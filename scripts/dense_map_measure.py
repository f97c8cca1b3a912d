"""What the dense point-cloud map costs: the VLS-128 sequence replayed from host clouds, the next cloud announced
as bench.py does, with "DenseMap" 0 / 1 / 2 at leaf 0.1 and 0.2.  Per case: frames/s over the frames behind --warmup, the table's
voxels, capacity, occupancy and bytes at the end, the rehashes, the points skipped, the time of one export (get with min_frames 1:
compaction, radix sort, gather, download).  --trace 1: each DenseMap = 1 case once more as a child process under
`rocprofv3 --kernel-trace --stats` -- a run of its own, so that the tracer's overhead stays out of the frames/s -- for the times
of k_dense_claim, k_dense_apply and k_dense_rehash.  Appends to profiles/dense_map_measure.jsonl."""
import argparse, csv, glob, json, os, shutil, subprocess, sys, tempfile, time
import numpy as np
sys.path.insert(0, os.getcwd())
import lidarslam_amd as L

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=48)
ap.add_argument("--warmup", type=int, default=8)
ap.add_argument("--model", type=int, default=128)
ap.add_argument("--leaves", type=float, nargs="*", default=[0.1, 0.2])
ap.add_argument("--modes", type=int, nargs="*", default=[0, 1, 2])
ap.add_argument("--trace", type=int, default=0)
ap.add_argument("--child", type=int, default=0)  # the traced child: one case, nothing written
ap.add_argument("--tag", default="")
ap.add_argument("--out", default="profiles/dense_map_measure.jsonl")
a = ap.parse_args()


def emit(**kw):
    if a.tag:
        kw["tag"] = a.tag
    with open(a.out, "a") as out:
        out.write(json.dumps(kw) + "\n")
    print(kw, flush=True)


def drive(clouds, mode, leaf):
    s = L.Slam(0, EgoMotion=3)
    if mode:
        s.set_param("DenseMapLeafSize", leaf)
        s.set_param("DenseMap", mode)
    t0 = None
    for f, (pts, stamp) in enumerate(clouds):
        if f == a.warmup:
            t0 = time.perf_counter()
        if f + 1 < len(clouds):
            s.hint_next_frame(clouds[f + 1][0])
        s.add_frame(pts, stamp, f)
    if mode:
        L.dense_map_size(s)  # the insertions in flight belong to the drive
    wall = time.perf_counter() - t0
    return s, (len(clouds) - a.warmup) / wall


clouds = [L.synth_frame(a.model, 1000, f) for f in range(a.frames)]
if a.child:
    s, _ = drive(clouds, a.modes[0], a.leaves[0])
    s.close()
    sys.exit(0)

for leaf in a.leaves:
    for mode in a.modes:
        if mode == 0 and leaf != a.leaves[0]:
            continue
        s, fps = drive(clouds, mode, leaf)
        case = dict(what="drive", model=a.model, frames=a.frames, warmup=a.warmup, points_per_frame=int(clouds[0][0].size), dense_map=mode, leaf=leaf if mode else None,
                    frames_per_s=fps, keyframes=int(s.stats()[13]))
        if mode:
            voxels, nbytes = int(s.get_param("DenseMapVoxels")), int(s.get_param("DenseMapBytes"))
            t0 = time.perf_counter()
            pts, vox = L.dense_map(s, 1)
            export = time.perf_counter() - t0
            capacity = int(s.get_param("DenseMapCapacity"))  # slots; "DenseMapBytes" = 64 B a slot + the 4 B a point of the slot scratch
            case.update(voxels=voxels, table_and_scratch_bytes=nbytes, capacity=capacity, occupancy=voxels / capacity, rehashes=int(s.get_param("DenseMapRehashes")),
                        skipped=int(s.get_param("DenseMapSkipped")), refused=int(s.get_param("DenseMapRefusedFrames")), inserted_frames=int(s.get_param("DenseMapFrames")),
                        export_wall_s=export, export_device_and_download_s=s.get_param("DenseMapExportSeconds"), exported=int(pts.size),
                        voxels_seen_in_3_frames=int((vox["frames"] >= 3).sum()))
        emit(**case)
        s.close()

if a.trace and shutil.which("rocprofv3"):
    for leaf in a.leaves:
        d = tempfile.mkdtemp(prefix="dense_trace_")
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "--output-format", "csv", "--", sys.executable, os.path.abspath(__file__), "--child", "1", "--frames", str(a.frames),
               "--model", str(a.model), "--modes", "1", "--leaves", str(leaf)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=400)
        rows = {}
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                name = row.get("Name", "")
                for k in ("k_dense_claim", "k_dense_apply", "k_dense_rehash"):
                    if k in name:
                        rows[k] = dict(calls=int(row["Calls"]), total_us=float(row["TotalDurationNs"]) / 1e3, average_us=float(row["AverageNs"]) / 1e3,
                                       min_us=float(row["MinNs"]) / 1e3, max_us=float(row["MaxNs"]) / 1e3)
        emit(what="kernel_trace", tool="rocprofv3 --kernel-trace --stats, a run of its own", model=a.model, frames=a.frames, dense_map=1, leaf=leaf, returncode=r.returncode,
             kernels=rows, note="" if rows else (r.stderr[-300:] or "no kernel_stats.csv found"))
        shutil.rmtree(d, ignore_errors=True)
