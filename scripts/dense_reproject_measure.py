"""What the dense map's re-projection under a corrected trajectory costs: the VLS-128 sequence of
scripts/dense_map_measure.py mapped with "DenseMap" 1, "DenseMapOnTrajectory" 1 and the keypoint log on, then a trajectory
that moves every pose a little applied twice (there and back).  Per leaf: the table, "DenseMapReprojectSeconds" of both
applications (the first allocates the second table from the driver, the second finds memory the graveyard has given back or
not), the voxels before and after, the voxels dropped, the whole set_trajectory call by the host's clock, and one export for
comparison.  Appends to profiles/dense_reproject_measure.jsonl."""
import argparse, json, os, sys, time
import numpy as np
sys.path.insert(0, os.getcwd())
import lidarslam_amd as L

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=48)
ap.add_argument("--model", type=int, default=128)
ap.add_argument("--leaves", type=float, nargs="*", default=[0.1, 0.2])
ap.add_argument("--tag", default="")
ap.add_argument("--out", default="profiles/dense_reproject_measure.jsonl")
a = ap.parse_args()

clouds = [L.synth_frame(a.model, 1000, f) for f in range(a.frames)]
for leaf in a.leaves:
    s = L.Slam(0, EgoMotion=3, LoggingTimeout=-1, DenseMapLeafSize=leaf, DenseMap=1, DenseMapOnTrajectory=1)
    for f, (pts, stamp) in enumerate(clouds):
        if f + 1 < len(clouds):
            s.hint_next_frame(clouds[f + 1][0])
        s.add_frame(pts, stamp, f)
    voxels, capacity = L.dense_map_size(s), int(s.get_param("DenseMapCapacity"))
    P, t, _ = s.trajectory()
    P2 = P.copy()
    P2[:, 0, 3] += 0.01 * np.arange(P.shape[0])  # up to half a metre at the end: several leaves
    P2[:, 1, 3] -= 0.003 * np.arange(P.shape[0])
    runs = []
    for poses in (P2, P):
        t0 = time.perf_counter()
        s.set_trajectory(poses, t)
        wall = time.perf_counter() - t0
        runs.append(dict(reproject_s=s.get_param("DenseMapReprojectSeconds"), set_trajectory_wall_s=wall, voxels_after=L.dense_map_size(s)))
    t0 = time.perf_counter()
    L.dense_map(s, 1)
    case = dict(what="reproject", model=a.model, frames=a.frames, leaf=leaf, voxels=voxels, capacity=capacity, table_bytes=68 * capacity,
                reprojections=int(s.get_param("DenseMapReprojections")), clears=int(s.get_param("DenseMapClears")), dropped=int(s.get_param("DenseMapDropped")), runs=runs,
                export_device_and_download_s=s.get_param("DenseMapExportSeconds"), export_wall_s=time.perf_counter() - t0)
    if a.tag:
        case["tag"] = a.tag
    with open(a.out, "a") as out:
        out.write(json.dumps(case) + "\n")
    print(case, flush=True)
    s.close()
