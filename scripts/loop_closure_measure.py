"""One loop-closure registration timed (Slam.register_logged_frames): a VLS-128 log of --frames frames, the frame --query
registered against the window of --half-window frames around --revisited, --runs times; wall time of the call and the shares
of its stages (the two replays, the scratch maps' insertion and sub-map, the ICP loop) from the library's own clocks; and,
as the reference point, the time the same registration takes when it is composed of the CPU oracle's primitives on the logged
keypoints (what a caller without this call would do after downloading them).  Appends to profiles/loop_closure.jsonl."""
import argparse, json, os, sys, time
import numpy as np
sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import lidarslam_amd as L

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=40)
ap.add_argument("--model", type=int, default=128)
ap.add_argument("--query", type=int, default=35)
ap.add_argument("--revisited", type=int, default=10)
ap.add_argument("--half-window", type=int, default=5)
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--oracle", type=int, default=1)
ap.add_argument("--out", default="profiles/loop_closure.jsonl")
a = ap.parse_args()
out = open(a.out, "a")


def emit(**kw):
    out.write(json.dumps(kw) + "\n"); out.flush(); print(kw, flush=True)


s = L.Slam(0, EgoMotion=3, LoggingTimeout=-1)
for f in range(a.frames):
    pts, stamp = L.synth_frame(a.model, 1000, f)
    s.add_frame(pts, stamp, f)
P, t, _ = s.trajectory()
lp = L.LoopClosureParams(revisited_half_window=a.half_window, query_half_window=0, icp_max_iter=6, lm_max_iter=15, init_saturation=2.0, final_saturation=0.5)
guess = P[a.query].copy()
guess[:3, 3] += [0.18, 0.24, 0.0]  # 0.3 m off the logged pose
case = dict(model=a.model, frames=a.frames, query=a.query, revisited=a.revisited, half_window=a.half_window)
for run in range(a.runs):
    t0 = time.perf_counter()
    r = s.register_logged_frames(a.query, a.revisited, lp, guess)
    wall = time.perf_counter() - t0
    emit(what="register_logged_frames", run=run, **case, wall_s=wall, replay_s=s.get_param("LoopClosureReplaySeconds"), maps_s=s.get_param("LoopClosureMapsSeconds"),
         icp_s=s.get_param("LoopClosureIcpSeconds"), inside_s=s.get_param("LoopClosureSeconds"), status=r.status, iterations=r.iterations,
         target_points=r.target_points.tolist(), query_points=r.query_points.tolist(), matched_last=[int(r.last_histogram[k][0]) for k in range(3)],
         from_logged_pose_m=float(np.linalg.norm(r.world[:3, 3] - P[a.query][:3, 3])), position_error=r.position_error)
if a.oracle:
    from oracle import oracle as O
    import test_gpu_loop_closure as T
    T.ICP_MAX_ITER, T.LM_MAX_ITER, T.INIT_SAT, T.FINAL_SAT = 6, 15, 2.0, 0.5
    t0 = time.perf_counter()
    lo, hi = max(a.revisited - a.half_window, 0), min(a.revisited + a.half_window, a.frames - 1)
    raw = [[s.logged_keypoints(i, k) if (lo <= i <= hi or i == a.query) else np.zeros(0, L.POINT_DTYPE) for k in range(3)] for i in range(a.frames)]
    download = time.perf_counter() - t0
    ref = T.reference_registration(L, O, s, P, t, raw, a.query, a.revisited, a.half_window, 0, guess)
    wall = time.perf_counter() - t0
    d = np.linalg.inv(ref["world"]) @ r.world
    emit(what="oracle_composition", **case, wall_s=wall, download_s=download, iterations=ref["iterations"], target_points=ref["target_points"].tolist(),
         device_minus_oracle_m=float(np.linalg.norm(d[:3, 3])))
s.close()
