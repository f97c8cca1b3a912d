"""The rebuild of the maps from the keypoint log under a corrected trajectory, timed: a VLS-128 log of --frames frames,
Slam.set_trajectory with the maps on the device and with MapsOnDevice = 0, alternating, three runs each; the bytes the log
holds; k_log_replay's own time from the context's profiling scope (HIP events).  Appends to profiles/trajectory_rebuild.jsonl.
Under `rocprofv3 --kernel-trace --stats -- python scripts/trajectory_rebuild_measure.py --maps device --runs 3` the kernel's
time comes from the tool instead."""
import argparse, json, os, sys, time
import numpy as np
sys.path.insert(0, os.getcwd())
import lidarslam_amd as L

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=200)
ap.add_argument("--model", type=int, default=128)
ap.add_argument("--maps", default="both", choices=["both", "device", "host"])
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--out", default="profiles/trajectory_rebuild.jsonl")
a = ap.parse_args()
out = open(a.out, "a")


def emit(**kw):
    out.write(json.dumps(kw) + "\n"); out.flush(); print(kw, flush=True)


def bend(P, sign):
    Q = []
    for i, Pi in enumerate(P):
        c, s = np.cos(sign * 0.0002 * i), np.sin(sign * 0.0002 * i)
        C = np.eye(4); C[:2, :2] = [[c, -s], [s, c]]; C[:3, 3] = sign * 0.005 * i * np.array([0.6, 0.8, 0.0])
        Q.append(C @ Pi)
    return np.array(Q)


homes = {"both": [1, 0], "device": [1], "host": [0]}[a.maps]
slams = {}
for dev in homes:
    s = L.Slam(0, EgoMotion=3, LoggingTimeout=-1, MapsOnDevice=dev)
    for f in range(a.frames):
        pts, stamp = L.synth_frame(a.model, 1000, f)
        s.add_frame(pts, stamp, f)
    P, t, _ = s.trajectory()
    counts = [sum(s.context().kplog_count(i, k) for i in range(a.frames)) for k in range(3)]
    emit(what="log", maps="device" if dev else "host", model=a.model, frames=a.frames, keypoints=counts, bytes_held=s.get_param("LoggedKeypointsBytes"),
         bytes_of_points=32 * sum(counts), map_points=[int(s.map(k).size) for k in (0, 1)])
    slams[dev] = (s, P, t, counts)
for run in range(a.runs):
    for dev in homes:
        s, P, t, counts = slams[dev]
        ctx = s.context()
        ctx.profile(True); ctx.profile_reset()
        t0 = time.perf_counter()
        try:
            s.set_trajectory(bend(P, 1 if run % 2 == 0 else 0), t)  # in turn the bent trajectory and the logged one
            err = None
        except L.LsaError as e:
            err = str(e)
        n_edges = s.map(0).size  # (waits for the maps: the insertion is enqueued, not waited for, by the call itself)
        wall = time.perf_counter() - t0
        scopes = {x["name"]: x for x in ctx.profile_stats() if x["name"] in ("log_replay", "map_add")}
        ctx.profile(False)
        row = dict(what="set_trajectory", maps="device" if dev else "host", run=run, frames=a.frames, keypoints=sum(counts), wall_s=wall, error=err, map_edges=int(n_edges))
        if "log_replay" in scopes and scopes["log_replay"]["total_ms"] > 0:
            ms, by = scopes["log_replay"]["total_ms"], scopes["log_replay"]["bytes"]
            row.update(replay_ms=ms, replay_bytes=by, replay_GBps=by / (ms * 1e-3) / 1e9, replay_fraction_of_8TBps=by / (ms * 1e-3) / 8e12)
        if "map_add" in scopes:
            row.update(map_add_ms=scopes["map_add"]["total_ms"])
        emit(**row)
for s, *_ in slams.values():
    s.close()
