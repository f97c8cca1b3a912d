"""Place recognition timed (Slam.recognize_place): a VLS-128 log of --frames frames; host wall time of the first call for
the last frame (describes every logged frame, then searches), of --runs further calls (search only: one launch, one copy,
one wait), and of the same query answered by the host statement on downloaded keypoints (L.scan_descriptor,
L.place_distance, L.place_select) -- the only reference there is for a time, the library having had no such call before.
--profile 1: then --runs more search-only calls with profiling on, for the event time of the "place_search" scope (the
search kernel's launch).  --tag goes into every line (which build was measured).
Appends to profiles/place_recognition.jsonl."""
import argparse, json, os, sys, time
import numpy as np
sys.path.insert(0, os.getcwd())
import lidarslam_amd as L

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=200)
ap.add_argument("--model", type=int, default=128)
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--host", type=int, default=1)
ap.add_argument("--profile", type=int, default=0)
ap.add_argument("--tag", default="")
ap.add_argument("--out", default="profiles/place_recognition.jsonl")
a = ap.parse_args()
out = open(a.out, "a")


def emit(**kw):
    if a.tag:
        kw["tag"] = a.tag
    out.write(json.dumps(kw) + "\n"); out.flush(); print(kw, flush=True)


s = L.Slam(0, EgoMotion=3, LoggingTimeout=-1)
for f in range(a.frames):
    pts, stamp = L.synth_frame(a.model, 1000, f)
    s.add_frame(pts, stamp, f)
P, t, _ = s.trajectory()
query = a.frames - 1
search = dict(min_travelled=2.0, max_distance=0.0, exclusion_half_window=5)
keypoints = [sum(s.context().kplog_count(i, k) for k in (L.EDGE, L.PLANE)) for i in range(a.frames)]
case = dict(model=a.model, frames=a.frames, query=query, rings=20, sectors=60, keypoints_per_frame=float(np.mean(keypoints)))
t0 = time.perf_counter()
first = s.recognize_place(query, capacity=5, **search)
emit(what="recognize_place_first_call", **case, wall_s=time.perf_counter() - t0, described=s.context().kplog_described(), candidates=[(c[0], float(c[1]), c[2]) for c in first])
for run in range(a.runs):
    t0 = time.perf_counter()
    again = s.recognize_place(query, capacity=5, **search)
    emit(what="recognize_place_search_only", run=run, **case, wall_s=time.perf_counter() - t0, described=s.context().kplog_described(), same=again == first)
if a.profile:
    ctx = s.context()
    ctx.profile(True)
    ctx.profile_reset()
    for run in range(a.runs):
        s.recognize_place(query, capacity=5, **search)
    ctx.sync()
    stat = {k["name"]: k for k in ctx.profile_stats()}["place_search"]
    ctx.profile(False)
    emit(what="place_search_scope", **case, total_ms=stat["total_ms"], launches=stat["launches"], event_overhead_us=ctx.profile_event_overhead_us())
if a.host:
    t0 = time.perf_counter()
    raw = [np.concatenate([s.logged_keypoints(i, k) for k in (L.EDGE, L.PLANE)]) for i in range(a.frames)]
    download = time.perf_counter() - t0
    desc = [L.scan_descriptor(r) for r in raw]
    describe = time.perf_counter() - t0 - download
    table = [L.place_distance(desc[query], desc[i]) for i in range(query)]
    ref = L.place_select([d for d, _ in table], [sh for _, sh in table], P, t, query, capacity=5, **search)
    wall = time.perf_counter() - t0
    emit(what="host_statement", **case, wall_s=wall, download_s=download, describe_s=describe, search_s=wall - download - describe, same=ref == first)
s.close()
