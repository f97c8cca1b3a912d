"""Place recognition against the maps timed (recognize_place_in_maps): the maps of a VLS-128 drive of --frames frames, a
viewpoint at every logged position, the query the last frame's raw keypoints.  Host wall time of the first call (describes the
maps at every viewpoint, then searches), of --runs further calls (search only: the query's descriptor, one search launch, one
copy, one wait), of a description with the slices out of reach passed over and with all of them read ("map_describe_cull"),
and of the same answer from the host statement on the downloaded maps (L.map_descriptor, L.place_distance,
L.map_place_select) -- the only reference there is for a time, the library having had no such call before.  One run each.
--viewpoints N ...: instead of a viewpoint at every logged position, the last N of them (a search among one or four
candidates), first call and search-only calls for each N; --profile 1: then --runs more search-only calls with profiling on,
for the event time of the "place_search" scope.  --tag goes into every line (which build was measured).
--strip N: instead, a made-up map much longer than the descriptor's reach -- N points on a strip of --strip-km sorted along it,
a viewpoint every 2 m -- described from an uploaded array (map_place_describe) with the cull on and off: what passing slices
over is worth where most of them are out of reach.  Appends to profiles/map_place.jsonl."""
import argparse, json, os, sys, time
import numpy as np
sys.path.insert(0, os.getcwd())
import lidarslam_amd as L

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=200)
ap.add_argument("--model", type=int, default=128)
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--host", type=int, default=1)
ap.add_argument("--strip", type=int, default=0)
ap.add_argument("--strip-km", type=float, default=4.0)
ap.add_argument("--viewpoints", type=int, nargs="*", default=[0])
ap.add_argument("--profile", type=int, default=0)
ap.add_argument("--tag", default="")
ap.add_argument("--out", default="profiles/map_place.jsonl")
a = ap.parse_args()
out = open(a.out, "a")


def emit(**kw):
    if a.tag:
        kw["tag"] = a.tag
    out.write(json.dumps(kw) + "\n"); out.flush(); print(kw, flush=True)


def brief(found):
    return [(c[0], float(c[1]), c[2]) for c in found]


if a.strip > 0:
    rng = np.random.default_rng(1)
    length = 1000.0 * a.strip_km
    pts = np.zeros(a.strip, L.POINT_DTYPE)
    pts["x"], pts["y"], pts["z"] = np.sort(rng.uniform(0, length, a.strip)), rng.uniform(-30, 30, a.strip), rng.uniform(-2, 6, a.strip)
    vp = np.zeros((int(length / 2), 3))
    vp[:, 0] = 2.0 * np.arange(vp.shape[0])
    ctx = L.Context(0)
    L.map_place_describe(ctx, pts[:1000], vp[:10])  # (the first launches of a process)
    tables = {}
    for k, cull in enumerate((1, 0, 1, 0)):
        ctx.debug_set("map_describe_cull", cull)
        t0 = time.perf_counter()
        L.map_place_describe(ctx, pts, vp)
        wall = time.perf_counter() - t0
        tables[cull] = L.map_place_descriptors(ctx, 0, vp.shape[0] - 1).tobytes()
        emit(what="strip_describe_points", cull=cull, run=k // 2, points=a.strip, strip_km=a.strip_km, viewpoints=int(vp.shape[0]), rings=20, sectors=60,
             slices=int(L.map_place_slices(ctx).shape[0]), wall_s=wall, includes="upload of the points, slice boxes, description, one wait")
    emit(what="strip_cull_on_equals_off", same=tables[1] == tables[0])
    ctx.close()
    sys.exit(0)

s = L.Slam(0, EgoMotion=3, LoggingTimeout=-1)
for f in range(a.frames):
    pts, stamp = L.synth_frame(a.model, 1000, f)
    s.add_frame(pts, stamp, f)
P, _, _ = s.trajectory()
ctx = s.context()
for nv in a.viewpoints:
    vp = P[-nv:, :3, 3].copy()  # (nv = 0: all of them)
    t0 = time.perf_counter()
    first, summary = L.recognize_place_in_maps(s, vp, capacity=5)
    wall = time.perf_counter() - t0
    case = dict(model=a.model, frames=a.frames, viewpoints=int(vp.shape[0]), rings=20, sectors=60, map_points=[int(v) for v in summary.map_points],
                query_points=[int(v) for v in summary.query_points], way_m=float(np.linalg.norm(np.diff(P[:, :3, 3], axis=0), axis=1).sum()))
    emit(what="first_call_describe_and_search", **case, wall_s=wall, described=summary.described, candidates=brief(first))
    for run in range(a.runs):
        t0 = time.perf_counter()
        again, summary = L.recognize_place_in_maps(s, vp, capacity=5)
        emit(what="search_only", run=run, **case, wall_s=time.perf_counter() - t0, described=summary.described, same=brief(again) == brief(first))
    if a.profile:
        ctx.profile(True)
        ctx.profile_reset()
        for run in range(a.runs):
            L.recognize_place_in_maps(s, vp, capacity=5)
        ctx.sync()
        stat = {k["name"]: k for k in ctx.profile_stats()}["place_search"]
        ctx.profile(False)
        emit(what="place_search_scope", **case, total_ms=stat["total_ms"], launches=stat["launches"], event_overhead_us=ctx.profile_event_overhead_us())
if a.viewpoints != [0]:
    s.close()
    sys.exit(0)
# a description again (viewpoint 0 moved by a nanometre, so that the table is not kept), slices out of reach passed over or not
boxes = L.map_place_slices(ctx)
reach = 80.0 * (1.0 + 2.0 ** -20)
dx = np.maximum(np.maximum(boxes[None, :, 0] - vp[:, None, 0], vp[:, None, 0] - boxes[None, :, 2]), 0.0)
dy = np.maximum(np.maximum(boxes[None, :, 1] - vp[:, None, 1], vp[:, None, 1] - boxes[None, :, 3]), 0.0)
far = dx * dx + dy * dy > reach * reach
for k, cull in enumerate((1, 0, 1, 0)):
    ctx.debug_set("map_describe_cull", cull)
    moved = vp.copy()
    moved[0, 0] += 1e-9 * (k + 1)
    t0 = time.perf_counter()
    again, summary = L.recognize_place_in_maps(s, moved, capacity=5)
    emit(what="describe_and_search_again", cull=cull, **case, wall_s=time.perf_counter() - t0, described=summary.described, slices=int(boxes.shape[0]),
         pairs_out_of_reach=int(far.sum()), pairs=int(far.size), same=brief(again) == brief(first))
ctx.debug_set("map_describe_cull", 1)
if a.host:
    t0 = time.perf_counter()
    maps = np.concatenate([s.map(k) for k in (L.EDGE, L.PLANE)])
    query = np.concatenate([s.keypoints(k, which=2) for k in (L.EDGE, L.PLANE)])
    download = time.perf_counter() - t0
    dq = L.scan_descriptor(query)
    table = [L.map_descriptor(maps, v) for v in vp]
    describe = time.perf_counter() - t0 - download
    pairs = [L.place_distance(dq, d) for d in table]
    ref = L.map_place_select([d for d, _ in pairs], [sh for _, sh in pairs], vp, capacity=5)
    wall = time.perf_counter() - t0
    emit(what="host_statement", **case, wall_s=wall, download_s=download, describe_s=describe, search_s=wall - download - describe, same=brief(ref) == brief(first))
s.close()
