"""Loop detection over the whole log timed (L.detect_loop_closures): a VLS-128 log of --frames frames, every
frame a query, the descriptors present.
  whole_log     host wall time of one detect_loop_closures against the loop of Slam.recognize_place over the same queries (the
                only way to ask before; its code is untouched, so the loop run here is the parent commit's), alternated,
                --runs each; the two must give the same candidates
  kernel        event time (ProfScope) of k_place_search_rows per computed pair -- four columns at a time, and one at a time
                (lsa_debug_set "place_untiled"), the scope "place_search_rows" -- against k_place_search's over the loop of
                recognitions (the scope "place_search"), at 20 x 60 and 32 x 120, in a run of its own with profiling on
  gates         pairs computed / pairs total with max_distance = 30 m
--tag goes into every line (which build was measured).  Appends to profiles/loop_detection.jsonl."""
import argparse, json, os, sys, time
import numpy as np
sys.path.insert(0, os.getcwd())
import lidarslam_amd as L

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=200)
ap.add_argument("--model", type=int, default=128)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--tag", default="")
ap.add_argument("--out", default="profiles/loop_detection.jsonl")
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
n = a.frames
ctx = s.context()
search = dict(min_travelled=2.0, max_distance=0.0, exclusion_half_window=5)
gated = dict(search, max_distance=30.0)
case = dict(model=a.model, frames=n, queries=n, per_query=5)


def loop_of_recognitions(**params):
    return [(q,) + c for q in range(n) for c in s.recognize_place(q, capacity=5, **search, **params)]


def pairs_computed(**gates):
    """what the gates leave of the pairs i < q, by the definition's arithmetic in float64 (a count, not a result)"""
    xyz = P[:, :3, 3]
    way = np.concatenate([[0.0], np.cumsum(np.linalg.norm(np.diff(xyz, axis=0), axis=1))])
    total = 0
    for q in range(n):
        ok = way[q] - way[:q] >= gates.get("min_travelled", 0.0)
        if gates.get("max_distance", 0.0) > 0:
            ok &= np.linalg.norm(xyz[:q] - xyz[q], axis=1) <= gates["max_distance"]
        total += int(ok.sum())
    return total


for shape in (dict(rings=20, sectors=60), dict(rings=32, sectors=120, type_mask=7)):
    first = L.detect_loop_closures(s, per_query=5, **search, **shape)  # describes what is missing
    walls = {"detect_loop_closures": [], "recognize_place_loop": []}
    same = True
    for run in range(a.runs):
        t0 = time.perf_counter()
        got = L.detect_loop_closures(s, per_query=5, **search, **shape)
        walls["detect_loop_closures"].append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        ref = loop_of_recognitions(**shape)
        walls["recognize_place_loop"].append(time.perf_counter() - t0)
        same = same and got == ref == first
    emit(what="whole_log", **case, **shape, wall_s=walls, same=same, candidates=len(first), pairs=n * (n - 1) // 2, pairs_computed=pairs_computed(**search))
    # kernel time per computed pair, profiling on (events around every launch): a run of its own
    ctx.profile(True)
    for run in range(a.runs):
        ctx.profile_reset()
        L.detect_loop_closures(s, per_query=5, **search, **shape)
        ctx.sync()
        rows = {k["name"]: k for k in ctx.profile_stats()}
        ctx.debug_set("place_untiled", 1)
        ctx.profile_reset()
        L.detect_loop_closures(s, per_query=5, **search, **shape)
        ctx.sync()
        untiled = {k["name"]: k for k in ctx.profile_stats()}
        ctx.debug_set("place_untiled", 0)
        ctx.profile_reset()
        loop_of_recognitions(**shape)
        ctx.sync()
        one = {k["name"]: k for k in ctx.profile_stats()}
        emit(what="kernel", run=run, **case, **shape, search_rows_ms=rows["place_search_rows"]["total_ms"], search_rows_launches=rows["place_search_rows"]["launches"],
             search_rows_untiled_ms=untiled["place_search_rows"]["total_ms"], select_rows_ms=rows["place_select_rows"]["total_ms"], pairs_computed=pairs_computed(**search),
             place_search_ms=one["place_search"]["total_ms"], place_search_launches=one["place_search"]["launches"], pairs_of_the_loop=n * (n - 1) // 2,
             event_overhead_us=ctx.profile_event_overhead_us())
        # the same with the position gate at 30 m: what the gates skip
        ctx.profile_reset()
        t0 = time.perf_counter()
        got = L.detect_loop_closures(s, per_query=5, **gated, **shape)
        wall = time.perf_counter() - t0
        ctx.sync()
        rows = {k["name"]: k for k in ctx.profile_stats()}
        emit(what="gates", run=run, **case, **shape, max_distance=30.0, wall_s_profiling_on=wall, search_rows_ms=rows["place_search_rows"]["total_ms"],
             select_rows_ms=rows["place_select_rows"]["total_ms"], pairs=n * (n - 1) // 2, pairs_computed=pairs_computed(**gated), candidates=len(got))
    ctx.profile(False)
s.close()
