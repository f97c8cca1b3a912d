"""Load / save times of a synthetic map of a few million points, per format, device maps and host maps, both forms of the kernels."""
import json, os, sys, time
import numpy as np
sys.path.insert(0, os.getcwd())
import lidarslam_amd as L

N = 3_000_000
REPS = 5
out = open("profiles/map_io.jsonl", "w")
rng = np.random.default_rng(1)
pts = np.zeros(N, L.POINT_DTYPE)
pts["x"], pts["y"], pts["z"] = rng.uniform(-200, 200, N), rng.uniform(-200, 200, N), rng.uniform(-5, 15, N)
pts["w"] = 1; pts["time"] = rng.uniform(0, 100, N); pts["intensity"] = rng.uniform(0, 255, N); pts["laser_id"] = rng.integers(0, 64, N)
d = "_t_map_io"; os.makedirs(d, exist_ok=True)
paths = {}
for fmt in range(3):
    paths[fmt] = f"{d}/cloud_{fmt}.pcd"
    t = time.perf_counter(); L.write_pcd(paths[fmt], pts, fmt); print("wrote", fmt, time.perf_counter() - t, os.path.getsize(paths[fmt]), flush=True)

def emit(**kw):
    out.write(json.dumps(kw) + "\n"); out.flush(); print(kw, flush=True)

ctx = L.Context(0)
ctx.profile(True)
def scopes():
    return {s["name"]: s for s in ctx.profile_stats() if s["name"] in ("pcd_upload", "pcd_decode", "pcd_encode", "map_add")}
g = L.DeviceGrid(ctx, LeafSize=0.2)
for lds in (0, 1):
    ctx.debug_set("pcd_lds", lds)
    for fmt in range(3):
        rows = []
        for rep in range(REPS + 1):
            g.clear(); ctx.sync(); ctx.profile_reset()
            t = time.perf_counter(); g.add_pcd(paths[fmt], time=1.0); n = g.size(); wall = time.perf_counter() - t
            T = g.pcd_io_times(); s = scopes()
            rows.append(dict(wall=wall, file=T[0], lzf=T[1], text=T[2], pieces=T[3], add=T[4], bytes=T[5],
                             upload_ms=s.get("pcd_upload", {}).get("total_ms", 0), decode_ms=s.get("pcd_decode", {}).get("total_ms", 0), decode_bytes=s.get("pcd_decode", {}).get("bytes", 0), add_ms=s.get("map_add", {}).get("total_ms", 0), voxels=n))
        rows = rows[1:]
        med = {k: float(np.median([r[k] for r in rows])) for k in rows[0]}
        med["decode_GBps"] = med["decode_bytes"] / (med["decode_ms"] * 1e-3) / 1e9 if med["decode_ms"] else 0
        emit(what="load", maps="device", fmt=L.PCD_FORMAT_NAMES[fmt], lds=lds, points=N, reps=REPS, **med)
    for fmt in range(3):
        rows = []
        for rep in range(REPS + 1):
            ctx.sync(); ctx.profile_reset()
            t = time.perf_counter(); n = g.save_pcd(f"{d}/saved_{fmt}.pcd", fmt); wall = time.perf_counter() - t
            T = g.pcd_io_times(); s = scopes()
            rows.append(dict(wall=wall, file=T[0], lzf=T[1], text=T[2], pieces=T[3], get=T[4], bytes=T[5], encode_ms=s.get("pcd_encode", {}).get("total_ms", 0), encode_bytes=s.get("pcd_encode", {}).get("bytes", 0), points_saved=n))
        rows = rows[1:]
        med = {k: float(np.median([r[k] for r in rows])) for k in rows[0]}
        med["encode_GBps"] = med["encode_bytes"] / (med["encode_ms"] * 1e-3) / 1e9 if med["encode_ms"] else 0
        emit(what="save", maps="device", fmt=L.PCD_FORMAT_NAMES[fmt], lds=lds, points=N, reps=REPS, **med)
ctx.debug_set("pcd_lds", -1)
g.close(); ctx.close()
# host maps: decode on the host, the host grid's Add
h = L.RollingGrid(LeafSize=0.2, AddThreads=4)
for fmt in range(3):
    rows = []
    for rep in range(3):
        h.clear()
        t = time.perf_counter(); p = L.read_pcd(paths[fmt]); t1 = time.perf_counter(); h.add(p, time=1.0); t2 = time.perf_counter()
        rows.append(dict(read=t1 - t, add=t2 - t1, wall=t2 - t))
    emit(what="load", maps="host", fmt=L.PCD_FORMAT_NAMES[fmt], points=N, reps=3, **{k: float(np.median([r[k] for r in rows])) for k in rows[0]})
for fmt in range(3):
    rows = []
    for rep in range(3):
        t = time.perf_counter(); p = h.get(); t1 = time.perf_counter(); L.write_pcd(f"{d}/hsaved_{fmt}.pcd", p, fmt); t2 = time.perf_counter()
        rows.append(dict(get=t1 - t, write=t2 - t1, wall=t2 - t))
    emit(what="save", maps="host", fmt=L.PCD_FORMAT_NAMES[fmt], points=N, reps=3, **{k: float(np.median([r[k] for r in rows])) for k in rows[0]})
import shutil; shutil.rmtree(d)
