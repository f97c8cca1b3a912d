"""The device pose-graph solver timed (Context.pose_graph_solve) on synthetic graphs that need no LiDAR data: --laps laps of a
circle, --poses poses in all, noisy odometry, --loops true loop edges between the laps.  Records the device's wall time, LM
iterations and PCG iterations per LM step; the share of factor / apply / spmv with the profiling scopes on; the host
statement's time for the same graph; and the device solver with the preconditioner reduced to its diagonal blocks
(preconditioner = 1), so that the file itself shows what the cyclic reduction buys.  Appends to profiles/pose_graph.jsonl.
--gps: the GPS case instead -- every pose free, a position prior every --gps_every poses behind a lever arm, in a frame a known
world transform away, the start laid onto the fixes by trajectory_alignment; without loop edges and with --loops of them.
Appends to profiles/pose_graph_gps.jsonl: the device's wall time, LM and PCG iterations, and the host statement's time."""
import argparse, json, os, sys, time
import numpy as np
sys.path.insert(0, os.getcwd())
import lidarslam_amd as L

ap = argparse.ArgumentParser()
ap.add_argument("--poses", type=int, nargs="+", default=[5000, 500])
ap.add_argument("--laps", type=int, default=2)
ap.add_argument("--loops", type=int, default=5)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--diag_pcg_max_iter", type=int, default=20000)
ap.add_argument("--gps", action="store_true")
ap.add_argument("--gps_every", type=int, default=10)
ap.add_argument("--out", default=None)
a = ap.parse_args()
a.out = a.out or ("profiles/pose_graph_gps.jsonl" if a.gps else "profiles/pose_graph.jsonl")
out = open(a.out, "a")


def emit(**kw):
    out.write(json.dumps(kw) + "\n"); out.flush(); print(kw, flush=True)


def rot(phi):
    th = np.linalg.norm(phi)
    S = np.array([[0, -phi[2], phi[1]], [phi[2], 0, -phi[0]], [-phi[1], phi[0], 0]])
    return np.eye(3) + S + 0.5 * S @ S if th < 1e-6 else np.eye(3) + np.sin(th) / th * S + (1 - np.cos(th)) / th**2 * S @ S


def pose(angle):
    T = np.eye(4)
    T[:3, :3] = rot(np.array([0, 0, angle + np.pi / 2])) @ rot(np.array([0.03 * np.sin(3 * angle), 0.02 * np.cos(2 * angle), 0]))
    T[:3, 3] = [20 * np.cos(angle), 20 * np.sin(angle), 0.5 * np.sin(angle)]
    return T


def graph(n, laps, loops, seed=1, gps=0):
    rng = np.random.default_rng(seed)
    truth = [pose(2 * np.pi * laps * i / n) for i in range(n)]
    W = np.diag([1e4] * 3 + [2.5e5] * 3)
    sig = np.array([0.01] * 3 + [0.002] * 3)
    edges, init = [], [truth[0]]
    for i in range(1, n):
        Z = np.linalg.inv(truth[i - 1]) @ truth[i]
        d = sig * rng.standard_normal(6)
        Z[:3, 3] += Z[:3, :3] @ d[:3]
        Z[:3, :3] = Z[:3, :3] @ rot(d[3:])
        edges.append((i - 1, i, Z, W))
        init.append(init[-1] @ Z)
    per_lap = n // laps
    for k in range(loops):  # the same place one lap later
        a0 = 1 + (k * (per_lap - 2)) // max(loops, 1)
        b0 = min(n - 1, a0 + per_lap * (laps - 1))
        edges.append((a0, b0, np.linalg.inv(truth[a0]) @ truth[b0], W))
    fixed = np.zeros(n, np.uint8)
    fixed[0] = 1
    if gps:
        # fixes of 0.03 m at every gps-th pose, seen through a lever arm from a frame 100 m and 0.8 rad away
        Wt, O = np.eye(4), np.eye(4)
        Wt[:3, :3], Wt[:3, 3] = rot(np.array([0, 0, 0.8])) @ rot(np.array([0.02, -0.03, 0])), [100, -50, 10]
        O[:3, :3], O[:3, 3] = rot(np.array([0.1, -0.2, 0.3])), [0.4, -0.3, 1.2]
        priors = [(i, (Wt @ truth[i] @ O)[:3, 3] + 0.03 * rng.standard_normal(3), np.eye(3) / 0.03**2) for i in range(0, n, gps)]
        A = L.trajectory_alignment([(init[i] @ O)[:3, 3] for i, _, _ in priors], [g for _, g, _ in priors])
        return L.pose_graph_premultiply(np.array(init), A), np.zeros(n, np.uint8), L.pose_graph_edges(edges), L.pose_graph_priors(priors), O
    return np.array(init), fixed, L.pose_graph_edges(edges)


ctx = L.Context(0)
if a.gps:
    for n in a.poses:
        for loops in (0, a.loops):
            P, fixed, E, R, O = graph(n, a.laps, loops, gps=a.gps_every)
            case = dict(poses=n, laps=a.laps, loops=loops, edges=int(E.size), priors=int(R.size))
            ctx.pose_graph_solve(P, fixed, E, priors=R, offset=O)  # buffers
            for run in range(a.runs):
                t0 = time.perf_counter()
                dev, r = ctx.pose_graph_solve(P, fixed, E, priors=R, offset=O)
                emit(what="device_gps", run=run, **case, wall_s=time.perf_counter() - t0, lm_iterations=r.iterations, pcg_iterations=r.pcg_iterations,
                     pcg_per_lm=r.pcg_iterations / max(r.iterations, 1), termination=r.termination, initial_cost=r.initial_cost, final_cost=r.final_cost)
            t0 = time.perf_counter()
            host, hr = L.pose_graph_solve_host(P, fixed, E, priors=R, offset=O)
            emit(what="host_statement_gps", **case, wall_s=time.perf_counter() - t0, lm_iterations=hr.iterations, pcg_iterations=hr.pcg_iterations, termination=hr.termination,
                 final_cost=hr.final_cost, max_position_difference_m=float(np.abs(host[:, :3, 3] - dev[:, :3, 3]).max()))
    ctx.close()
    sys.exit(0)
for n in a.poses:
    P, fixed, E = graph(n, a.laps, a.loops)
    case = dict(poses=n, laps=a.laps, loops=a.loops, edges=int(E.size))
    ctx.pose_graph_solve(P, fixed, E)  # buffers
    for run in range(a.runs):
        t0 = time.perf_counter()
        dev, r = ctx.pose_graph_solve(P, fixed, E)
        emit(what="device", run=run, **case, wall_s=time.perf_counter() - t0, lm_iterations=r.iterations, pcg_iterations=r.pcg_iterations,
             pcg_per_lm=r.pcg_iterations / max(r.iterations, 1), termination=r.termination, initial_cost=r.initial_cost, final_cost=r.final_cost)
    ctx.profile(True)
    ctx.profile_reset()
    t0 = time.perf_counter()
    ctx.pose_graph_solve(P, fixed, E)
    wall = time.perf_counter() - t0
    stats = {s["name"]: (s["launches"], s["total_ms"]) for s in ctx.profile_stats() if s["name"].startswith("pgo_")}
    ctx.profile(False)
    emit(what="device_profiled", **case, wall_s=wall, scopes_launches_ms=stats)
    t0 = time.perf_counter()
    host, hr = L.pose_graph_solve_host(P, fixed, E)
    emit(what="host_statement", **case, wall_s=time.perf_counter() - t0, lm_iterations=hr.iterations, pcg_iterations=hr.pcg_iterations, termination=hr.termination,
         final_cost=hr.final_cost, max_position_difference_m=float(np.abs(host[:, :3, 3] - dev[:, :3, 3]).max()))
    t0 = time.perf_counter()
    _, dr = ctx.pose_graph_solve(P, fixed, E, preconditioner=1, pcg_max_iter=a.diag_pcg_max_iter)
    emit(what="device_block_jacobi", **case, wall_s=time.perf_counter() - t0, lm_iterations=dr.iterations, pcg_iterations=dr.pcg_iterations,
         pcg_per_lm=dr.pcg_iterations / max(dr.iterations, 1), pcg_truncated=dr.pcg_truncated, termination=dr.termination, final_cost=dr.final_cost)
ctx.close()
