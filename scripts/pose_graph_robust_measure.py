"""Robust losses in the device pose-graph solver, timed on the synthetic graphs of scripts/pose_graph_measure.py (DESIGN.md 3.9:
--laps laps of a circle, --poses poses in all, noisy odometry, --loops true loop edges between the laps) with --false false
loop edges added: true loops of other places moved by 50 m.  Per graph, --runs runs each, in one session:
  existing_clean     Context.pose_graph_solve (lsa_pgo_solve) on the graph WITHOUT the false edges -- the figure of
                     profiles/pose_graph.jsonl, and the solve every other one is compared with ("distance_to_clean_m")
  existing           the same entry on the graph with the false edges
  robust_<loss>      pose_graph_solve_robust (lsa_pgo_solve_robust) with each loss on the loop edges at --scale sigmas, verdicts
                     asked for
with the host's wall time, LM and PCG iterations, the termination and the weights of the true and the false loops.  The loops of
these graphs claim 0.01 m / 0.002 rad while the odometry has drifted by metres when they close, so the default scale is 300
sigmas (3 m): below the drift a loss that is flat beyond its scale lets go of the true loops with the false ones.
Appends to profiles/pose_graph_robust.jsonl.  --host: the host statement instead of the device (for a machine without one)."""
import argparse, json, os, sys, time
import numpy as np
sys.path.insert(0, os.getcwd())
import lidarslam_amd as L

ap = argparse.ArgumentParser()
ap.add_argument("--poses", type=int, nargs="+", default=[5000, 500])
ap.add_argument("--laps", type=int, default=2)
ap.add_argument("--loops", type=int, default=5)
ap.add_argument("--false", type=int, default=2, dest="false_loops")
ap.add_argument("--scale", type=float, default=300.0)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--host", action="store_true")
ap.add_argument("--out", default="profiles/pose_graph_robust.jsonl")
a = ap.parse_args()
out = open(a.out, "a")
LOSSES = ["none", "huber", "geman_mcclure", "tukey"]


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


def graph(n, laps, loops, false_loops, seed=1):
    """scripts/pose_graph_measure.py's graph (the same draws), then the false loops behind the true ones"""
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
    for k in range(false_loops):  # another place claimed 50 m from where it is
        a0, b0 = n // 7 + k * (n // 5), n - 1 - n // 9 - k * (n // 4)
        Z = np.linalg.inv(truth[a0]) @ truth[b0]
        Z[:3, 3] += [30.0, -40.0, 0.0]
        edges.append((a0, b0, Z, W))
    fixed = np.zeros(n, np.uint8)
    fixed[0] = 1
    return np.array(init), fixed, L.pose_graph_edges(edges)


ctx = None if a.host else L.Context(0)
for n in a.poses:
    P, fixed, E = graph(n, a.laps, a.loops, a.false_loops)
    m, chain = int(E.size), n - 1
    clean_E = E[: chain + a.loops]
    mask = np.zeros(m, np.uint8)
    mask[chain:] = 1
    true_loops, false_loops = slice(chain, chain + a.loops), slice(chain + a.loops, m)
    case = dict(poses=n, laps=a.laps, loops=a.loops, false_loops=a.false_loops, edges=m, scale=a.scale, where="host" if a.host else "device")
    start_chi2 = L.pose_graph_linearize(P, E)[2]
    emit(what="start", **case, true_loop_chi2=[float(v) for v in start_chi2[true_loops]], false_loop_chi2=[float(v) for v in start_chi2[false_loops]])
    L.pose_graph_solve(P, fixed, clean_E, ctx)  # buffers
    for run in range(a.runs):
        t0 = time.perf_counter()
        clean, r = L.pose_graph_solve(P, fixed, clean_E, ctx)
        emit(what="existing_clean", run=run, **case, wall_s=time.perf_counter() - t0, lm_iterations=r.iterations, pcg_iterations=r.pcg_iterations, termination=r.termination,
             initial_cost=r.initial_cost, final_cost=r.final_cost)
    for run in range(a.runs):
        t0 = time.perf_counter()
        bent, r = L.pose_graph_solve(P, fixed, E, ctx)
        emit(what="existing", run=run, **case, wall_s=time.perf_counter() - t0, lm_iterations=r.iterations, pcg_iterations=r.pcg_iterations, termination=r.termination,
             initial_cost=r.initial_cost, final_cost=r.final_cost, distance_to_clean_m=float(np.abs(bent[:, :3, 3] - clean[:, :3, 3]).max()))
    for loss, name in enumerate(LOSSES):
        rb = L.PoseGraphRobust(edge_loss=loss, edge_scale=a.scale)
        for run in range(a.runs):
            t0 = time.perf_counter()
            got, r, ev, _ = L.pose_graph_solve_robust(P, fixed, E, rb, mask=mask, ctx=ctx)
            emit(what="robust_" + name, run=run, **case, wall_s=time.perf_counter() - t0, lm_iterations=r.iterations, pcg_iterations=r.pcg_iterations, termination=r.termination,
                 initial_cost=r.initial_cost, final_cost=r.final_cost, distance_to_clean_m=float(np.abs(got[:, :3, 3] - clean[:, :3, 3]).max()),
                 true_loop_weights=[float(v) for v in ev[true_loops, 1]], false_loop_weights=[float(v) for v in ev[false_loops, 1]])
if ctx is not None:
    ctx.close()
