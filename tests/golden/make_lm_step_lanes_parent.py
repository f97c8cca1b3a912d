#!/usr/bin/env python3
"""Records tests/golden/lm_step_lanes_parent.npz: what lsa_solve_device returns for the cases of tests/lm_step_lanes_cases.py.

Run ONCE on an MI355X with the library of the commit BEFORE the change that is to be pinned, never with the code under test:

    git worktree add ../parent <commit> && make -C ../parent/lidarslam_amd/csrc
    LSA_LIB=../parent/lidarslam_amd/liblidarslam_amd.so python tests/golden/make_lm_step_lanes_parent.py --commit <commit>

Contents: `commit` (the commit whose library wrote the file), `names`, and per case its inputs (`rings`, `two_d`, `w0` -- for
a restarted case the start point the recorded library derived --, `max_iter`, `min_matches`, `give_up_block`, `restart_of`,
`yaw_turns`) and `result` (45 doubles, see lm_solve_pinned_cases.RESULT_DOUBLES).  Every sensor model's cases are run twice
and must come out the same before they are written, and the record must hold the branches the cases are there for
(lm_step_lanes_cases.py; tests/test_gpu_lm_step_lanes.py asserts the same of the file).
"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

import lidarslam_amd as L  # noqa: E402
import lm_solve_pinned_cases as PC  # noqa: E402
import lm_step_lanes_cases as SC  # noqa: E402
from oracle import oracle as O  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="the commit the library in use was built from")
    ap.add_argument("--out", default=os.path.join(HERE, "lm_step_lanes_parent.npz"))
    args = ap.parse_args()
    ctx = L.Context(0)
    all_cases = SC.cases()
    results = {}
    for model in SC.MODELS:
        kps = PC.keypoints(O, L, model)
        a, b = SC.run_model(ctx, L, model, kps), SC.run_model(ctx, L, model, kps)
        for name in a:
            assert np.array_equal(a[name].view(np.uint64), b[name].view(np.uint64)), f"{name}: two runs differ"
            r = a[name]
            print(f"{name:34s} code {int(r[42])} successful {int(r[37])} unsuccessful {int(r[38])} iterations {int(r[39])} evaluations {int(r[40])} matches {int(r[43])} final cost {r[7]!r}")
        results.update(a)
    ctx.close()
    starts = np.stack([SC.start_point(c, results) for c in all_cases])
    out = {
        "commit": np.array(args.commit),
        "names": np.array([c[0] for c in all_cases]),
        "rings": np.array([c[1] for c in all_cases], np.int32),
        "two_d": np.array([int(c[2]) for c in all_cases], np.int32),
        "w0": starts,
        "max_iter": np.array([c[4] for c in all_cases], np.int32),
        "min_matches": np.array([c[5] for c in all_cases], np.int64),
        "give_up_block": np.array([c[6] for c in all_cases], np.int32),
        "restart_of": np.array([c[7] or "" for c in all_cases]),
        "yaw_turns": np.array([c[8] for c in all_cases], np.int32),
        "result": np.stack([results[c[0]] for c in all_cases]),
    }
    res = results
    unsuccessful = [n for n, r in res.items() if r[38] >= 1]
    codes = sorted({int(r[42]) for r in res.values()})
    twice = [s for s in ("r16_3d_wild_a", "r16_3d_wild_b", "r16_2d_wild_a", "r16_2d_wild_b") if any(k + 1 in SC.rejected_iterations(res, s) for k in SC.rejected_iterations(res, s))]
    print(f"cases with rejected steps: {len(unsuccessful)}; termination codes: {codes}; two rejections in a row: {twice}")
    assert len(unsuccessful) >= 3 and len(codes) >= 5 and twice, "the record does not hold the branches it is there for"
    np.savez_compressed(args.out, **out)
    print(f"wrote {args.out}: {len(all_cases)} cases from {args.commit}, library {L._native.LIB_PATH}")


if __name__ == "__main__":
    main()
