#!/usr/bin/env python3
"""Records tests/golden/lm_solve_parent.npz: what lsa_solve_device returns for the cases of tests/lm_solve_pinned_cases.py.

Run on an MI355X with the library of the commit BEFORE the change that is to be pinned, never with the code under test:

    git worktree add ../parent <commit> && make -C ../parent/lidarslam_amd/csrc
    LSA_LIB=../parent/lidarslam_amd/liblidarslam_amd.so python tests/golden/make_lm_solve_parent.py --commit <commit>

Contents: `commit` (the commit whose library wrote the file), `names`, and per case its inputs (`rings`, `two_d`, `w0`,
`max_iter`, `min_matches`, `give_up_block`) and `result` (45 doubles, see lm_solve_pinned_cases.RESULT_DOUBLES).  Every
case is solved twice and must come out the same before it is written.
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
from oracle import oracle as O  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="the commit the library in use was built from")
    ap.add_argument("--out", default=os.path.join(HERE, "lm_solve_parent.npz"))
    args = ap.parse_args()
    ctx = L.Context(0)
    all_cases = PC.cases()
    results = {}
    for model in PC.MODELS:
        PC.setup_residuals(ctx, L, PC.keypoints(O, L, model))
        for case in all_cases:
            if case[1] != model:
                continue
            a, b = PC.run_case(ctx, L, case), PC.run_case(ctx, L, case)
            assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), f"{case[0]}: two runs differ"
            results[case[0]] = a
            print(f"{case[0]:28s} evaluations {int(a[40])} iterations {int(a[39])} code {int(a[42])} matches {int(a[43])} final cost {a[7]!r}")
    ctx.close()
    out = {
        "commit": np.array(args.commit),
        "names": np.array([c[0] for c in all_cases]),
        "rings": np.array([c[1] for c in all_cases], np.int32),
        "two_d": np.array([int(c[2]) for c in all_cases], np.int32),
        "w0": np.stack([c[3] for c in all_cases]),
        "max_iter": np.array([c[4] for c in all_cases], np.int32),
        "min_matches": np.array([c[5] for c in all_cases], np.int64),
        "give_up_block": np.array([c[6] for c in all_cases], np.int32),
        "result": np.stack([results[c[0]] for c in all_cases]),
    }
    np.savez_compressed(args.out, **out)
    print(f"wrote {args.out}: {len(all_cases)} cases from {args.commit}, library {L._native.LIB_PATH}")


if __name__ == "__main__":
    main()
