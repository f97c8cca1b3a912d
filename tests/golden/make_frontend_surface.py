#!/usr/bin/env python3
"""Records tests/golden/frontend_surface.json: what `import lidarslam_amd as L` exposes.

Run ONCE with the package of the commit BEFORE a change that must leave the front end's surface alone:

    python tests/golden/make_frontend_surface.py --commit <commit>

Contents: `commit`, `names` (every public module-level name that is not an imported module such as `os`),`functions` (name -> inspect.signature string of every public
function) and `classes` (for Context, Slam, RollingGrid, DeviceGrid and Sensors: member name -> signature string, "property"
for a property).  tests/test_abi.py::test_frontend_surface_is_the_recorded_one holds the package to the record.  Needs no
library and no device: nothing is called.
"""
import argparse
import inspect
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

CLASSES = ["Context", "Slam", "RollingGrid", "DeviceGrid", "Sensors"]


def members(cls):
    """name -> signature string of everything the class itself defines (dunders other than __init__ by name only)"""
    out = {}
    for name, v in vars(cls).items():
        if name in ("__module__", "__doc__", "__dict__", "__weakref__", "__qualname__", "__firstlineno__", "__static_attributes__"):
            continue
        f = v.__func__ if isinstance(v, (staticmethod, classmethod)) else v
        if isinstance(v, property):
            out[name] = "property"
        elif callable(f):
            out[name] = type(v).__name__ + str(inspect.signature(f))
        else:
            out[name] = "attribute"
    return out


def surface(L):
    names = sorted(n for n, v in vars(L).items() if not n.startswith("_") and not inspect.ismodule(v))
    functions = {n: str(inspect.signature(getattr(L, n))) for n in names if inspect.isfunction(getattr(L, n))}
    return {"names": names, "functions": functions, "classes": {c: members(getattr(L, c)) for c in CLASSES}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="the commit the package in use is of")
    ap.add_argument("--out", default=os.path.join(HERE, "frontend_surface.json"))
    args = ap.parse_args()
    import lidarslam_amd as L

    rec = {"commit": args.commit, **surface(L)}
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {args.out}: {len(rec['names'])} names, {len(rec['functions'])} functions, {sum(len(m) for m in rec['classes'].values())} class members")


if __name__ == "__main__":
    main()
