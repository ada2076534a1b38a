#!/usr/bin/env python3
"""The surface of the reference's get_evalnet_miou_v2, read out of its evalnet.py (names and values only; nothing is copied).

Run where a checkout of the reference is on disk:

    IMK_REFERENCE=/path/to/InconsistencyMasks python tests/golden/make_golden_evalnet_v2.py

Writes tests/golden/reference_surface_evalnet_v2.json: the argument names and defaults of the three constructors of evalnet.py and the
names that module defines, which tests/test_cpu_evalnet_v2.py holds the package and the repo-root shim to."""
import ast
import json
import os
import sys

OUT = os.path.dirname(os.path.abspath(__file__))


def main():
    ref = os.environ.get("IMK_REFERENCE")
    if not ref or not os.path.isfile(os.path.join(ref, "evalnet.py")):
        sys.exit("set IMK_REFERENCE to a checkout of the reference")
    tree = ast.parse(open(os.path.join(ref, "evalnet.py")).read())
    sig = {}
    for node in tree.body:
        if isinstance(node, ast.FunctionDef):
            a = node.args
            defaults = [None] * (len(a.args) - len(a.defaults)) + [repr(ast.literal_eval(d)) for d in a.defaults]
            sig[node.name] = [[arg.arg, d] for arg, d in zip(a.args, defaults)]
    rec = {"module": "evalnet.py", "functions": sorted(sig), "signatures": {k: sig[k] for k in sorted(sig) if k.startswith("get_evalnet")}}
    with open(os.path.join(OUT, "reference_surface_evalnet_v2.json"), "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
