#!/usr/bin/env python3
"""Generate tests/golden/runtime_calls_golden.json: what every batch wrapper of roman_amd.runtime.Context hands to the C ABI and
makes of what comes back, for the cases of tests/_runtime_calls.py, through the recording library of that module (no GPU, no
libroman_hip.so).  The file pins the behaviour of the roman_amd/runtime.py it is generated WITH, so it is generated with the
runtime.py of the commit a change to the wrappers starts from — before that file is touched, or with --runtime pointing at
that commit's copy of it — and never with the changed one.  Re-run with:

    python tests/golden/make_runtime_calls_golden.py --source "<commit the runtime.py is from>" [--runtime path/to/runtime.py]
"""
import argparse
import importlib.util
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--source", required=True, help="the commit whose roman_amd/runtime.py this run uses (stored in the file)")
    ap.add_argument("--runtime", default=None, help="that commit's runtime.py, when the tree's own has already changed")
    ap.add_argument("--out", default=os.path.join(HERE, "runtime_calls_golden.json"))
    args = ap.parse_args()
    if args.runtime:                                               # the given file takes the place of roman_amd.runtime
        import roman_amd
        spec = importlib.util.spec_from_file_location("roman_amd.runtime", args.runtime)
        mod = importlib.util.module_from_spec(spec)
        sys.modules["roman_amd.runtime"] = mod
        spec.loader.exec_module(mod)
        roman_amd.runtime = mod
    import _runtime_calls as rc
    from roman_amd import _abi
    _abi._LIB = rc.CallRecorder()
    out = {"generated_from": args.source}
    out.update(rc.run_all())
    with open(args.out, "w") as f:
        json.dump(out, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print(f"{os.path.relpath(args.out, ROOT)} written: {len(out['cases'])} cases, {os.path.getsize(args.out)} bytes")


if __name__ == "__main__":
    main()
