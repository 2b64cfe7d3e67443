#!/usr/bin/env python3
"""Record the argument traces of tests/args_trace.py's case table (what omgsr_amd.ops hands the library) as the expected values of
tests/test_args_trace_gpu.py. Run it on the MI355X against the omgsr_amd/ops.py the traces are to be held to - before a refactor of that
file, not after it: the output stores that file's git blob id (`git rev-parse HEAD:omgsr_amd/ops.py` of the commit it was taken from).

    python tools/record_args_trace.py [--out tests/golden/args_trace.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import args_trace as T
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=T.GOLDEN)
    out = ap.parse_args().out
    cases = {name: T.run_case(name) for name in T.CASES}
    # one case per line: recorded results only, and a diff of two recordings names the cases that moved
    lines = ",\n".join(f"  {json.dumps(name)}: {json.dumps(cases[name], sort_keys=True, separators=(',', ':'))}" for name in sorted(cases))
    with open(out, "w") as f:
        f.write('{\n "ops_blob": %s,\n "cases": {\n%s\n }\n}\n' % (json.dumps(T.blob_id(os.path.join(ROOT, "omgsr_amd", "ops.py"))), lines))
    print(f"{len(cases)} cases -> {out} ({os.path.getsize(out)} bytes)")


if __name__ == "__main__":
    main()
