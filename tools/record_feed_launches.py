#!/usr/bin/env python3
"""Record tests/golden/feed_launches.json: the sha256 of the output bytes of every call of tests/feed_cases.py, on an MI355X.

tests/test_gpu_feed_launches.py holds the file feeds and si_patch_rate to these digests, so record them only at a commit whose outputs
are the ones to keep -- the float64 references of the other feed tests say which those are.  Every call runs twice; digests that do not
repeat are an error and nothing is written.

usage: python tools/record_feed_launches.py [--out tests/golden/feed_launches.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "feed_launches.json"))
    args = ap.parse_args()
    import torch
    from tests import feed_cases as FC
    eng = FC.engine()
    runs = []
    for _ in range(2):
        digests = {}
        for name, make in sorted(FC.groups().items()):
            for key, call, _ in make(eng):
                outs = call()
                torch.cuda.synchronize()
                digests[key] = FC.digest(*outs)
        runs.append(digests)
    differ = [k for k in runs[0] if runs[0][k] != runs[1][k]]
    if differ:
        sys.exit(f"{len(differ)} of {len(runs[0])} digests do not repeat: {differ[:4]}")
    with open(args.out, "w") as f:
        json.dump(runs[0], f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(runs[0])} digests -> {args.out}")


if __name__ == "__main__":
    main()
