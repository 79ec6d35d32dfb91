#!/usr/bin/env python3
"""Records tests/golden/arena_footprints.json: the device bytes every job of tests/arena_footprint_worker.py holds on the host emulation, once with RBT_ARENA_SHARE=0 and
once with =1. tests/test_arena_footprint.py holds every later build against these figures, so run this on the commit whose layout is the one to keep (the parent of a change
that is meant to leave the layout alone), never to make a failing test pass.

Run:  python3 tests/golden/make_arena_footprints.py
"""
import json, os, sys
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import arena_footprint_cases as T


def main():
    T.build_hostemu()
    rec = {"share_" + s: T.run(s) for s in ("0", "1")}
    with open(T.GOLDEN, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True); f.write("\n")
    print(json.dumps(rec, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
