"""Record what wrsn_entity_act writes on case 1 of tests/test_entity_act.py, from the CPU-emulated build of the tree this runs in:

    python tools/gen_entity_act_golden.py --out NEW_FILE.npz

The file holds recorded results only: per node count N in {70, 33, 257} the five outputs (action, action_f64, logp, mean, log_std) of the
B = 96, M = 3 call.  tests/test_entity_pointer.py compares a later tree's bytes against them, so the file is made ONCE, on the commit
before a change that must leave wrsn_entity_act alone, and never regenerated on the changed tree: the tool has no default output and
refuses to write over an existing file (the committed fixture is tests/golden/entity_act/case1.npz)."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "emu")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    if os.path.exists(a.out):
        raise SystemExit("%s exists: a recorded fixture is never regenerated (write to a new file and compare)" % a.out)
    import entity_act_ref as R
    import test_entity_act as T
    from sides import EmuSide
    out = {}
    for N in (70, 33, 257):
        side = T.make_side(EmuSide, N, T.B1, T.M1)
        call, _ = T.case1_call(side, N)
        got = call.run()
        for k in R.OUTS:
            out["n%d_%s" % (N, k)] = got[k].copy()
        side.close()
    np.savez_compressed(a.out, **out)
    print("wrote", a.out, os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()
