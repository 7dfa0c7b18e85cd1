"""Record what wrsn_entity_pointer_act writes on the first eight rows of the sampled case of tests/test_entity_pointer.py, from the
CPU-emulated build of the tree this runs in:

    python tools/gen_entity_pointer_act_golden.py --out NEW_FILE.npz

The file holds recorded results only: per node count N in {70, 33, 257} the eight outputs (node, stored, action, action_f64, logp,
node_logp, charge_mean, charge_log_std) of a B = 8, M = 3 call with Gumbel noise and charge draws.  tests/test_entity_pointer_mask.py
compares a later tree's bytes against them, so the file is made ONCE, on the commit before a change that must leave the call alone
(the candidate mask of wrsn_set_entity_pointer_mask, off), and never regenerated on the changed tree: the tool has no default output and
refuses to write over an existing file (the committed fixture is tests/golden/entity_pointer_act/case1.npz)."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "emu")]

ROWS = 8


def golden_call(side, N):
    """The call whose bytes are recorded: rows 0 .. 7 of test_entity_pointer.case(N) (M = 3, sampled)."""
    import entity_pointer_ref as P
    import test_entity_pointer as T
    ids, g, eps, node, mc, env, _ = T.case(N)
    return P.Call(side, T.M1, node[:ROWS], mc[:ROWS], env[:ROWS], ids[:ROWS], g[:ROWS], eps[:ROWS])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    if os.path.exists(a.out):
        raise SystemExit("%s exists: a recorded fixture is never regenerated (write to a new file and compare)" % a.out)
    import entity_pointer_ref as P
    import test_entity_pointer as T
    from sides import EmuSide
    out = {}
    for N in (70, 33, 257):
        side = T.make_side(EmuSide, N, ROWS, T.M1)
        got = golden_call(side, N).run()
        for k in P.OUTS:
            out["n%d_%s" % (N, k)] = got[k].copy()
        side.close()
    np.savez_compressed(a.out, **out)
    print("wrote", a.out, os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()
