"""Record what the single-group node-pointer calls write on two cases of tests/test_entity_pointer_update.py, from the CPU-emulated build
of the tree this runs in:

    python tools/gen_entity_pointer_grad_golden.py --out NEW_FILE.npz

The file holds recorded results only: per case (n, N, M) in {(8, 33, 3), (2, 257, 3)} the two gradient buffers and the statistics row of
wrsn_entity_pointer_ppo_grad and the six outputs of wrsn_entity_pointer_eval (logp, entropy, node_logp, charge_mean, charge_log_std,
value).  tests/test_entity_pointer_joint.py compares a later tree's bytes against them, so the file is made ONCE, on the commit before a
change that must leave the single-group calls' bytes alone, and never regenerated on the changed tree: the tool has no default output and
refuses to write over an existing file (the committed fixture is tests/golden/entity_pointer_grad/case1.npz)."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "emu")]

CASES = ((8, 33, 3), (2, 257, 3))
EVAL_OUTS = ("logp", "entropy", "node_logp", "charge_mean", "charge_log_std", "value")


def record(Side):
    """{key: array} of the single-group calls on CASES through `Side` (the generator and the comparing test share this)."""
    import entity_pointer_train_ref as Q
    import test_entity_pointer_update as U
    out = {}
    for shape in CASES:
        n, N, M = shape
        nets, rows, batch, _ = U.grad_case(shape)
        side = U.side_for(Side, N, M)
        job = Q.Job(side, nets, rows, batch, N, M)
        ga, gc, stats = job.grad()
        fwd = job.eval()
        tag = "n%d_N%d_M%d_" % shape
        out[tag + "grad_actor"], out[tag + "grad_critic"], out[tag + "stats"] = ga.copy(), gc.copy(), stats.copy()
        for k in EVAL_OUTS:
            out[tag + k] = fwd[k].copy()
        side.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    if os.path.exists(a.out):
        raise SystemExit("%s exists: a recorded fixture is never regenerated (write to a new file and compare)" % a.out)
    from sides import EmuSide
    np.savez_compressed(a.out, **record(EmuSide))
    print("wrote", a.out, os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()
