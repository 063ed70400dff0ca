"""Writes tests/golden/bdd100k_ref.npz: the seeded BDD100K data set of tests/bdd100k_ref.seeded_dataset (ground-truth and predicted
index maps, and the overlapping boolean planes as bits) and what the REFERENCE's own evaluator makes of it, run in place through
tests/bdd100k_ref.py: the 22 global figures and the per-object table of ``BDD100KEvaluator.evaluate()`` on the set written as indexed
PNGs, and the per-frame arrays and frame counts of ``_evaluate_semisupervised(mp_pool=False)`` per sequence, in index mode and in the
"objects may overlap" mode.  J, F and the statistics inside the reference are the project's own (the stand-in for the absent
``davis2017``): the file pins the protocol.  Nothing of sam_pt_amd's BDD100K code takes part.

Regenerate (needs the reference tree, SAMPT_REFERENCE or the default of oracle/reference_loader.py):

    python tools/make_bdd100k_golden.py [--seed 7]

The conditions the tests assert on the set are checked here first (tests/bdd100k_ref.check_conditions): every global figure finite,
all three length bins populated, an object on the border, one covering a whole frame, one that disappears and returns, a prediction
where the truth is invisible, a frame where both are empty, and an object that first appears on the last frame.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import bdd100k_ref as B  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--out", default=B.GOLDEN)
    args = ap.parse_args()
    assert B.available(), "the reference tree (and pandas, PIL, tqdm for it) is required"
    dataset = B.seeded_dataset(args.seed)
    ref = B.reference_arrays(dataset)
    B.check_conditions(dataset, ref)
    np.savez_compressed(args.out, seed=np.int64(args.seed), **B.input_arrays(dataset), **ref)
    print(f"{args.out}: {os.path.getsize(args.out)} bytes, {len(ref['seq_Sequence'])} objects in {len(dataset)} sequences, "
          f"global = {dict(zip(ref['g_names'].tolist(), np.round(ref['g_values'], 4).tolist()))}")


if __name__ == "__main__":
    main()
