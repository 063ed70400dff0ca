"""Writes tests/golden/interactive_ref.npz: what scikit-learn and the REFERENCE's own code make of the seeded cases of
tests/interactive_ref.py.

* ``dbscan_<case>``: ``sklearn.cluster.DBSCAN(eps, min_samples).fit(X).labels_`` as int16 (the points are regenerated from seeds, only
  the labels are stored).
* ``extract_<case>``: the (x, y) points of the reference's ``extract_largest_cluster_points`` run in place (k-medoids: the project's
  stand-in), same ``torch.manual_seed``.
* ``loop_<config>_*``: the interaction history (every field) and the final logits of the reference's ``SamPtInteractive.forward`` run
  in place in a temporary working directory over the oracle's CPU SAM (seeded weights) and a scripted tracker, for the offline, online
  and ``disable_point_tracking`` configurations and one with a refinement iteration.

Nothing of sam_pt_amd's DBSCAN, click selection or loop takes part.  Regenerate (needs scikit-learn and the reference tree,
SAMPT_REFERENCE or the default of oracle/reference_loader.py):

    python tools/make_interactive_golden.py

The tool refuses to write unless the offline and the online run each exercise all four actions at least once (remove negative, remove positive, add
positive, add negative) and every branch of the click selection is taken by the case named after it.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import interactive_ref as IR  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=IR.GOLDEN)
    args = ap.parse_args()
    assert IR.available() and IR.sklearn_available(), "scikit-learn and the reference tree (with PIL, tqdm for it) are required"
    out = {}
    for name, (X, eps, ms) in IR.dbscan_cases().items():
        labels = IR.sklearn_labels(X, eps, ms)
        assert labels.max() < 2 ** 15
        out[f"dbscan_{name}"] = labels.astype(np.int16)
    n_cl = {n: int(out[f"dbscan_{n}"].max()) + 1 for n in ("all_noise", "bridge", "n1000", "ref_18000")}
    assert n_cl["all_noise"] == 0 and n_cl["bridge"] == 2 and n_cl["n1000"] == 12 and n_cl["ref_18000"] == 2, n_cl
    for name, (mask, n, seed) in IR.extract_cases().items():
        out[f"extract_{name}"] = IR.reference_extract(mask, n, seed)
    missing = []
    for name in IR.LOOP_CONFIGS:
        rows, logits = IR.run_reference_loop(name)
        out.update(IR.history_arrays(f"loop_{name}", rows, logits))
        print(f"loop {name}: {len(rows)} interactions, actions {sorted(IR.actions_of(rows))}")
        if name in IR.ALL_FOUR:
            missing += [(name, a) for a in IR.ACTIONS if a not in IR.actions_of(rows)]
    if missing:
        raise SystemExit(f"refusing to write {args.out}: these runs never take these actions: {missing}")
    np.savez_compressed(args.out, **out)
    print(f"{args.out}: {os.path.getsize(args.out)} bytes; clusters {n_cl}")


if __name__ == "__main__":
    main()
