"""The BDD100K protocol on HIP tensors: equal to the host path and to tests/golden/bdd100k_ref.npz, the reference's own numbers, with
``==`` (labels and counts exactly, floats with NaN equal to NaN), in index mode and in the "objects may overlap" mode."""
import functools

import numpy as np
import pytest
import torch

from sam_pt_amd import vos_metrics as VM
from tests import bdd100k_ref as B

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(B.GOLDEN) as z:
        return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def host_arrays():
    return B.our_arrays(B.dataset_of(golden()))


def test_device_equals_the_reference_and_the_host(dev):
    exp = {k: v for k, v in golden().items() if not k.startswith("in_") and k != "seed"}
    assert np.isfinite(exp["g_values"]).all() and set(exp["seq_label"].tolist()) == {"short", "medium", "long"}
    got = B.our_arrays(B.dataset_of(golden()), to=lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev))
    B.assert_same(got, exp)                                               # the reference's figures, tables and per-frame arrays
    B.assert_same(got, host_arrays())


def test_overlapping_tables_and_mixed_inputs(dev):
    data = B.dataset_of(golden())
    host, device = VM.BDD100KEval(object_overlapping_allowed=True), VM.BDD100KEval(object_overlapping_allowed=True)
    for name, (gt, _, planes) in data.items():
        host.add(name, planes, gt)
        device.add(name, torch.from_numpy(planes).to(dev), gt)            # the ground truth follows the prediction to the device
    (gh, th), (gd, td) = host.summarize(), device.summarize()
    assert list(gh) == list(VM.BDD100K_GLOBAL_NAMES) and th["Sequence"] == td["Sequence"]
    assert np.array_equal(np.array(list(gh.values())), np.array(list(gd.values())), equal_nan=True)
    for k in th:
        if k not in ("Sequence", "short-medium-long"):
            assert np.array_equal(np.array(th[k]), np.array(td[k]), equal_nan=True), k
    assert th["short-medium-long"] == td["short-medium-long"]


def test_refusals_on_the_device(dev):
    gt, pr, planes = B.dataset_of(golden())["b"]
    d = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)       # noqa: E731
    bad = gt.copy()
    bad[0, 0, 0] = 255
    with pytest.raises(ValueError, match="255"):
        VM.evaluate_bdd100k_sequence(d(pr), d(bad))
    hi = pr.copy()
    hi[0, 0, 0] = 3
    with pytest.raises(ValueError, match="index 3"):
        VM.evaluate_bdd100k_sequence(d(hi), d(gt))
    with pytest.raises(ValueError, match="object id 2 is never visible"):
        VM.evaluate_bdd100k_sequence(d(pr), d(np.where(gt == 2, 3, gt).astype(np.uint8)))
    with pytest.raises(ValueError, match="K \\+ 1"):
        VM.evaluate_bdd100k_sequence(d(planes[:, :2]), d(gt), object_overlapping_allowed=True)
