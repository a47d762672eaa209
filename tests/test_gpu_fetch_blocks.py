"""The four fetches above a run -- afx_batch_fetch_high_level, _classification_features, _class_signature, _class_decision --
share one reused result block of the batch's workspace, each with a layout of its own (afec_amd/csrc/afx_block.h).  One
batch, one run, the fetches interleaved in two orders with partial high-level fetches in between: whatever lay in the
block before, every array of every repeat is the first one's, bit for bit; the decision's class signature is the signature
fetch's, and the features the models' kernel consumed are the ones the feature fetch hands out."""
import numpy as np
import pytest

import afec_amd as afx
from tests import _gbdt_ref as ref
from tests.test_gpu_class_signature import IDENTITY, generated, pcm

pytestmark = pytest.mark.gpu


def flat(result):
    """the arrays of one fetch, by name"""
    if isinstance(result, dict):
        return dict(result)
    return {str(i): a for i, a in enumerate(result)}


def same(got, want, what):
    got, want = flat(got), flat(want)
    assert got.keys() == want.keys(), what
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
        assert got[k].tobytes() == want[k].tobytes(), (what, k)


def test_interleaved_fetches_on_the_one_result_block():
    plan = afx.Plan()
    # no samples, one frame, three frames, 65 frames (past time position 44), a refused buffer (double PCM in a float batch)
    bufs = [np.zeros(0, dtype=np.float32), pcm(1, 1), pcm(3, 2), pcm(65, 3), pcm(3, 4).astype(np.float64)]
    batch = plan.batch(bufs, afx.D_CLASS_DECISION_INPUTS | afx.D_HIGH_LEVEL_INPUTS)
    cm = afx.Model(plan, [ref.write_lightgbm(generated(11 + s, 2, 10 + s)) for s in range(2)], *IDENTITY)
    gm = afx.Model(plan, [ref.write_lightgbm(generated(100 * s + 7, 7, 12 + s, spread=0.4)) for s in range(2)], *IDENTITY)
    try:
        batch.run()
        assert np.diff(batch.fetch()["frame_offset"]).tolist() == [0, 1, 3, 65, 0]
        fetches = {
            "high": lambda: batch.fetch_high_level(),
            "features": lambda: batch.fetch_classification_features(),
            "class": lambda: batch.fetch_class_signature(cm),
            "category": lambda: batch.fetch_class_signature(gm),
            "decision": lambda: batch.fetch_class_decision(class_model=cm, category_model=gm, category_none_class=3),
            "scalars": lambda: batch.fetch_high_level(want=("scalars",)),            # partial: a pointer of afx_high_out is NULL
            "pitch": lambda: batch.fetch_high_level(want=("pitch", "peak", "status")),
        }
        first = {name: fetch() for name, fetch in fetches.items()}
        orders = (["decision", "scalars", "high", "class", "features", "pitch", "category", "decision", "high", "features", "class"],
                  ["features", "high", "pitch", "decision", "category", "scalars", "class", "features", "decision", "high", "class"])
        for order in orders:
            for step, name in enumerate(order):
                same(fetches[name](), first[name], f"{name} at step {step} of {order}")
        same({k: first["high"][k] for k in ("scalars",)}, first["scalars"], "partial high-level fetch")
        same({k: first["high"][k] for k in ("pitch", "peak", "status")}, first["pitch"], "partial high-level fetch")

        features, bad, status = first["features"]
        assert status.tolist() == [0, 0, 0, 0, -6] and np.all(bad == 0)
        decision = first["decision"]
        assert decision["class_signature"].tobytes() == first["class"][0].tobytes()
        assert decision["category_signature"].tobytes() == first["category"][0].tobytes()
        # the features the models' kernel read in the block are the ones the feature fetch hands out: the same kernel on them
        # as the caller's vectors gives the same signature, for the buffers that have frames (a vector has no frame count)
        live = [1, 2, 3]
        for model, name in ((cm, "class"), (gm, "category")):
            sig, used, _ = model.evaluate_features(features[live])
            assert sig.tobytes() == first[name][0][live].tobytes() and used.tobytes() == first[name][1][live].tobytes(), name
        assert np.any(first["class"][0][live] != 0.0) and not np.any(first["class"][0][[0, 4]])
    finally:
        cm.close()
        gm.close()
        batch.close()
        plan.close()
