"""What "the device's records equal the oracle's" means, shared by the GPU parity tests (test_gpu_parity.py,
test_gpu_frame_layouts.py)."""
import numpy as np

REL_TOL_ENERGY = 1e-5      # BASELINE.json north_star: "within 1e-5 relative for the float residual energy"


def compare(gpu_out, ora_out, K):
    counts, choices, energy, swept = gpu_out
    ocounts, odelta, ocoef, oenergy, oswept = ora_out
    assert (counts == ocounts).all(), f"{(counts != ocounts).sum()} count mismatches"
    # records 0..count inclusive (terminating record) are defined; compare them all
    idx = np.arange(K)[None, None, :]
    valid = idx <= np.minimum(ocounts[:, :, None], K - 1)
    assert (choices["deltaId"][valid] == odelta[valid]).all()
    assert (choices["intCoeff"][valid] == ocoef[valid]).all()
    assert (swept == oswept).all()
    assert np.allclose(energy, oenergy, rtol=REL_TOL_ENERGY, atol=0.0)
    assert (energy.view(np.uint64) == oenergy.view(np.uint64)).all(), "energy not bit-identical"
