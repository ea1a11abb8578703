"""examples/explicit_impact.py at a reduced step count: the archive holds the ledger series, E* stays at its start value up
to rounding, the bar has yielded at the wall and not at its far end."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_explicit_impact_example(tmp_path):
    spec = importlib.util.spec_from_file_location("explicit_impact", os.path.join(ROOT, "examples", "explicit_impact.py"))
    example = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(example)
    out = os.path.join(str(tmp_path), "impact.npz")
    import _explicit_cases as ec
    steps, every = ec.EX_STEPS, ec.EX_EVERY
    solid = example.run(steps=steps, every=every, out=out)
    with np.load(out) as z:
        data = {k: z[k] for k in z.files}
    for k in example.LEDGER + ("time", "x", "x_dot", "x_ref", "accumulated_plastic_strain", "time_step_size"):
        assert k in data, k
    assert all(len(data[k]) == steps // every + 1 for k in example.LEDGER + ("time",))
    assert np.allclose(data["time"], np.arange(steps // every + 1) * every * float(data["time_step_size"]), rtol=1e-12)
    assert 0 < float(data["time_step_size"]) == solid.time_step_size
    # the bar hit the wall: kinetic energy went into internal work (elastic, plastic and the wall's penalty)
    assert data["KE"][-1] < 0.95 * data["KE"][0] and data["W_int"][-1] > 0.05 * data["KE"][0]
    assert np.all(data["W_ext"] == 0.0) and np.all(data["W_damp"] == 0.0)
    # E*: the bar of tests/test_explicit_gpu.py::test_e_star_is_conserved_over_200_steps -- 8 x the largest |E*_n - E*_0| of the
    # float64 restatement on this input (the oracle's bar, law and plane; tests/_explicit_cases.py), run at the example's own step
    import _explicit_cases as ec
    assert (example.LENGTH, example.GAP, example.PENALTY) == (ec.EX_LENGTH, ec.EX_GAP, ec.EX_PENALTY)
    assert solid.time_step_size == pytest.approx(ec.example_dt(), rel=1e-3)
    ref = ec.example_reference(float(solid.time_step_size), steps, every)
    drift = np.abs(data["E_star"] - data["E_star"][0]).max()
    print(f"E* drift {drift:.2e}; the restatement's {ref.drift:.2e} (bar {8 * ref.drift:.2e}), scale {data['KE'][0]:.3e}")
    for k in ("KE", "W_int"):
        assert abs(data[k][-1] - float(ref.series[-1][k])) <= 1e-6 * data["KE"][0], k          # the run is the restatement's
    assert drift <= 8.0 * ref.drift
    # plastic at the impact face, untouched at the far end (the elastic wave has not arrived)
    eqps, x_ref = data["accumulated_plastic_strain"], data["x_ref"]
    wall, far = x_ref[:, 0] == x_ref[:, 0].max(), x_ref[:, 0] == x_ref[:, 0].min()
    assert eqps[wall].min() > 0.0 and eqps[wall].max() > 1e-4
    assert np.all(eqps[far] == 0.0)
