"""The reference AS EXECUTED against the oracle and the kernel arithmetic, with the suite: 2 x 3 000
bodies in which every field is, with some probability, a special value - exact zeros, the model's thresholds (speeds of 1e-6
and 0.2), quantised and axis-aligned vectors, cube rotations, non-unit and zero quaternions, dimensions of 0 / 1e-7 / 3e-7 m,
p_z on exact ties (tests/tools/reference_fuzz.py).  CPU only.  The reference's outputs on the two populations are the
committed fixtures tests/golden/fuzz_<seed>.npz, which tests/golden/make_golden.py writes by executing the reference; each
carries a digest of the population it was made from.  3 000 bodies per seed keeps them small and still holds every count
asserted below (round 4 ran 2 x 20 000 against the reference directly: tests/tools/reference_fuzz.py still does, for any size).

What is asserted is the classification the tool used to print:
  * oracle == reference: the nine outputs and the ratio to 1e-9 of the body's scale on every body, the behaviour-level net
    wrench (hydrodynamics_behavior.py:194-226 executed) to the same metric as the gate;
  * kernel arithmetic (host instantiation of csrc/hydro_body.h) vs reference: inside the 1e-5 gate for EVERY body whose
    smallest dimension is >= 1e-6 m; centres within half an fp32 ulp, the acceleration-independent components to 1e-6;
  * bodies thinner than that (plates of 0 / 1e-7 / 3e-7 m: not a reachable configuration) may exceed the gate against the
    reference as it stands - the reference forms WORLD-space centres and subtracts the position again
    (hydrodynamics_behavior.py:212-214), which at |p_xy| ~ 50 m costs 1e-14 m of a 1e-7 m lever arm whose torque is a
    300-fold cancellation - but EVERY one of them is inside the gate against the reference re-run at p_x = p_y = 0 (the
    wrench does not depend on them: numba_hydrodynamics.py:54-105 only ever uses z).
"""
import os
import sys

import pytest

from conftest import REPO


@pytest.fixture(scope="module")
def fuzz(native_built):
    sys.path.insert(0, os.path.join(REPO, "tests", "tools"))
    import reference_fuzz
    return reference_fuzz


@pytest.mark.parametrize("seed", [20251, 20252])
def test_reference_as_executed_on_special_value_populations(fuzz, seed):
    r = fuzz.run(3000, seed)
    assert r["reference_source"] == "fixture", r                      # the committed outputs of the reference, never a re-run
    assert r["reference_finite"] > 0.8 * r["n"] and r["rest_completed"] > 0 and r["dry"] > 500 and r["full"] > 500, r
    assert r["tiny_bodies"] > 1000                                    # the thin plates are in the population
    # oracle == reference
    assert r["oracle_components_over_1e-9"] == 0 and r["oracle_components_max"] <= 1e-9, r
    assert r["oracle_wrench_max"] <= 1e-5, r                          # (the oracle restates the reference's order of operations: it shares its spread on the thin plates)
    # kernel arithmetic vs reference, ordinary bodies: the gate, no allowance
    assert r["kernel_wrench_over_gate_ordinary_bodies"] == 0 and r["kernel_wrench_max_ordinary_bodies"] <= 5e-7, r
    # thin plates: against the reference at p_x = p_y = 0, all of them
    assert r["tiny_over_gate_at_pxy0"] == 0 and r["tiny_max_at_pxy0"] <= 1e-6, r
    assert r["kernel_wrench_over_gate"] <= 0.002 * r["n"]             # as it stands: a handful (6 / 30 000, 10 / 60 000 in round 4)
    # components
    assert r["centres_outside_half_ulp"] == 0 and r["components_beyond_1e-6"] == 0 and r["ratio_max_diff"] <= 6e-8, r
