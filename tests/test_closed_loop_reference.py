"""closed_loop_reference.closed_loop with no option set is integrator_oracle.closed_loop, bit for bit: the one tie between the
loop the CPU feature tests run their scenes through and the loop the GPU tests compare the device with."""
import numpy as np
import pytest

import populations
from closed_loop_reference import closed_loop
from oracle import integrator_oracle as io

N, STEPS = 65, 5


def _pattern(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


@pytest.mark.parametrize("coeff", ["f32", "f16"])
@pytest.mark.parametrize("implicit", [False, True], ids=["explicit", "implicit"])
def test_without_options_it_is_the_integrator_oracles_loop(implicit, coeff):
    state, prev, params = populations.integrator_population(N)
    rho, g, dt = populations.RHO, populations.G, populations.DT
    want = io.closed_loop(state, prev, params, rho, g, dt, STEPS, implicit=implicit, coeff_dtype=coeff)
    got = closed_loop(state, prev, params, rho, g, dt, STEPS, implicit=implicit, coeff_dtype=coeff)
    assert len(got) == len(want) == STEPS
    for r, w in zip(got, want):
        assert set(r) == {"input", "state", "wrench", "hydro", "k"}
        for key in ("input", "state", "wrench"):
            assert r[key].dtype == w[key].dtype == np.float32 and np.array_equal(_pattern(r[key]), _pattern(w[key])), key
        assert (r["k"] is None) == (w["k"] is None) == (not implicit)
        if implicit:
            for a, b in zip(r["k"], w["k"]):
                assert a.dtype == b.dtype == np.float64 and np.array_equal(_pattern(a), _pattern(b))
    assert not np.array_equal(got[-1]["state"], got[0]["input"])    # and the bodies moved
