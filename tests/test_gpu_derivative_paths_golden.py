"""The spatial-gradient and the Hessian decode against what they gave at the commit before both were put on one walk, one host driver
and shared device helpers: tests/golden/derivative_paths.npz, recorded once on an MI355X (tests/golden/make_golden_derivative_paths.py
has the list of calls).  It adds to test_gpu_decode_paths_golden.py what that pin leaves out: every Hessian entry and mode, the `chunk`
argument, the SIREN methods themselves and a net of two coordinates.  The kernels are deterministic and the comparison is exact."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def made():
    spec = importlib.util.spec_from_file_location("make_golden_derivative_paths", os.path.join(GOLDEN, "make_golden_derivative_paths.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    return mg, mg.run_all()


def test_every_derivative_path_gives_the_recorded_bits(made, golden):
    mg, calls = made
    want = golden("derivative_paths")
    assert sorted(calls) == sorted(want)
    for name in sorted(want):
        got, ref = calls[name], want[name]
        assert got.dtype == ref.dtype and got.shape == ref.shape, name
        assert np.array_equal(got, ref, equal_nan=ref.dtype.kind == "f"), name
        assert (ref.size == 0) == (name in mg.NONE_BY_CONTRACT), name


def test_the_chunk_loop_changes_no_bit(made):
    _, calls = made
    assert np.array_equal(calls["single_hessian_chunk"], calls["single_hessian_components"])
    assert np.array_equal(calls["single_gradient_chunk"], calls["single_gradient_whole"])
