"""Every public decode entry against what it gave at the commit before the artefact reader (brief_pytorch_amd/artefact.py) replaced
the per-mode copies of "open the artefact": tests/golden/decode_paths.npz, recorded once on an MI355X from the three stored artefacts
under tests/golden/decode_paths/ (tests/golden/make_golden_decode_paths.py has the artefacts and the list of calls).  The other GPU
tests compare one decode path with another of the same commit; this one pins the bits themselves.  The kernels are deterministic and
the comparison is exact: integers, float gradients and NaN depths alike."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def calls():
    spec = importlib.util.spec_from_file_location("make_golden_decode_paths", os.path.join(GOLDEN, "make_golden_decode_paths.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    return mg.run_all()


def test_every_decode_path_gives_the_recorded_bits(calls, golden):
    want = golden("decode_paths")
    assert sorted(calls) == sorted(want)
    assert any(np.isnan(want[k]).any() for k in want if want[k].dtype.kind == "f"), "no NaN depth in the recording: equal_nan tests nothing"
    for name in sorted(want):
        got, ref = calls[name], want[name]
        assert got.dtype == ref.dtype and got.shape == ref.shape, name
        assert np.array_equal(got, ref, equal_nan=ref.dtype.kind == "f"), name
