"""Every bit of the Winograd paths, both forms: the cases of tools/winograd_bits.py (each transform kernel through its C entry point
on geometries that take every branch of the index arithmetic, wgrad_finish with one and with five splits, and the whole operations
through ops) against tests/golden/g22_winograd_bits.npz, recorded from the commit before F(2x2,3x3) and F(4x4,3x3) became one
kernel family.  The accuracy tests next to this one would pass a changed operation order; this one does not.  A mismatch names the
result and means that an expression tree or a summation order moved: the code is wrong, not the fixture."""
import functools
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "g22_winograd_bits.npz"))


@functools.lru_cache(maxsize=None)
def _tool():
    spec = importlib.util.spec_from_file_location("winograd_bits", os.path.join(ROOT, "tools", "winograd_bits.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@functools.lru_cache(maxsize=None)
def _results():
    """All cases, run once and shared (read-only) by the tests."""
    return _tool().run_cases()


def test_the_run_produces_exactly_the_recorded_results():
    assert sorted(_results()) == sorted(GOLDEN.files)


@pytest.mark.parametrize("name", GOLDEN.files)
def test_bits_equal_the_recorded_ones(name):
    """Arrays: torch.equal on the int32 bit patterns.  Results of more than 16384 elements: equality of the SHA-256 of their bytes.
    The one refusal (F(2x2) weight gradient over 162 tiles): the error's text."""
    got, want = _results()[name], GOLDEN[name]
    if want.dtype.kind == "U":
        assert str(_tool().stored(got)) == str(want), name
    else:
        assert got.dtype == torch.int32 and torch.equal(got, torch.from_numpy(want)), name
