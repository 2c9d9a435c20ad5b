"""The decode attention entry points against the bits recorded in tests/golden/attn_bits.npz (tests/golden/make_attn_bits.py): the output and
the appended K / V rows of every case of tests/attn_bits_cases.py, bit for bit.  The float64 references of the other attention tests allow an
interval, which a changed summation order passes; this pins the arithmetic itself, so that moving or sharing kernel code cannot alter it
unnoticed.  A case whose inputs no longer hash to the recorded digest fails as such: the fixture is neither skipped nor re-recorded here."""
import os

import numpy as np
import pytest

from tests import attn_bits_cases as BC

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attn_bits.npz")


@pytest.fixture(scope="module")
def lib():
    from llamole_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def golden():
    with np.load(FIXTURE) as z:
        return {k: z[k] for k in z.files}


def test_the_fixture_holds_exactly_these_cases(golden):
    assert {k.split("/")[0] for k in golden if "/" in k} == set(BC.CASES)


@pytest.mark.parametrize("name", list(BC.CASES))
def test_bits_as_recorded(lib, golden, name):
    got = BC.run(lib, name)
    assert got["in"] == str(golden[name + "/in"]), f"{name}: the inputs of this case are not the ones the fixture was recorded on (input digest differs)"
    for what in ("out", "k", "v"):
        want = golden[f"{name}/{what}"]
        assert got[what].shape == want.shape, (name, what, got[what].shape, want.shape)
        assert np.array_equal(got[what], want), (name, what, int((got[what] != want).sum()), "elements differ from the recorded bits")
