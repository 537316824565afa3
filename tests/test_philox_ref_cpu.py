"""tests/philox_ref.py against the three Random123 known-answer vectors of Philox4x32-10 (kat_vectors of the Random123
distribution; Salmon et al., SC'11), and its numpy form against its scalar form.  No GPU: the dropout kernel's own known-answer
test (test_gpu_dropout_philox.py) stands on this."""
import numpy as np
import pytest

import philox_ref as P

KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


@pytest.mark.parametrize("counter,key,want", KAT)
def test_known_answer_vectors(counter, key, want):
    assert P.philox4x32_10(counter, key) == want


def test_constants_are_the_published_ones():
    assert (P.M0, P.M1, P.W0, P.W1, P.ROUNDS) == (0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85, 10)


@pytest.mark.parametrize("seed,offset", [(0, 0), (0x9E3779B97F4A7C15, 0x100000004), (0xFFFFFFFFFFFFFFFF, 12)])
def test_vector_form_equals_scalar_form(seed, offset):
    n = 300
    got = P.first_words(n, seed, offset)
    want = [P.philox4x32_10((i, 0, offset & P.MASK, offset >> 32), (seed & P.MASK, seed >> 32))[0] for i in range(n)]
    assert got.dtype == np.int64 and got.tolist() == want
    assert P.uniform24(n, seed, offset).tolist() == [w >> 8 for w in want]


def test_vector_form_reproduces_the_first_known_answer():
    # counter (0, 0, 0, 0), key (0, 0) is plane 0 of (seed 0, offset 0)
    assert int(P.first_words(1, 0, 0)[0]) == 0x6627E8D5
