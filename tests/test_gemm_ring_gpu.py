"""GPU: the bf16 x bf16 instances of gemm_bf16_fast give, with their register ring, the bits the library gave when it
fetched one tile (K tile 32) or two (K tile 64) ahead -- tests/golden/gemm_ring_bits.npz, recorded with the library of
the commit before the ring by tests/golden/make_gemm_ring_golden.py.  tests/gemm_ring.py has the cases and why they
are these; every call first asserts the plan it is meant for, writes C inside a sentinel-filled buffer, and is made
twice where it is split over K.
"""
import pytest

pytestmark = pytest.mark.gpu

import gemm_ring as ring  # noqa: E402
from helpers import load_golden  # noqa: E402


@pytest.fixture(scope="module")
def golden():
    return load_golden(ring.GOLDEN_FILE)


@pytest.mark.parametrize("c", ring.CASES, ids=[c.name for c in ring.CASES])
def test_ring_keeps_the_recorded_bits(c, golden):
    out, fails = ring.run(c)
    bad = ring.mismatch(c.name, out, golden)
    if bad:
        fails.append(bad)
    assert not fails, "\n".join(fails)
