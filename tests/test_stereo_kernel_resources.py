"""The register / occupancy budgets of the stereo sequence's own kernels (the append-mode densify),
from the compiler's remarks of the build, in the manner of tests/test_kernel_resources.py."""
import pytest

from test_kernel_resources import _kernels, _one

# As compiled for gfx950 when the sequence tests first passed:
#   k_densify_append_scan   22 VGPRs, no scratch, 16 B LDS, 8 waves / SIMD
#   k_densify_append_emit   45 VGPRs, no scratch, 16 B LDS, 8 waves / SIMD
# (streaming kernels: 8 waves per SIMD is the most this target runs; the floor is that figure)
BUDGETS = [("21k_densify_append_scanE", 8), ("21k_densify_append_emitE", 8)]


@pytest.mark.parametrize("needle,min_waves", BUDGETS)
def test_append_kernels_budget(needle, min_waves):
    k = _one(_kernels(), needle)
    assert k["VGPRs Spill"] == 0 and k["SGPRs Spill"] == 0, k
    assert k["ScratchSize"] == 0, k
    assert k["Occupancy"] >= min_waves, k


def test_the_pair_densify_kernels_are_still_there():
    ks = _kernels()
    for needle in ("15k_densify_countE", "14k_densify_scanE", "14k_densify_emitE"):
        assert _one(ks, needle)["VGPRs Spill"] == 0
