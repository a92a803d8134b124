"""The overview reduction's kernels (amhip_tiff_overview.hip) use no scratch memory, spill
nothing and take no LDS, from the compiler's remarks of the build, in the manner of
tests/test_tiff_encode_kernel_resources.py."""
import pytest

from test_kernel_resources import _kernels, _one

# As compiled for gfx950 when the pyramid first matched the reference's bytes (VGPRs; no LDS):
#   k_tovr_reduce<f32, layer>  14    <f32, raster>  14    <u8, layer>  12    <u8, raster>  5
#   k_tovr_reduce<rgb8, layer>  12   <rgb8, raster>  11
KERNELS = ["13k_tovr_reduceILi0ELb1E", "13k_tovr_reduceILi0ELb0E", "13k_tovr_reduceILi1ELb1E",
           "13k_tovr_reduceILi1ELb0E", "13k_tovr_reduceILi2ELb1E", "13k_tovr_reduceILi2ELb0E"]


@pytest.mark.parametrize("needle", KERNELS)
def test_tovr_kernels_use_no_scratch_spill_nothing_and_take_no_lds(needle):
    k = _one(_kernels(), needle)
    assert k["VGPRs Spill"] == 0 and k["SGPRs Spill"] == 0, k
    assert k["ScratchSize"] == 0, k
    assert k["LDS Size"] == 0, k
    assert k["VGPRs"] <= 32, k          # (a lane per pixel and four loads: nothing that needs more)


def test_every_new_kernel_is_listed():
    names = [k for k in _kernels() if "k_tovr_" in k]
    assert len(names) == len(KERNELS), sorted(names)
