"""The GeoTIFF reader's own kernels (amhip_tiff_decode.hip) use no scratch memory, spill nothing and
need no LDS, as DESIGN 4.17 states, from the compiler's remarks of the build, in the manner of
tests/test_tiff_encode_kernel_resources.py.  (Its inflate step is the PNG decoder's kernel:
tests/test_png_decode_kernel_resources.py.)"""
import pytest

from test_kernel_resources import _kernels, _one

# As compiled for gfx950 when the reader first matched its reference (VGPRs):
#   k_tiffd_unpredict  44        k_tiffd_place  16
KERNELS = ["17k_tiffd_unpredictE", "13k_tiffd_placeE"]


@pytest.mark.parametrize("needle", KERNELS)
def test_tiff_decode_kernels_use_no_scratch_no_lds_and_spill_nothing(needle):
    k = _one(_kernels(), needle)
    assert k["VGPRs Spill"] == 0 and k["SGPRs Spill"] == 0, k
    assert k["ScratchSize"] == 0 and k["LDS Size"] == 0, k
    assert k["VGPRs"] <= 64, k          # (eight waves a SIMD: the row scans hide their loads behind other rows)


def test_every_new_kernel_is_listed():
    names = [k for k in _kernels() if "k_tiffd_" in k]
    assert len(names) == len(KERNELS), sorted(names)
