"""The GeoTIFF encoder's kernels (amhip_tiff_encode.hip) use no scratch memory and spill nothing, and
the producer's LDS stays within the stage DESIGN 4.16 states, from the compiler's remarks of the
build, in the manner of tests/test_png_encode_kernel_resources.py."""
import pytest

from test_kernel_resources import _kernels, _one

# As compiled for gfx950 when the encoder first matched zlib's bytes (VGPRs, LDS):
#   k_tiff_tile<f32, layer|raster>  45, 12.0 KB    k_tiff_tile<u8, ..>  37, 12.0 KB
#   k_tiff_tile<rgb8, ..>  36, 12.0 KB             k_tiff_offsets  12        k_tiff_gather  10
KERNELS = ["11k_tiff_tileILi0ELb1E", "11k_tiff_tileILi0ELb0E", "11k_tiff_tileILi1ELb1E", "11k_tiff_tileILi1ELb0E",
           "11k_tiff_tileILi2ELb1E", "11k_tiff_tileILi2ELb0E", "14k_tiff_offsetsE", "13k_tiff_gatherE"]


@pytest.mark.parametrize("needle", KERNELS)
def test_tiff_encode_kernels_use_no_scratch_and_spill_nothing(needle):
    k = _one(_kernels(), needle)
    assert k["VGPRs Spill"] == 0 and k["SGPRs Spill"] == 0, k
    assert k["ScratchSize"] == 0, k


def test_every_new_kernel_is_listed():
    names = [k for k in _kernels() if "k_tiff_" in k]
    assert len(names) == len(KERNELS), sorted(names)


@pytest.mark.parametrize("needle", KERNELS[:6])
def test_the_producer_keeps_its_stage_in_lds_within_the_stated_bound(needle):
    k = _one(_kernels(), needle)
    # the sample rows a piece of 4096 bytes can touch (12288 bytes) and three words
    assert 12288 <= k["LDS Size"] <= 12288 + 64, k
