"""The JPEG decoder's kernels (amhip_jpeg_decode.hip) use no scratch memory and spill nothing, from
the compiler's remarks of the build, in the manner of tests/test_jpeg_kernel_resources.py."""
import pytest

from test_kernel_resources import _kernels, _one

# As compiled for gfx950 when the decoder first matched libjpeg's pixels:
#   k_jpegd_entropy  42 VGPRs, 70 SGPRs, 4.7 KB LDS (four Huffman tables, 1 KB of file bytes, one block)
#   k_jpegd_idct     44 VGPRs, 9 KB LDS (32 blocks x 72 ints)
#   k_jpegd_colour   15 VGPRs
KERNELS = ["15k_jpegd_entropyE", "12k_jpegd_idctE", "14k_jpegd_colourE"]


@pytest.mark.parametrize("needle", KERNELS)
def test_jpeg_decode_kernels_use_no_scratch_and_spill_nothing(needle):
    k = _one(_kernels(), needle)
    assert k["VGPRs Spill"] == 0 and k["SGPRs Spill"] == 0, k
    assert k["ScratchSize"] == 0, k
    assert k["Occupancy"] >= 8, k


def test_the_entropy_kernel_keeps_a_frames_tables_in_lds():
    k = _one(_kernels(), "15k_jpegd_entropyE")
    # four tables of 908 bytes + 1024 file bytes + one block of int16
    assert 4 * 908 + 1024 + 128 <= k["LDS Size"] <= 8 * 1024, k
