"""The PNG decoder's kernels (amhip_png_decode.hip) use no scratch memory and spill nothing, from
the compiler's remarks of the build, in the manner of tests/test_jpeg_decode_kernel_resources.py."""
import pytest

from test_kernel_resources import _kernels, _one

# As compiled for gfx950 when the decoder first matched zlib's scanlines and Pillow's pixels:
#   k_pngd_inflate   79 VGPRs, 105 SGPRs, 36.7 KB LDS (the 32 KiB window, 1 KB of stream, the tables)
#   k_pngd_unfilter  60 VGPRs
#   k_pngd_pixels    8 VGPRs
KERNELS = ["14k_pngd_inflateE", "15k_pngd_unfilterE", "13k_pngd_pixelsE"]


@pytest.mark.parametrize("needle", KERNELS)
def test_png_decode_kernels_use_no_scratch_and_spill_nothing(needle):
    k = _one(_kernels(), needle)
    assert k["VGPRs Spill"] == 0 and k["SGPRs Spill"] == 0, k
    assert k["ScratchSize"] == 0, k


def test_the_inflate_kernel_keeps_window_and_tables_in_lds():
    k = _one(_kernels(), "14k_pngd_inflateE")
    # the ring, 1 KB of stream, the two lookup tables (2 KB + 512 B); DESIGN 4.12 documents 40 KB as
    # the bound, which leaves room for four frames per CU
    assert 32768 + 1024 + 2048 + 512 <= k["LDS Size"] <= 40 * 1024, k
