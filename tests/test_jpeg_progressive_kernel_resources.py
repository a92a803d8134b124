"""The progressive entropy kernel (k_jpegd_entropy_prog, amhip_jpeg_decode.hip) uses no scratch
memory and spills nothing, from the compiler's remarks of the build, in the manner of
tests/test_jpeg_decode_kernel_resources.py; and the kernels beside it still do not."""
import pytest

from test_kernel_resources import _kernels, _one

# As compiled for gfx950 when the kernel first matched libjpeg's pixels:
#   k_jpegd_entropy_prog  60 VGPRs, 106 SGPRs (none spilled), 7 waves per SIMD, 3920 bytes of LDS: three
#                         Huffman tables of 908 bytes, 1 KB of file bytes, the scan being walked (80
#                         bytes) and the frame's geometry (88 bytes).  The block itself lies in registers.
#   k_jpegd_entropy       as before: 50 VGPRs, no spill, 8 waves per SIMD, 4784 bytes of LDS
PROG = "20k_jpegd_entropy_progE"


def test_the_progressive_entropy_kernel_uses_no_scratch_and_spills_nothing():
    k = _one(_kernels(), PROG)
    assert k["VGPRs Spill"] == 0 and k["SGPRs Spill"] == 0, k
    assert k["ScratchSize"] == 0, k
    assert k["Occupancy"] >= 4, k       # (one wave per frame: the walk is not bound by occupancy)


def test_the_progressive_entropy_kernel_keeps_tables_window_and_scan_in_lds():
    k = _one(_kernels(), PROG)
    # three tables of 908 bytes + 1024 file bytes + the scan and the geometry, and no more than that
    assert 3 * 908 + 1024 <= k["LDS Size"] <= 3 * 908 + 1024 + 256, k


@pytest.mark.parametrize("needle", ["15k_jpegd_entropyE", "12k_jpegd_idctE", "14k_jpegd_colourE"])
def test_the_kernels_beside_it_are_found_alone_and_spill_nothing(needle):
    """the new kernel's name does not hide the baseline kernel from its own test"""
    k = _one(_kernels(), needle)
    assert k["VGPRs Spill"] == 0 and k["SGPRs Spill"] == 0 and k["ScratchSize"] == 0, k
