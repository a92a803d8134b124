"""The register / occupancy budgets of the JPEG encoder's kernels (amhip_jpeg.hip), from the
compiler's remarks of the build, in the manner of tests/test_stereo_kernel_resources.py."""
import pytest

from test_kernel_resources import _kernels, _one

# As compiled for gfx950 when the encoder first matched libjpeg's bytes:
#   k_jpeg_blocks<0|1|2>  44 VGPRs, 13.3 KB LDS (32 blocks x (8 x 9 ints + 64 int16) + tables)
#   k_jpeg_lengths        47 VGPRs, 2.1 KB LDS (the four Huffman tables)
#   k_jpeg_pack           47 VGPRs, 2.1 KB LDS
#   k_jpeg_scan_top       20 VGPRs, one wave
#   k_jpeg_ff_count       17 VGPRs;   k_jpeg_stuff  20 VGPRs
# All are streaming kernels designed for the 8 waves per SIMD this target runs at the most: the
# block kernel's LDS allows 11 workgroups per CU, its registers (<= 64) all 8 waves.
BUDGETS = [("13k_jpeg_blocksILi0E", 8), ("13k_jpeg_blocksILi1E", 8), ("13k_jpeg_blocksILi2E", 8),
           ("14k_jpeg_lengthsE", 8), ("15k_jpeg_scan_topE", 8), ("11k_jpeg_packE", 8),
           ("15k_jpeg_ff_countE", 8), ("12k_jpeg_stuffE", 8)]


@pytest.mark.parametrize("needle,min_waves", BUDGETS)
def test_jpeg_kernels_budget(needle, min_waves):
    k = _one(_kernels(), needle)
    assert k["VGPRs Spill"] == 0 and k["SGPRs Spill"] == 0, k
    assert k["ScratchSize"] == 0, k
    assert k["Occupancy"] >= min_waves, k


def test_the_block_kernel_keeps_its_lds_small_enough_for_eight_waves():
    ks = _kernels()
    for mode in range(3):
        assert _one(ks, "13k_jpeg_blocksILi%dE" % mode)["LDS Size"] <= 160 * 1024 // 8
