"""The PNG encoder's kernels (amhip_png_encode.hip) use no scratch memory and spill nothing, and the
plan kernel's LDS stays within the bound DESIGN 4.15 states, from the compiler's remarks of the build,
in the manner of tests/test_png_decode_kernel_resources.py."""
import pytest

from test_kernel_resources import _kernels, _one

# As compiled for gfx950 when the encoder first matched zlib's bytes (VGPRs, LDS):
#   k_pnge_filter<0|1|2>  22        k_pnge_scan_runs  42, 2 KB     k_pnge_tokens<0>  31, 1 KB
#   k_pnge_scan_counts  20, 2 KB    k_pnge_tokens<1>  50, 1 KB     k_pnge_plan  21, 6.6 KB
#   k_pnge_offsets  19              k_pnge_pack  22, 1.8 KB        k_pnge_file_offsets  12
#   k_pnge_frame  10, 1 KB
KERNELS = ["13k_pnge_filterILi0E", "13k_pnge_filterILi1E", "13k_pnge_filterILi2E", "16k_pnge_scan_runsE",
           "13k_pnge_tokensILb0E", "13k_pnge_tokensILb1E", "18k_pnge_scan_countsE", "11k_pnge_planE",
           "14k_pnge_offsetsE", "11k_pnge_packE", "19k_pnge_file_offsetsE", "12k_pnge_frameE"]


@pytest.mark.parametrize("needle", KERNELS)
def test_png_encode_kernels_use_no_scratch_and_spill_nothing(needle):
    k = _one(_kernels(), needle)
    assert k["VGPRs Spill"] == 0 and k["SGPRs Spill"] == 0, k
    assert k["ScratchSize"] == 0, k


def test_every_new_kernel_is_listed():
    names = [k for k in _kernels() if "k_pnge_" in k]
    assert len(names) == len(KERNELS), sorted(names)


def test_the_plan_kernel_keeps_its_trees_in_lds_within_the_stated_bound():
    k = _one(_kernels(), "11k_pnge_planE")
    # the three trees with their heap (amhip_png_encode_host.h: Work, 5.5 KB) and the block's histogram
    # (287 words); DESIGN 4.15 states 8 KB as the bound, which leaves room for 20 blocks per CU
    assert 5500 + 287 * 4 <= k["LDS Size"] <= 8 * 1024, k
