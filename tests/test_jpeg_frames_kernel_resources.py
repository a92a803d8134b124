"""The register / occupancy budgets of the batched JPEG encoder's kernels (the k_jpegf_* of
amhip_jpeg.hip), from the compiler's remarks of the build, in the manner of
tests/test_jpeg_kernel_resources.py: each runs the body of a single-image kernel with the frame on a
second grid dimension and must keep that kernel's occupancy."""
import pytest

from test_kernel_resources import _kernels, _one

# (mangled-name fragment, waves per SIMD of the single-image kernel it corresponds to)
BUDGETS = [("14k_jpegf_blocksILi0E", 8), ("14k_jpegf_blocksILi1E", 8),   # k_jpeg_blocks<0|1>
           ("15k_jpegf_lengthsE", 8),                                     # k_jpeg_lengths
           ("12k_jpegf_scanE", 8),                                        # k_jpeg_scan_top
           ("12k_jpegf_packE", 8),                                        # k_jpeg_pack
           ("16k_jpegf_ff_countE", 8),                                    # k_jpeg_ff_count
           ("15k_jpegf_offsetsE", 8),                                     # (one wave, as k_jpeg_scan_top)
           ("13k_jpegf_stuffE", 8)]                                       # k_jpeg_stuff


@pytest.mark.parametrize("needle,min_waves", BUDGETS)
def test_jpeg_frames_kernels_budget(needle, min_waves):
    k = _one(_kernels(), needle)
    assert k["VGPRs Spill"] == 0 and k["SGPRs Spill"] == 0, k
    assert k["ScratchSize"] == 0, k
    assert k["Occupancy"] >= min_waves, k


def test_every_new_kernel_is_listed():
    """a k_jpegf_* kernel added later has to be given a budget here"""
    names = [k for k in _kernels() if "k_jpegf_" in k]
    assert len(names) == len(BUDGETS), sorted(names)
    # the stack never holds CV_16SC3: no third pixel mode
    assert not [k for k in names if "14k_jpegf_blocksILi2E" in k]


def test_the_block_kernel_keeps_its_lds_small_enough_for_eight_waves():
    ks = _kernels()
    for mode in range(2):
        assert _one(ks, "14k_jpegf_blocksILi%dE" % mode)["LDS Size"] <= 20 * 1024
