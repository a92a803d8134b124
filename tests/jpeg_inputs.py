"""The JPEG encoder's input list (seeded): what tests/test_jpeg_reference.py holds the NumPy
restatement to, byte for byte against the files libjpeg wrote (tests/golden/jpeg/), and what
tests/test_gpu_jpeg.py holds the GPU encoder to against the restatement.

A case is an image; every case is encoded at every quality of QUALITIES.  Gray (H, W) and colour
(H, W, 3 in B, G, R) at every size, with every content at every size but "stuffed", whose seeds
were searched for the two sizes that have room for it."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg")

QUALITIES = (95, 100, 50, 1)   # (1: the 255 clamp of the quantisation tables)

# (width, height): one block and less; pixel padding; 17 x 17 = padding and dummy blocks both ways;
# 65 x 8 = 9 blocks, one more than the 8 a wave of the block kernel holds; several MCU rows
SIZES = [(1, 1), (7, 9), (8, 8), (9, 8), (16, 16), (17, 17), (33, 15), (65, 8), (129, 47), (513, 24)]
# "stuffed" too: a size with dummy blocks, and one whose scan is longer than a stuffing chunk
CONTENT_SIZES = [(17, 17), (129, 47)]
CONTENTS = ["zero", "full", "mid", "noise", "ramp", "checker", "lone_hf", "stuffed"]

# The scan of the GPU encoder's bit counts sums 256 blocks per workgroup and then walks the
# workgroups' sums 64 at a time: 1032 x 1024 gray is 16 512 blocks = 64.5 workgroups, so the walk
# takes a second step and carries.  Not a fixture (the file is ~1 MB).
LARGE_SIZE = (1032, 1024)

# the GPU stuffing pass: bytes per lane, bytes per workgroup
STUFF_LANE_BYTES = 16
STUFF_CHUNK_BYTES = 4096

# "stuffed": seeds found by search, so that at quality 100 the scan has two 0xFF bytes next to each
# other and a 0xFF as the last byte of a lane's 16 (and, where the scan is long enough, as the last
# byte of a workgroup's 4096); tests/test_jpeg_reference.py asserts that they still do
STUFFED_SEEDS = {(17, 17, 1): 2, (17, 17, 3): 14, (129, 47, 1): 71, (129, 47, 3): 110}


class Case(object):
    def __init__(self, content, width, height, channels):
        self.content, self.width, self.height, self.channels = content, width, height, channels
        self.name = "%s_%dx%d_%s" % (content, width, height, "gray" if channels == 1 else "bgr")

    def __repr__(self):
        return self.name

    def image(self):
        return make_image(self.content, self.width, self.height, self.channels)


def _seed(content, w, h, ch):
    return [CONTENTS.index(content), w, h, ch]


def stuffed_image(w, h, ch, seed):
    """pixels 0 or 255 at random: large coefficients everywhere, long codes and all-ones values"""
    rng = np.random.default_rng([7, w, h, ch, seed])
    return (rng.integers(0, 2, (h, w) if ch == 1 else (h, w, 3), dtype=np.uint8) * 255).astype(np.uint8)


def make_image(content, w, h, ch):
    shape = (h, w) if ch == 1 else (h, w, 3)
    y, x = np.mgrid[0:h, 0:w]
    if content in ("zero", "full", "mid"):
        return np.full(shape, {"zero": 0, "full": 255, "mid": 128}[content], np.uint8)
    if content == "noise":
        return np.random.default_rng(_seed(content, w, h, ch)).integers(0, 256, shape, dtype=np.uint8)
    if content == "ramp":
        g = (255 * (2 * x + y)) // max(2 * (w - 1) + (h - 1), 1)
        if ch == 1:
            return g.astype(np.uint8)
        return np.stack([g, 255 - g, (255 * y) // max(h - 1, 1)], axis=-1).astype(np.uint8)
    if content == "checker":
        # 8 x 8 blocks of 0 / 255: DC differences of +-2040 at quality 100, category 11
        g = (((x // 8) + (y // 8)) & 1) * 255
    elif content == "lone_hf":
        # mid gray plus the (7, 7) basis function: coefficient 63 alone, a zero run of 62
        c = np.cos((2 * np.arange(8) + 1) * 7 * np.pi / 16)
        g = np.rint(128 + 127 * c[y % 8] * c[x % 8]).astype(np.int64)
    elif content == "stuffed":
        return stuffed_image(w, h, ch, STUFFED_SEEDS[(w, h, ch)])
    else:
        raise ValueError(content)
    g = g.astype(np.uint8)
    return g if ch == 1 else np.stack([g, g, g], axis=-1)


def cases():
    out = []
    for (w, h) in SIZES:
        for ch in (1, 3):
            contents = CONTENTS if (w, h) in CONTENT_SIZES else [c for c in CONTENTS if c != "stuffed"]
            out += [Case(c, w, h, ch) for c in contents]
    return out


def large_case():
    return Case("noise", LARGE_SIZE[0], LARGE_SIZE[1], 1)


def golden_npz(case):
    return os.path.join(GOLDEN, case.name + ".npz")


def golden_jpg(case, quality):
    return os.path.join(GOLDEN, "%s_q%d.jpg" % (case.name, quality))
