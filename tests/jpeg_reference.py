"""NumPy restatement of the baseline JPEG file libjpeg writes at the settings the reference's
cv::imwrite / Pillow's Image.save(f, "JPEG", quality=q, subsampling=2, optimize=False) use:
sequential DCT, 8 bit, the standard Huffman tables, one scan, no restart markers; gray images as one
component (declared 2x2 like Pillow does, coded block by block), colour images as Y 2x2, Cb 1x1,
Cr 1x1 (4:2:0).

Every rule names the libjpeg function it restates (IJG libjpeg 6b / libjpeg-turbo file names).
Unlike the OpenCV restatements this one IS pinned: tests/golden/jpeg/ holds the files the real
library wrote for tests/jpeg_inputs.py, and tests/test_jpeg_reference.py compares byte for byte.
This module is the yardstick of the GPU encoder (aerial_mapper_amd/csrc/amhip_jpeg.hip).

Also a small baseline decoder (segments -> Huffman -> quantised coefficients per block -> float
IDCT -> pixels), so that a mismatch can be located by block and coefficient.

Integer arithmetic only on the encoding side (int64; >> on negative numbers is arithmetic, as
libjpeg's RIGHT_SHIFT).  Images are (H, W) uint8 or (H, W, 3) uint8 in OpenCV's B, G, R order.
"""
import numpy as np

# ---------------------------------------------------------------------------
# tables
# ---------------------------------------------------------------------------
# jpeg_natural_order (jutils.c): zigzag position -> natural (row-major) index
ZIGZAG = np.array([
    0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20,
    13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59,
    52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63], np.int64)

# std_luminance_quant_tbl / std_chrominance_quant_tbl (jcparam.c), natural order
STD_LUM_Q = np.array([
    16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
    14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113,
    92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99], np.int64)
STD_CHR_Q = np.array([
    17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
    47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32, np.int64)

# std_huff_tables (jcparam.c / jstdhuff.c): bits[1..16], values
DC_LUM_BITS = [0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]
DC_CHR_BITS = [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0]
DC_VALS = list(range(12))
AC_LUM_BITS = [0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d]
AC_LUM_VALS = [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07,
    0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0,
    0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28,
    0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49,
    0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
    0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
    0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7,
    0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5,
    0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
    0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8,
    0xf9, 0xfa]
AC_CHR_BITS = [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77]
AC_CHR_VALS = [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71,
    0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0,
    0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26,
    0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
    0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68,
    0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
    0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5,
    0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
    0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
    0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8,
    0xf9, 0xfa]
assert len(AC_LUM_VALS) == sum(AC_LUM_BITS) == 162 and len(AC_CHR_VALS) == sum(AC_CHR_BITS) == 162


def quant_tables(quality):
    """jpeg_set_quality(cinfo, quality, force_baseline=TRUE): jpeg_quality_scaling, then
    jpeg_add_quant_table's (base * scale + 50) / 100 clamped to 1..255.  -> (lum, chroma), natural
    order.  `clamped` counts are for the tests (how many entries hit 255)."""
    q = min(max(int(quality), 1), 100)
    scale = 5000 // q if q < 50 else 200 - 2 * q
    out = []
    for base in (STD_LUM_Q, STD_CHR_Q):
        t = (base * scale + 50) // 100
        out.append(np.clip(t, 1, 255))
    return out[0], out[1]


def quant_clamped_entries(quality):
    """entries of both tables the 255 clamp of force_baseline changed"""
    q = min(max(int(quality), 1), 100)
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return int(sum(((b * scale + 50) // 100 > 255).sum() for b in (STD_LUM_Q, STD_CHR_Q)))


def huff_codes(bits, vals):
    """jpeg_make_c_derived_tbl (jchuff.c): symbol -> (code, length); canonical codes by length."""
    code, k, out = 0, 0, {}
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


def _code_arrays(bits, vals, n):
    code = np.zeros(n, np.uint64)
    size = np.zeros(n, np.int64)
    for sym, (c, l) in huff_codes(bits, vals).items():
        code[sym], size[sym] = c, l
    return code, size


# [table 0 = luminance, 1 = chrominance]
DC_CODE = [_code_arrays(DC_LUM_BITS, DC_VALS, 12), _code_arrays(DC_CHR_BITS, DC_VALS, 12)]
AC_CODE = [_code_arrays(AC_LUM_BITS, AC_LUM_VALS, 256), _code_arrays(AC_CHR_BITS, AC_CHR_VALS, 256)]

# ---------------------------------------------------------------------------
# pixels -> component planes
# ---------------------------------------------------------------------------


def rgb_to_ycc(bgr):
    """rgb_ycc_convert (jccolor.c): 16-bit fixed point, FIX(x) = (int)(x * 65536 + 0.5); ONE_HALF is
    folded into the B tables, and the chroma tables carry CBCR_OFFSET + ONE_HALF - 1."""
    b = bgr[..., 0].astype(np.int64)
    g = bgr[..., 1].astype(np.int64)
    r = bgr[..., 2].astype(np.int64)
    half, off = 1 << 15, 128 << 16
    y = (19595 * r + 38470 * g + 7471 * b + half) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + off + half - 1) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + off + half - 1) >> 16
    return y, cb, cr


def _edge(plane, rows, cols):
    """expand_right_edge / expand_bottom_edge (jcsample.c, jcprepct.c): replicate the last column,
    then the last row"""
    h, w = plane.shape
    return np.pad(plane, ((0, rows - h), (0, cols - w)), mode="edge")


def h2v2_downsample(plane, out_rows, out_cols):
    """h2v2_downsample (jcsample.c) behind pre_process_data (jcprepct.c): the full-size plane is
    replicated to the right up to 2 * out_cols and down to an even number of rows; each output is
    (a + b + c + d + bias) >> 2 with bias 1, 2, 1, 2, ... along a row; the DOWNSAMPLED rows are
    then replicated down to out_rows."""
    h, w = plane.shape
    p = _edge(plane, h + (h & 1), 2 * out_cols)
    s = p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2]
    bias = 1 + (np.arange(out_cols, dtype=np.int64) & 1)
    d = (s + bias[None, :]) >> 2
    return _edge(d, out_rows, out_cols)


def to_blocks(plane):
    """(8 * R, 8 * C) -> (R, C, 8, 8)"""
    r, c = plane.shape[0] // 8, plane.shape[1] // 8
    return plane.reshape(r, 8, c, 8).transpose(0, 2, 1, 3)


# ---------------------------------------------------------------------------
# forward DCT + quantisation
# ---------------------------------------------------------------------------
CONST_BITS, PASS1_BITS = 13, 2
F_0_298, F_0_390, F_0_541, F_0_765, F_0_899, F_1_175 = 2446, 3196, 4433, 6270, 7373, 9633
F_1_501, F_1_847, F_1_961, F_2_053, F_2_562, F_3_072 = 12299, 15137, 16069, 16819, 20995, 25172


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _fdct_1d(d, first):
    """one pass of jpeg_fdct_islow (jfdctint.c) along the last axis"""
    t0, t7 = d[..., 0] + d[..., 7], d[..., 0] - d[..., 7]
    t1, t6 = d[..., 1] + d[..., 6], d[..., 1] - d[..., 6]
    t2, t5 = d[..., 2] + d[..., 5], d[..., 2] - d[..., 5]
    t3, t4 = d[..., 3] + d[..., 4], d[..., 3] - d[..., 4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    out = np.empty_like(d)
    n = CONST_BITS - PASS1_BITS if first else CONST_BITS + PASS1_BITS
    if first:
        out[..., 0] = (t10 + t11) << PASS1_BITS
        out[..., 4] = (t10 - t11) << PASS1_BITS
    else:
        out[..., 0] = _descale(t10 + t11, PASS1_BITS)
        out[..., 4] = _descale(t10 - t11, PASS1_BITS)
    z1 = (t12 + t13) * F_0_541
    out[..., 2] = _descale(z1 + t13 * F_0_765, n)
    out[..., 6] = _descale(z1 + t12 * (-F_1_847), n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * F_1_175
    t4, t5, t6, t7 = t4 * F_0_298, t5 * F_2_053, t6 * F_3_072, t7 * F_1_501
    z1, z2, z3, z4 = z1 * (-F_0_899), z2 * (-F_2_562), z3 * (-F_1_961), z4 * (-F_0_390)
    z3, z4 = z3 + z5, z4 + z5
    out[..., 7] = _descale(t4 + z1 + z3, n)
    out[..., 5] = _descale(t5 + z2 + z4, n)
    out[..., 3] = _descale(t6 + z2 + z3, n)
    out[..., 1] = _descale(t7 + z1 + z4, n)
    return out


def fdct_islow(blocks):
    """(..., 8, 8) samples -> coefficients scaled by 8: forward_DCT's level shift (jcdctmgr.c:
    sample - CENTERJSAMPLE), rows, then columns"""
    d = blocks.astype(np.int64) - 128
    d = _fdct_1d(d, True)
    d = _fdct_1d(d.swapaxes(-1, -2), False).swapaxes(-1, -2)
    return d


def quantise(coef, qtable):
    """forward_DCT (jcdctmgr.c): divisor = 8 * table entry; (|c| + q / 2) / q, sign restored.
    coef (..., 8, 8); -> (..., 64) in zigzag order"""
    q = (qtable.reshape(8, 8) * 8).astype(np.int64)
    a = (np.abs(coef) + (q >> 1)) // q
    v = np.where(coef < 0, -a, a)
    return v.reshape(v.shape[:-2] + (64,))[..., ZIGZAG]


# ---------------------------------------------------------------------------
# the scan's blocks
# ---------------------------------------------------------------------------


def component_planes(image):
    """the samples the DCT sees: [(plane padded to whole blocks of the component's own grid, quant
    table index)], Y (or gray) first"""
    image = np.asarray(image)
    h, w = image.shape[:2]
    bh, bw = (h + 7) // 8, (w + 7) // 8
    if image.ndim == 2:
        return [(_edge(image.astype(np.int64), 8 * bh, 8 * bw), 0)]
    y, cb, cr = rgb_to_ycc(image)
    my, mx = (h + 15) // 16, (w + 15) // 16
    return [(_edge(y, 8 * bh, 8 * bw), 0), (h2v2_downsample(cb, 8 * my, 8 * mx), 1),
            (h2v2_downsample(cr, 8 * my, 8 * mx), 1)]


class Blocks(object):
    """coef (N, 64) quantised coefficients, zigzag order, in the order the scan codes them;
    comp (N,) component (0 Y / gray, 1 Cb, 2 Cr); dummy (N,) blocks that only fill the last MCU
    column / row."""

    def __init__(self, coef, comp, dummy):
        self.coef, self.comp, self.dummy = coef, comp, dummy


def blocks_of(image, quality):
    image = np.asarray(image)
    assert image.dtype == np.uint8 and image.ndim in (2, 3)
    qlum, qchr = quant_tables(quality)
    h, w = image.shape[:2]
    if image.ndim == 2:
        bh, bw = (h + 7) // 8, (w + 7) // 8
        y = _edge(image.astype(np.int64), 8 * bh, 8 * bw)
        coef = quantise(fdct_islow(to_blocks(y)), qlum).reshape(-1, 64)
        n = coef.shape[0]
        return Blocks(coef, np.zeros(n, np.int64), np.zeros(n, bool))
    assert image.shape[2] == 3
    y, cb, cr = rgb_to_ycc(image)
    my, mx = (h + 15) // 16, (w + 15) // 16           # MCUs
    bh, bw = (h + 7) // 8, (w + 7) // 8               # the Y component's own block grid
    yq = quantise(fdct_islow(to_blocks(_edge(y, 8 * bh, 8 * bw))), qlum)   # (bh, bw, 64)
    cq = [quantise(fdct_islow(to_blocks(h2v2_downsample(p, 8 * my, 8 * mx))), qchr) for p in (cb, cr)]
    # compress_data (jccoefct.c): per MCU Y00 Y01 Y10 Y11 Cb Cr; a block beyond the component's
    # grid is a dummy: AC zero, DC = the DC of the block before it in the MCU
    coef = np.zeros((my, mx, 6, 64), np.int64)
    dummy = np.zeros((my, mx, 6), bool)
    for k in range(4):
        by = 2 * np.arange(my)[:, None] + (k >> 1)
        bx = 2 * np.arange(mx)[None, :] + (k & 1)
        real = (by < bh) & (bx < bw)
        coef[:, :, k, :] = np.where(real[..., None], yq[np.minimum(by, bh - 1), np.minimum(bx, bw - 1)], 0)
        dummy[:, :, k] = ~real
        if k:
            coef[:, :, k, 0] = np.where(real, coef[:, :, k, 0], coef[:, :, k - 1, 0])
    coef[:, :, 4, :] = cq[0]
    coef[:, :, 5, :] = cq[1]
    comp = np.broadcast_to(np.array([0, 0, 0, 0, 1, 2]), (my, mx, 6))
    return Blocks(coef.reshape(-1, 64), comp.reshape(-1).copy(), dummy.reshape(-1))


# ---------------------------------------------------------------------------
# entropy coding (jchuff.c: encode_one_block, emit_bits, flush_bits)
# ---------------------------------------------------------------------------
_NBITS = np.zeros(4096, np.int64)
for _k in range(1, 4096):
    _NBITS[_k] = _k.bit_length()


class Tokens(object):
    """per block 65 slots of (bits, length): slot 0 the DC code + value, slot z (1..63) the code of a
    nonzero coefficient with the ZRLs in front of it, slot 64 EOB.  Counters for the tests."""

    def __init__(self, value, length, zrl, max_dc_cat, eob):
        self.value, self.length, self.zrl, self.max_dc_cat, self.eob = value, length, zrl, max_dc_cat, eob


def tokens_of(blocks):
    coef, comp = blocks.coef, blocks.comp
    n = coef.shape[0]
    tbl = (comp > 0).astype(np.int64)
    value = np.zeros((n, 65), np.uint64)
    length = np.zeros((n, 65), np.int64)
    # DC: difference against the previous block of the same component (last_dc_val)
    diff = np.zeros(n, np.int64)
    for c in range(3):
        idx = np.nonzero(comp == c)[0]
        if idx.size:
            dc = coef[idx, 0]
            diff[idx] = dc - np.concatenate([[0], dc[:-1]])
    cat = _NBITS[np.abs(diff)]
    # a negative value is sent as the low bits of value - 1
    low = np.where(diff < 0, diff - 1, diff) & ((1 << cat) - 1)
    for t in (0, 1):
        m = tbl == t
        code, size = DC_CODE[t]
        value[m, 0] = (code[cat[m]] << cat[m].astype(np.uint64)) | low[m].astype(np.uint64)
        length[m, 0] = size[cat[m]] + cat[m]
    # AC: run of zeros r before each nonzero coefficient; r > 15 -> ZRL (0xF0) per 16
    ac = coef[:, 1:]
    nz = ac != 0
    pos = np.arange(1, 64, dtype=np.int64)[None, :]
    last = np.maximum.accumulate(np.where(nz, pos, 0), axis=1)
    prev = np.concatenate([np.zeros((n, 1), np.int64), last[:, :-1]], axis=1)
    run = pos - prev - 1
    size_ac = _NBITS[np.abs(ac)]
    low_ac = np.where(ac < 0, ac - 1, ac) & ((1 << size_ac) - 1)
    nzrl = np.where(nz, run >> 4, 0)
    sym = ((run & 15) << 4) | size_ac
    for t in (0, 1):
        code, size = AC_CODE[t]
        m = (tbl == t)[:, None] & nz
        zc, zs = int(code[0xF0]), int(size[0xF0])
        s = sym[m]
        k = nzrl[m]
        v = np.zeros(s.shape, np.uint64)
        for j in (1, 2, 3):   # (a run is at most 62: up to three ZRLs)
            v = np.where(k >= j, (v << np.uint64(zs)) | np.uint64(zc), v)
        sa = size_ac[m]
        v = (v << (size[s] + sa).astype(np.uint64)) | (code[s] << sa.astype(np.uint64)) | low_ac[m].astype(np.uint64)
        vv = value[:, 1:64]
        ll = length[:, 1:64]
        vv[m] = v
        ll[m] = k * zs + size[s] + sa
        # EOB (0x00) when the block ends in zeros
        e = (tbl == t) & (last[:, -1] != 63)
        value[e, 64] = code[0]
        length[e, 64] = size[0]
    return Tokens(value, length, int(nzrl.sum()), int(cat.max()) if n else 0, int((length[:, 64] > 0).sum()))


def block_bits(blocks):
    """bits every block's codes take (what the GPU's length pass computes)"""
    return tokens_of(blocks).length.sum(axis=1)


def pack_scan(tokens):
    """emit_bits MSB first; flush_bits pads the last byte with 1-bits; -> bytes before stuffing"""
    value = tokens.value.reshape(-1)
    length = tokens.length.reshape(-1)
    keep = length > 0
    value, length = value[keep], length[keep]
    total = int(length.sum())
    owner = np.repeat(np.arange(length.size), length)
    start = np.cumsum(length) - length
    k = np.arange(total, dtype=np.int64) - start[owner]
    shift = (length[owner] - 1 - k).astype(np.uint64)
    bits = ((value[owner] >> shift) & np.uint64(1)).astype(np.uint8)
    pad = (-total) % 8
    bits = np.concatenate([bits, np.ones(pad, np.uint8)])
    return np.packbits(bits)


def stuff(raw):
    """emit_byte's 0xFF -> 0xFF 0x00"""
    ff = np.nonzero(raw == 0xFF)[0]
    return np.insert(raw, ff + 1, 0)


# ---------------------------------------------------------------------------
# the file (jcmarker.c)
# ---------------------------------------------------------------------------


def _seg(marker, payload):
    n = len(payload) + 2
    return bytes([0xFF, marker, n >> 8, n & 255]) + bytes(payload)


def header(width, height, channels, quality):
    """write_file_header + write_frame_header + write_scan_header: SOI, APP0 (JFIF 1.01, no units,
    density 1 x 1), one DQT per table, SOF0, one DHT per table (DC then AC, per component), SOS"""
    qlum, qchr = quant_tables(quality)
    out = b"\xff\xd8"
    out += _seg(0xE0, b"JFIF\0" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
    out += _seg(0xDB, bytes([0]) + bytes(int(v) for v in qlum[ZIGZAG]))
    if channels == 3:
        out += _seg(0xDB, bytes([1]) + bytes(int(v) for v in qchr[ZIGZAG]))
    # (gray: Pillow's subsampling=2 sets the one component's factors to 2 x 2 as well; a scan of one
    # component is not interleaved, so the data are those of a 1 x 1 component -- the fixtures decide)
    comps = [(1, 0x22, 0)] if channels == 1 else [(1, 0x22, 0), (2, 0x11, 1), (3, 0x11, 1)]
    sof = bytes([8, height >> 8, height & 255, width >> 8, width & 255, len(comps)])
    for cid, samp, tq in comps:
        sof += bytes([cid, samp, tq])
    out += _seg(0xC0, sof)
    out += _seg(0xC4, bytes([0x00] + DC_LUM_BITS + DC_VALS))
    out += _seg(0xC4, bytes([0x10] + AC_LUM_BITS + AC_LUM_VALS))
    if channels == 3:
        out += _seg(0xC4, bytes([0x01] + DC_CHR_BITS + DC_VALS))
        out += _seg(0xC4, bytes([0x11] + AC_CHR_BITS + AC_CHR_VALS))
    sos = bytes([len(comps)])
    for cid, _, tq in comps:
        sos += bytes([cid, tq * 0x11])
    out += _seg(0xDA, sos + bytes([0, 63, 0]))
    return out


class Encoded(object):
    def __init__(self, data, blocks, tokens, raw_scan):
        self.data, self.blocks, self.tokens, self.raw_scan = data, blocks, tokens, raw_scan

    @property
    def stuffed(self):
        return int((self.raw_scan == 0xFF).sum())


def encode_full(image, quality=95):
    image = np.asarray(image)
    blocks = blocks_of(image, quality)
    tokens = tokens_of(blocks)
    raw = pack_scan(tokens)
    h, w = image.shape[:2]
    data = header(w, h, 1 if image.ndim == 2 else 3, quality) + stuff(raw).tobytes() + b"\xff\xd9"
    return Encoded(data, blocks, tokens, raw)


def encode(image, quality=95):
    """-> the file's bytes"""
    return encode_full(image, quality).data


# ---------------------------------------------------------------------------
# decoder (baseline, what encode() writes and a little more: any sampling factors)
# ---------------------------------------------------------------------------


class Decoded(object):
    """width, height; comps: list of dicts (id, h, v, tq, td, ta); qtables {id: natural-order 64};
    coef (N, 64) quantised, zigzag order, scan order; comp (N,); pixels (H, W) or (H, W, 3) B, G, R"""
    pass


def _decode_tables(bits, vals):
    """16-bit lookahead -> (length, symbol)"""
    look_len = np.zeros(65536, np.uint8)
    look_sym = np.zeros(65536, np.uint8)
    for sym, (code, length) in huff_codes(bits, vals).items():
        lo = code << (16 - length)
        look_len[lo:lo + (1 << (16 - length))] = length
        look_sym[lo:lo + (1 << (16 - length))] = sym
    return look_len.tolist(), look_sym.tolist()


def parse_segments(data):
    """-> list of (marker, payload) up to SOS, the entropy-coded bytes (still stuffed), and whether
    the file ends with EOI"""
    assert data[:2] == b"\xff\xd8", "no SOI"
    p, segs = 2, []
    while True:
        assert data[p] == 0xFF, "marker expected at %d" % p
        m = data[p + 1]
        n = (data[p + 2] << 8) | data[p + 3]
        segs.append((m, data[p + 4:p + 2 + n]))
        p += 2 + n
        if m == 0xDA:
            break
    assert data[-2:] == b"\xff\xd9", "no EOI"
    return segs, data[p:-2]


def decode(data):
    data = bytes(data)
    segs, scan = parse_segments(data)
    out = Decoded()
    out.qtables, huff = {}, {}
    for m, pl in segs:
        if m == 0xDB:
            q = 0
            while q < len(pl):
                assert pl[q] >> 4 == 0, "16-bit quantisation table"
                t = np.zeros(64, np.int64)
                t[ZIGZAG] = np.frombuffer(pl[q + 1:q + 65], np.uint8)
                out.qtables[pl[q] & 15] = t
                q += 65
        elif m == 0xC4:
            q = 0
            while q < len(pl):
                bits = list(pl[q + 1:q + 17])
                nv = sum(bits)
                huff[pl[q]] = _decode_tables(bits, list(pl[q + 17:q + 17 + nv]))
                q += 17 + nv
        elif m == 0xC0:
            assert pl[0] == 8
            out.height, out.width = (pl[1] << 8) | pl[2], (pl[3] << 8) | pl[4]
            out.comps = [dict(id=pl[6 + 3 * i], h=pl[7 + 3 * i] >> 4, v=pl[7 + 3 * i] & 15,
                              tq=pl[8 + 3 * i]) for i in range(pl[5])]
        elif m == 0xDA:
            assert pl[0] == len(out.comps)
            for i, c in enumerate(out.comps):
                assert pl[1 + 2 * i] == c["id"]
                c["td"], c["ta"] = pl[2 + 2 * i] >> 4, pl[2 + 2 * i] & 15
        elif m in (0xC1, 0xC2, 0xC9, 0xCA, 0xDD):
            raise AssertionError("not a baseline file without restarts: marker %02x" % m)
    # unstuff
    raw = np.frombuffer(scan, np.uint8)
    ff = np.nonzero(raw[:-1] == 0xFF)[0]
    assert np.all(raw[ff + 1] == 0), "marker inside the scan"
    raw = np.delete(raw, ff + 1)
    buf = raw.tobytes() + b"\xff\xff\xff\xff"
    if len(out.comps) == 1:   # a scan of one component is not interleaved: one block per MCU
        out.comps[0]["h"] = out.comps[0]["v"] = 1
    hmax, vmax = max(c["h"] for c in out.comps), max(c["v"] for c in out.comps)
    mx = (out.width + 8 * hmax - 1) // (8 * hmax)
    my = (out.height + 8 * vmax - 1) // (8 * vmax)
    order = [ci for ci, c in enumerate(out.comps) for _ in range(c["h"] * c["v"])]
    nb = mx * my * len(order)
    coef = np.zeros((nb, 64), np.int64)
    pred = [0] * len(out.comps)
    p = 0   # bit position

    def peek16():
        q = p >> 3
        return (int.from_bytes(buf[q:q + 4], "big") >> (16 - (p & 7))) & 0xFFFF

    def receive(nbits):
        q = p >> 3
        return (int.from_bytes(buf[q:q + 4], "big") >> (32 - (p & 7) - nbits)) & ((1 << nbits) - 1)

    b = 0
    for _ in range(mx * my):
        for ci in order:
            c = out.comps[ci]
            dl, ds = huff[c["td"]]
            al, asym = huff[0x10 | c["ta"]]
            w = peek16()
            assert dl[w], "bad DC code in block %d" % b
            p += dl[w]
            s = ds[w]
            d = 0
            if s:
                d = receive(s)
                p += s
                if d < (1 << (s - 1)):
                    d -= (1 << s) - 1
            pred[ci] += d
            row = coef[b]
            row[0] = pred[ci]
            k = 1
            while k < 64:
                w = peek16()
                assert al[w], "bad AC code in block %d at %d" % (b, k)
                p += al[w]
                rs = asym[w]
                r, s = rs >> 4, rs & 15
                if s == 0:
                    if r != 15:
                        break
                    k += 16
                    continue
                k += r
                v = receive(s)
                p += s
                if v < (1 << (s - 1)):
                    v -= (1 << s) - 1
                assert k < 64, "run past the block in block %d" % b
                row[k] = v
                k += 1
            b += 1
    assert (p + 7) // 8 == len(raw), "scan length: %d bits read, %d bytes" % (p, len(raw))
    out.scan_bits = p
    out.coef = coef
    out.comp = np.tile(np.array(order), mx * my)
    out.pixels = _reconstruct(out, mx, my, hmax, vmax)
    return out


def _idct_matrix():
    k = np.arange(8)
    m = np.cos((2 * k[None, :] + 1) * k[:, None] * np.pi / 16) * 0.5
    m[0, :] = np.sqrt(0.125)
    return m   # (frequency, sample)


def _reconstruct(d, mx, my, hmax, vmax):
    """dequantise, float IDCT, level shift, box upsampling, YCbCr -> BGR; rounding only at the end"""
    m = _idct_matrix()
    planes = []
    per_mcu = sum(c["h"] * c["v"] for c in d.comps)
    coef = d.coef.reshape(my, mx, per_mcu, 64)
    at = 0
    for c in d.comps:
        n = c["h"] * c["v"]
        nat = np.zeros((my, mx, n, 64))
        nat[..., ZIGZAG] = coef[:, :, at:at + n, :] * d.qtables[c["tq"]][ZIGZAG]
        at += n
        blk = nat.reshape(my, mx, c["v"], c["h"], 8, 8)
        px = np.einsum("ur,...uv,vc->...rc", m, blk, m) + 128.0
        plane = px.transpose(0, 2, 4, 1, 3, 5).reshape(my * c["v"] * 8, mx * c["h"] * 8)
        plane = np.repeat(np.repeat(plane, vmax // c["v"], axis=0), hmax // c["h"], axis=1)
        planes.append(plane[:d.height, :d.width])
        d.planes = getattr(d, "planes", []) + [px.transpose(0, 2, 4, 1, 3, 5).reshape(
            my * c["v"] * 8, mx * c["h"] * 8)]   # (the components before upsampling, whole blocks)
    if len(planes) == 1:
        return planes[0]
    y, cb, cr = planes[0], planes[1] - 128.0, planes[2] - 128.0
    r = y + 1.402 * cr
    g = y - 0.344136 * cb - 0.714136 * cr
    b = y + 1.772 * cb
    return np.stack([b, g, r], axis=-1)
