"""A second, independent statement of the two kernels on either side of the stereo matchers, in
numpy only: stereo::Rectifier::rectifyStereoPair + computeMask (aerial_mapper_dense_pcl/src/
rectifier.cpp:34-128) and the loop of stereo::Densifier::computePointCloud (densifier.cpp:25-108).

Written from those two files and from the definitions of the Eigen / OpenCV calls that
oracle/amo_rectify.h adopts (its header comment), not from the kernels and not from the oracle's
C++: the oracle and the kernels share an author; this file is what both are compared with
(tests/test_stereo_front_reference.py on the CPU, tests/test_gpu_rectify.py and
tests/test_gpu_densify.py on the GPU).

Besides the results every function returns the counts a test needs to show that an input reaches
what it was built for (pixels rejected by isinf, NaN points kept, border taps, clamps that bite,
masks decided by the all-non-positive branch, pixels with w == 0) -- from this file alone."""
import numpy as np

F32 = np.float32
INVALID = 0x7FC00000          # kInvalidPoint: the quiet NaN of std::numeric_limits<float>


# ---- densifier.cpp:25-108 ------------------------------------------------------------------------
def densify_full(disp, img, K, baseline, R, t):
    """-> dict: xyz (n, 3) f64 and intensity (n,) i32 in raster order, pc2 (H * W, 4) u32, keep
    (H, W) bool, and the counts rejected_inf, nan_kept."""
    disp = np.asarray(disp, F32)
    img = np.asarray(img, np.uint8)
    H, W = disp.shape
    assert img.shape == (H, W) and baseline != 0.0                      # CHECK_NE(baseline, 0.0), :39
    K = np.asarray(K, np.float64).reshape(3, 3)
    R = np.asarray(R, np.float64).reshape(3, 3)
    t = np.asarray(t, np.float64).reshape(3)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    with np.errstate(all="ignore"):
        Q03, Q11, Q13, Q23, Q32 = -cx, fx / fy, -cy * (fx / fy), fx, np.float64(1.0) / np.float64(baseline)   # :45-47
        v, u = np.mgrid[0:H, 0:W].astype(np.float64)
        d = disp.astype(np.float64)
        w = Q32 * d                                                      # :62
        p = ((u + Q03) / w, (Q11 * v + Q13) / w, Q23 / w)                # :68-69
        g = [((R[k, 0] * p[0] + R[k, 1] * p[1]) + R[k, 2] * p[2]) + t[k] for k in range(3)]   # :72-73
        gf = [c.astype(F32) for c in g]                                  # :74-76
    above = disp > F32(1.0)                                              # :60 (false for NaN)
    keep = above & ~np.isinf(gf[2])                                      # :77
    k = keep.reshape(-1)
    xyz = np.stack([c.reshape(-1)[k] for c in g], -1).reshape(-1, 3)
    inten = img.reshape(-1)[k].astype(np.int32)
    # the PointCloud2 payload, :53-106: the offset advances BEFORE the write (:58), so pixel k lands
    # in slot k + 1, slot 0 keeps the zeros of data.resize(), the last pixel falls off the end
    rec = np.full((H * W, 4), INVALID, np.uint32)
    for c in range(3):
        rec[k, c] = gf[c].reshape(-1).view(np.uint32)[k]
    gray = img.reshape(-1).astype(np.uint32)
    rec[k, 3] = ((gray << 16) | (gray << 8) | gray)[k]
    pc2 = np.zeros((H * W, 4), np.uint32)
    pc2[1:] = rec[:-1]
    return {"xyz": xyz, "intensity": inten, "pc2": pc2, "keep": keep,
            "rejected_inf": int((above & ~keep).sum()),
            "nan_kept": int((keep & np.isnan(g[2])).sum())}


def densify_ref(disp, img, K, baseline, R, t):
    r = densify_full(disp, img, K, baseline, R, t)
    return r["xyz"], r["intensity"]


# ---- Eigen, as adopted: coefficient by coefficient, ((p0 + p1) + p2), no fused multiply-add --------
def _mul(a, b):
    return [[(a[i][0] * b[0][j] + a[i][1] * b[1][j]) + a[i][2] * b[2][j] for j in range(3)] for i in range(3)]


def _mulv(a, x):
    return [(a[i][0] * x[0] + a[i][1] * x[1]) + a[i][2] * x[2] for i in range(3)]


def _T(a):
    return [[a[j][i] for j in range(3)] for i in range(3)]


def _cof(a, i, j):
    i1, i2, j1, j2 = (i + 1) % 3, (i + 2) % 3, (j + 1) % 3, (j + 2) % 3
    return a[i1][j1] * a[i2][j2] - a[i1][j2] * a[i2][j1]


def _inv(a):
    """Eigen's fixed-size 3x3 inverse: cofactors times 1 / det, det along the first column."""
    c00, c10, c20 = _cof(a, 0, 0), _cof(a, 1, 0), _cof(a, 2, 0)
    det = (c00 * a[0][0] + c10 * a[1][0]) + c20 * a[2][0]
    invdet = np.float64(1.0) / det
    return [[_cof(a, j, i) * invdet for j in range(3)] for i in range(3)]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _norm(a):
    return np.sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2])


def _m(a):
    a = np.asarray(a, np.float64).reshape(3, 3)
    return [[np.float64(a[i, j]) for j in range(3)] for i in range(3)]


def rectify_plan(K, R1, R2, t1, t2):
    """rectifier.cpp:45-78 in float64 -> (R_G_C, baseline, T1, T1_inv f32, T2_inv f32)."""
    K, R1, R2 = _m(K), _m(R1), _m(R2)
    t1 = [np.float64(x) for x in np.asarray(t1, np.float64).reshape(3)]
    t2 = [np.float64(x) for x in np.asarray(t2, np.float64).reshape(3)]
    with np.errstate(all="ignore"):
        x = [t2[k] - t1[k] for k in range(3)]                            # :45
        baseline = _norm(x)                                              # :46
        y = _cross([R1[0][2], R1[1][2], R1[2][2]], x)                    # :49
        z = _cross(x, y)                                                 # :52
        nx, ny, nz = _norm(x), _norm(y), _norm(z)
        R = [[c / nx for c in x], [c / ny for c in y], [c / nz for c in z]]   # :55-58 (transposed)
        P33 = _mul(K, R)                                                 # :63-70, the 3x3 block
        T1 = _mul(P33, _inv(_mul(K, _T(R1))))                            # :73, :75
        T2 = _mul(P33, _inv(_mul(K, _T(R2))))                            # :74, :76
        I1 = np.array(_inv(T1), np.float64).astype(F32)                  # :77
        I2 = np.array(_inv(T2), np.float64).astype(F32)                  # :78
    return np.array(R, np.float64), float(baseline), np.array(T1, np.float64), I1, I2


def _maps(Ti, W, H):
    """:91-102, every product and every sum rounded to float32 on its own -> (mx, my, w)."""
    fv, fu = np.mgrid[0:H, 0:W].astype(F32)
    one = F32(1.0)
    with np.errstate(all="ignore"):
        x = (Ti[0, 0] * fu + Ti[0, 1] * fv) + Ti[0, 2] * one
        y = (Ti[1, 0] * fu + Ti[1, 1] * fv) + Ti[1, 2] * one
        w = (Ti[2, 0] * fu + Ti[2, 1] * fv) + Ti[2, 2] * one
        mx, my = x / w, y / w
    assert mx.dtype == F32 and w.dtype == F32
    return mx, my, w


def remap(src, mx, my):
    """cv::remap(8UC1, CV_32FC1 maps, INTER_LINEAR, BORDER_CONSTANT 0) as adopted: cvRound(map * 32)
    (to nearest even, saturated to int), 5 fractional bits, the integer part saturated to a short,
    weights (32 - fx)(32 - fy) 32 ..., (sum + 2^14) >> 15 -> (image, counts).
    What a NaN or an overflowing map value becomes (fmin / fmax saturation, so NaN -> INT_MAX, then the
    short clamp) is the convention oracle/amo_rectify.h ADOPTS, taken over here, not derived from
    OpenCV independently: no reference build confirms it (the reference's own loop stops at its CHECK
    on the one rig whose maps hold NaN)."""
    src = np.asarray(src, np.uint8)
    H, W = src.shape
    s, clamp31 = [], np.zeros(mx.shape, bool)
    for m in (mx, my):
        with np.errstate(all="ignore"):
            d = m.astype(np.float64) * 32.0
        c = np.fmax(-2147483648.0, np.fmin(2147483647.0, d))            # (fmin / fmax: a NaN gives INT_MAX)
        clamp31 |= ~(c == d)
        s.append(np.rint(c).astype(np.int64))
    sx, sy = s
    rx, ry = sx >> 5, sy >> 5
    ix, iy = np.clip(rx, -32768, 32767), np.clip(ry, -32768, 32767)
    fx, fy = sx & 31, sy & 31

    def px(xx, yy):
        inside = (xx >= 0) & (yy >= 0) & (xx < W) & (yy < H)
        return np.where(inside, src[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)].astype(np.int64), 0)
    acc = ((32 - fx) * (32 - fy) * 32 * px(ix, iy) + fx * (32 - fy) * 32 * px(ix + 1, iy) +
           (32 - fx) * fy * 32 * px(ix, iy + 1) + fx * fy * 32 * px(ix + 1, iy + 1))
    out = ((acc + (1 << 14)) >> 15).astype(np.uint8)
    rows = (iy >= -1) & (iy < H)
    counts = {"tap_left": int(((ix == -1) & rows).sum()),               # only the ix + 1 taps are inside
              "tap_right": int(((ix == W - 1) & rows).sum()),           # only the ix taps are inside
              "clamp_short": int(((ix != rx) | (iy != ry)).sum()),
              "clamp_2_31": int(clamp31.sum())}
    return out, counts


def mask_of(T1, W, H):
    """computeMask, :116-128: the corners through T1 in float64, truncated to cv::Point; the filled
    closed quadrilateral at the pixel centres: every edge function >= 0, or every one <= 0.  The
    edge functions are evaluated in Python integers.  -> (mask, corners, pixels decided by <= 0
    alone, pixels with an edge function beyond 32 bits)."""
    corners = []
    for cx, cy in ((0.0, 0.0), (W - 1.0, 0.0), (W - 1.0, H - 1.0), (0.0, H - 1.0)):
        h = _mulv(_m(T1), [np.float64(cx), np.float64(cy), np.float64(1.0)])
        with np.errstate(all="ignore"):
            qx, qy = h[0] / h[2], h[1] / h[2]
        assert abs(qx) < 2.0 ** 31 and abs(qy) < 2.0 ** 31, "the (int) of cv::Point is undefined here"
        corners.append((int(qx), int(qy)))                               # (int): towards zero
    V, U = np.mgrid[0:H, 0:W]
    V, U = V.astype(object), U.astype(object)                            # Python integers
    pos = np.ones((H, W), bool)
    neg = np.ones((H, W), bool)
    wide = np.zeros((H, W), bool)
    for k in range(4):
        (xk, yk), (xq, yq) = corners[k], corners[(k + 1) % 4]
        e = (xq - xk) * (V - yk) - (yq - yk) * (U - xk)
        pos &= (e >= 0).astype(bool)
        neg &= (e <= 0).astype(bool)
        wide |= (abs(e) >= 2 ** 31).astype(bool)
    mask = np.where(pos | neg, 255, 0).astype(np.uint8)
    return mask, corners, int((neg & ~pos).sum()), int(wide.sum())


def rectify_ref(K, R1, R2, t1, t2, left, right):
    """-> dict: R_G_C, baseline, maps (4, H, W) f32, left, right, mask, zero_w (CHECK_NE(xyw(2), 0.0)
    of :93 / :99 would have fired), and the reach counts (zero_w_pixels, neg_decided, wide_edges,
    tap_left, tap_right, clamp_short, clamp_2_31, corners)."""
    left = np.asarray(left, np.uint8)
    right = np.asarray(right, np.uint8)
    H, W = left.shape
    assert right.shape == (H, W)
    R, baseline, T1, I1, I2 = rectify_plan(K, R1, R2, t1, t2)
    x1, y1, w1 = _maps(I1, W, H)
    x2, y2, w2 = _maps(I2, W, H)
    out_l, cl = remap(left, x1, y1)
    out_r, cr = remap(right, x2, y2)
    mask, corners, neg_decided, wide_edges = mask_of(T1, W, H)
    zero = (w1 == 0) | (w2 == 0)
    r = {"R_G_C": R, "baseline": baseline, "maps": np.stack([x1, y1, x2, y2]), "left": out_l,
         "right": out_r, "mask": mask, "zero_w": bool(zero.any()), "zero_w_pixels": int(zero.sum()),
         "neg_decided": neg_decided, "wide_edges": wide_edges, "corners": corners}
    for k in cl:
        r[k] = cl[k] + cr[k]
    return r
