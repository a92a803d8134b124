"""CPU: the C ABI of the block matcher (amhip_bm_default_params / amhip_bm_disparity_dev): exports,
the reference's defaults, the struct layout, argument errors without a GPU, and the compiler's
register / occupancy remarks of its kernels."""
import ctypes as C
import re

import pytest

from test_kernel_resources import _kernels


@pytest.fixture(scope="module")
def L(hip_built):
    from aerial_mapper_amd import hip_lib
    hip_lib.load()
    return hip_lib


def test_exports(L):
    lib = C.CDLL(L.LIB_PATH)
    for name in ("amhip_bm_default_params", "amhip_bm_disparity_dev"):
        assert hasattr(lib, name) and name in L.EXPORTS
    assert L.NUM_KERNELS == 8   # (BM times into the existing k_stereo slot)


def test_default_params_are_the_references(L):
    p = L.BmParams()
    L.load().amhip_bm_default_params(C.byref(p))
    # BlockMatchingParameters::BM (aerial_mapper_dense_pcl common.h)
    assert [getattr(p, n) for n, _ in L.BmParams._fields_] == [1, 80, 31, 9, 80, 20, 100, 5, 0, 15]
    import aerial_mapper_amd as A
    mine = A.BmParameters()
    assert [getattr(mine, n) for n, _ in L.BmParams._fields_] == [getattr(p, n) for n, _ in L.BmParams._fields_]
    import bm_reference as B
    assert [getattr(B.Params(), n) for n, _ in L.BmParams._fields_] == [getattr(p, n) for n, _ in L.BmParams._fields_]


def test_struct_size(L):
    assert C.sizeof(L.BmParams) == 40


def test_block_matching_parameters_picks_as_the_densifier():
    import aerial_mapper_amd as A
    q = A.BlockMatchingParameters()
    assert q.use_BM is False and isinstance(q.sgbm, A.SgbmParameters) and isinstance(q.bm, A.BmParameters)
    assert A.BlockMatchingParameters(use_BM=True).use_BM is True
    for name in ("BmParameters", "BlockMatchingParameters", "compute_disparity_bm"):
        assert name in A.__all__


def test_argument_errors_without_a_gpu(L):
    lib = L.load()
    p = L.BmParams()
    lib.amhip_bm_default_params(C.byref(p))
    img, out = C.c_void_p(0x1000), C.c_void_p(0x2000)   # (never dereferenced: refused first)

    def call(ctx=None, W=64, H=32, ls=64, rs=64, mask=None, ms=0, ds=256, raw=None, rws=0, q=p,
             left=img, right=img, disp=out):
        return lib.amhip_bm_disparity_dev(ctx, C.byref(q) if q is not None else None, W, H, left, ls,
                                          right, rs, mask, ms, disp, ds, raw, rws)

    def err(**kw):
        assert call(**kw) == L.ERR_ARG
        return lib.amhip_last_error().decode()

    def with_(**kw):
        q = L.BmParams.from_buffer_copy(bytes(p))
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    assert "null context" in err()
    assert "null argument" in err(q=None)
    assert "null argument" in err(left=None)
    assert "null argument" in err(right=None)
    assert "null argument" in err(disp=None)
    for n in (0, -16, 72, 272):
        assert "multiple of 16" in err(q=with_(num_disparities=n))
    for b in (14, 3, 1, 33, 0):
        assert "block_size" in err(q=with_(block_size=b))
    assert "block_size" in err(q=with_(block_size=31), H=29, W=64, ls=64, rs=64)   # above min(W, H)
    assert "block_size" in err(q=with_(block_size=15), W=13, ls=13, rs=13, ds=52)
    for f in (0, 64, -1):
        assert "pre_filter_size" in err(q=with_(pre_filter_size=f))
    # pre_filter_cap is overwritten by the wrapper: any value is accepted before the context check
    assert "null context" in err(q=with_(pre_filter_cap=1000))
    assert "null context" in err(q=with_(disp_12_max_diff=-7))
    assert "texture_threshold" in err(q=with_(texture_threshold=-1))
    assert "uniqueness_ratio" in err(q=with_(uniqueness_ratio=-1))
    for m in (-4097, 4097):
        assert "min_disparity" in err(q=with_(min_disparity=m))
    # the CV_16S map holds (min_disparity - 1) * 16 >= -32768 and (min_disparity + D) * 16 <= 32767
    for D, first_bad, last_ok in ((16, 2032, 2031), (256, 1792, 1791), (16, -2048, -2047),
                                  (256, -2048, -2047)):
        assert "CV_16S" in err(q=with_(num_disparities=D, min_disparity=first_bad))
        assert "null context" in err(q=with_(num_disparities=D, min_disparity=last_ok))
    # BM passes speckle_range on unscaled: nothing to overflow, any value is accepted
    assert "null context" in err(q=with_(speckle_range=2 ** 31 - 1))
    for W, H in ((0, 32), (64, 0), (32768, 32), (64, 32768)):
        assert "width and height" in err(W=W, H=H)
    assert "step" in err(ls=63)
    assert "step" in err(rs=10)
    assert "step" in err(ds=255)
    assert "step" in err(mask=img, ms=32)
    assert "step" in err(raw=out, rws=100)
    assert "multiples of the element size" in err(ds=258)
    assert "multiples of the element size" in err(raw=out, rws=129)


def _bm_kernels():
    return {re.sub(r"^_ZN5amhip\d+", "", k): v for k, v in _kernels().items() if "k_bm_" in k}


def test_kernel_budgets_as_compiled():
    ks = _bm_kernels()
    assert not any("k_sgbm_" in k for k in ks)
    pre = [v for k, v in ks.items() if k.startswith("k_bm_prefilter")]
    match = {k: v for k, v in ks.items() if k.startswith("k_bm_match")}
    assert len(pre) == 1 and len(match) == 16, sorted(ks)   # one k_bm_match per D = 16 .. 256
    for k, v in list(match.items()) + [("k_bm_prefilter", pre[0])]:
        assert v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (k, v)
    assert pre[0]["Occupancy"] >= 8
    # k_bm_match holds the band's rows in LDS (94 rows x (62 + 318) bytes: block_size <= 31,
    # D <= 256), which allows four workgroups = four waves per SIMD per CU; the registers must not
    # lower that below three (only D = 256, 8 x 32 window sums per lane, needs more than 128 VGPRs)
    for k, v in match.items():
        assert v["LDS Size"] <= 40 * 1024, (k, v)
        assert v["Occupancy"] >= (3 if "ILi32E" in k else 4), (k, v)
