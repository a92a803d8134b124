"""CPU: the C ABI of the semi-global block matcher (amhip_sgbm_default_params /
amhip_sgbm_disparity_dev): exports, the reference's defaults, the struct layout, argument errors
without a GPU, and the compiler's register / occupancy remarks of its kernels."""
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
    for name in ("amhip_sgbm_default_params", "amhip_sgbm_disparity_dev"):
        assert hasattr(lib, name) and name in L.EXPORTS
    assert L.load().amhip_kernel_name(L.K_STEREO) == b"k_stereo" and L.NUM_KERNELS == 8


def test_default_params_are_the_references(L):
    p = L.SgbmParams()
    L.load().amhip_sgbm_default_params(C.byref(p))
    # BlockMatchingParameters::SGBM (aerial_mapper_dense_pcl common.h)
    assert [getattr(p, n) for n, _ in L.SgbmParams._fields_] == [1, 80, 35, 10, 100, 20, 0, 120, 250, 9]
    import aerial_mapper_amd as A
    mine = A.SgbmParameters()
    assert [getattr(mine, n) for n, _ in L.SgbmParams._fields_] == [getattr(p, n) for n, _ in L.SgbmParams._fields_]


def test_struct_size(L):
    assert C.sizeof(L.SgbmParams) == 40


def test_argument_errors_without_a_gpu(L):
    lib = L.load()
    p = L.SgbmParams()
    lib.amhip_sgbm_default_params(C.byref(p))
    img, out = C.c_void_p(0x1000), C.c_void_p(0x2000)   # (never dereferenced: refused first)

    def call(ctx=None, W=64, H=32, ls=64, rs=64, mask=None, ms=0, ds=256, raw=None, rws=0, q=p):
        return lib.amhip_sgbm_disparity_dev(ctx, C.byref(q), W, H, img, ls, img, rs, mask, ms, out, ds,
                                            raw, rws)

    def err(**kw):
        assert call(**kw) == L.ERR_ARG
        return lib.amhip_last_error().decode()

    assert "null context" in err()
    bad = L.SgbmParams.from_buffer_copy(bytes(p))
    bad.num_disparities = 72
    assert "multiple of 16" in err(q=bad)
    bad.num_disparities = 0
    assert "multiple of 16" in err(q=bad)
    bad = L.SgbmParams.from_buffer_copy(bytes(p))
    bad.block_size = 8
    assert "block_size" in err(q=bad)
    bad.block_size = 13
    assert "block_size" in err(q=bad)
    def with_(**kw):
        q = L.SgbmParams.from_buffer_copy(bytes(p))
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    for b_ in (2, 4, 6, 10, 12, 13, 15):
        assert "block_size" in err(q=with_(block_size=b_))
    assert "multiple of 16" in err(q=with_(num_disparities=272))
    assert "multiple of 16" in err(q=with_(num_disparities=-16))
    for kw in (dict(pre_filter_cap=64), dict(p1=4097), dict(p2=4097), dict(uniqueness_ratio=101),
               dict(min_disparity=4097), dict(min_disparity=-4097)):
        assert "out of range" in err(q=with_(**kw))
    assert "width" in err(W=2, ls=2, rs=2, ds=8)
    assert "half the block" in err(W=85, ls=85, rs=85, ds=340)   # w1 = 85 - 81 = 4 = block_size / 2
    # the last accepted value of each passes on to the context check
    for kw in (dict(pre_filter_cap=63), dict(p1=4096, p2=4096), dict(uniqueness_ratio=100),
               dict(block_size=11), dict(block_size=0), dict(num_disparities=256),
               dict(speckle_range=4096), dict(speckle_range=-4096)):
        assert "null context" in err(q=with_(**kw))
    # the CV_16S map holds (min_disparity - 1) * 16 >= -32768 and (min_disparity + D) * 16 <= 32767
    for D, first_bad, last_ok in ((16, 2032, 2031), (256, 1792, 1791), (16, -2048, -2047),
                                  (256, -2048, -2047)):
        assert "CV_16S" in err(q=with_(num_disparities=D, min_disparity=first_bad))
        assert "null context" in err(q=with_(num_disparities=D, min_disparity=last_ok), W=4800, ls=4800,
                                     rs=4800, ds=19200)
    for v in (4097, -4097, 2 ** 27, 2 ** 31 - 1, -2 ** 31):
        assert "speckle_range" in err(q=with_(speckle_range=v))
    assert "step" in err(ls=63)
    assert "step" in err(rs=10)
    assert "step" in err(ds=255)
    assert "step" in err(mask=img, ms=32)
    assert "step" in err(raw=out, rws=100)
    assert lib.amhip_sgbm_disparity_dev(None, None, 64, 32, img, 64, img, 64, None, 0, out, 256,
                                        None, 0) == L.ERR_ARG


def _sgbm_kernels():
    return {k: v for k, v in _kernels().items() if "k_sgbm_" in k}


def test_kernel_budgets_as_compiled():
    ks = _sgbm_kernels()
    names = set(re.sub(r"^_ZN5amhip\d+", "", k) for k in ks)
    for want in ("k_sgbm_hsum", "k_sgbm_vsum", "k_sgbm_lrcheck", "k_sgbm_median", "k_sgbm_final"):
        assert any(n.startswith(want) for n in names), (want, sorted(names))
    paths = {k: v for k, v in ks.items() if "k_sgbm_path" in k}
    assert len(paths) == 12                    # NJ = 1..4 x (S =, S +=, winner)
    for k, v in list(paths.items()) + [(k, v) for k, v in ks.items() if "k_sgbm_hsum" in k or
                                       "k_sgbm_vsum" in k]:
        assert v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (k, v)
    # the aggregation is one wave per chain, latency bound: keep eight waves per SIMD resident
    for k, v in paths.items():
        assert v["Occupancy"] >= 8, (k, v)
    hs = next(v for k, v in ks.items() if "k_sgbm_hsum" in k)
    assert hs["Occupancy"] >= 4 and hs["LDS Size"] <= 24 * 1024, hs
