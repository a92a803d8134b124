"""CPU: the C ABI of the batched stereo matchers (amhip_sgbm_disparity_batch_dev,
amhip_bm_disparity_batch_dev) and of amhip_stereo_set_pairs_in_flight: the exports and the argument
errors that are reported before a context or an object is looked at."""
import ctypes as C

import pytest


@pytest.fixture(scope="module")
def L(hip_built):
    from aerial_mapper_amd import hip_lib
    hip_lib.load()
    return hip_lib


def test_exports(L):
    lib = C.CDLL(L.LIB_PATH)
    for name in ("amhip_sgbm_disparity_batch_dev", "amhip_bm_disparity_batch_dev",
                 "amhip_stereo_set_pairs_in_flight"):
        assert hasattr(lib, name) and name in L.EXPORTS
    assert L.STEREO_MAX_BATCH == 16
    hdr = open(__import__("os").path.join(__import__("os").path.dirname(L.PKG), "include",
                                          "aerial_mapper_hip.h")).read()
    assert "#define AMHIP_STEREO_MAX_BATCH 16" in hdr


W, H = 64, 32


def _call(L, matcher, ctx=None, batch=3, ls=W, lb=None, rs=W, rb=None, mask=None, ms=0, mb=0, ds=4 * W,
          db=None, raw=None, rws=0, rwb=0, q=None):
    lib = L.load()
    if matcher == "sgbm":
        p, fn = L.SgbmParams(), lib.amhip_sgbm_disparity_batch_dev
        lib.amhip_sgbm_default_params(C.byref(p))
    else:
        p, fn = L.BmParams(), lib.amhip_bm_disparity_batch_dev
        lib.amhip_bm_default_params(C.byref(p))
    p.num_disparities = 16
    for k, v in (q or {}).items():
        setattr(p, k, v)
    img, out = C.c_void_p(0x1000), C.c_void_p(0x2000)   # (never dereferenced: refused first)
    lb = H * ls if lb is None else lb
    rb = H * rs if rb is None else rb
    db = H * ds if db is None else db
    return fn(ctx, C.byref(p), W, H, batch, img, ls, lb, img, rs, rb, mask, ms, mb, out, ds, db, raw, rws, rwb)


@pytest.mark.parametrize("matcher", ["sgbm", "bm"])
def test_argument_errors_without_a_gpu(L, matcher):
    lib = L.load()

    def err(**kw):
        assert _call(L, matcher, **kw) == L.ERR_ARG
        return lib.amhip_last_error().decode()

    name = "amhip_%s_disparity_batch_dev" % matcher
    # the batch: 1 .. 16 pass on to the context check, 0 and 17 do not
    for b in (1, 2, 16):
        assert "null context" in err(batch=b)
    for b in (0, 17, -1, 1 << 20):
        msg = err(batch=b)
        assert "batch must be in [1, 16]" in msg and msg.startswith(name)
    # a batch stride below height * row step, array by array
    img, out = C.c_void_p(0x1000), C.c_void_p(0x2000)
    assert "batch stride" in err(lb=H * W - 1)
    assert "batch stride" in err(rb=H * W - 1)
    assert "batch stride" in err(db=H * 4 * W - 4)
    assert "batch stride" in err(ls=W + 8, lb=H * W)              # (the step counts, not the width)
    assert "batch stride" in err(mask=img, ms=W, mb=H * W - 1)
    assert "batch stride" in err(raw=out, rws=2 * W, rwb=H * 2 * W - 2)
    assert "batch stride" in err(batch=1, lb=0)                   # (also for one pair)
    assert "multiples of the element size" in err(db=H * 4 * W + 2)
    assert "multiples of the element size" in err(raw=out, rws=2 * W, rwb=H * 2 * W + 1)
    # accepted: the exact stride, a larger one, no mask (its stride is then not looked at), no raw map
    assert "null context" in err(lb=H * W + 13, rb=H * W + 1, db=H * 4 * W + 64)
    assert "null context" in err(mask=None, ms=0, mb=0)
    assert "null context" in err(mask=img, ms=W + 3, mb=H * (W + 3))
    assert "null context" in err(raw=out, rws=2 * W, rwb=H * 2 * W)
    # the rules of the one-pair call come first, under this call's name
    msg = err(q=dict(num_disparities=72))
    assert "multiple of 16" in msg and msg.startswith(name)
    assert "row step" in err(ls=W - 1)
    assert "block_size" in err(q=dict(block_size=4 if matcher == "bm" else 13))


def test_the_one_pair_calls_keep_their_error_texts(L):
    lib = L.load()
    img, out = C.c_void_p(0x1000), C.c_void_p(0x2000)
    p = L.SgbmParams()
    lib.amhip_sgbm_default_params(C.byref(p))
    p.num_disparities = 72
    assert lib.amhip_sgbm_disparity_dev(None, C.byref(p), W, H, img, W, img, W, None, 0, out, 4 * W, None, 0) == L.ERR_ARG
    assert lib.amhip_last_error().decode() == \
        "amhip_sgbm_disparity_dev: num_disparities must be a positive multiple of 16, <= 256"
    q = L.BmParams()
    lib.amhip_bm_default_params(C.byref(q))
    q.block_size = 4
    assert lib.amhip_bm_disparity_dev(None, C.byref(q), W, H, img, W, img, W, None, 0, out, 4 * W, None, 0) == L.ERR_ARG
    assert lib.amhip_last_error().decode() == \
        "amhip_bm_disparity_dev: block_size must be odd, in [5, 31] and <= min(width, height)"


def test_set_pairs_in_flight_refuses_bad_arguments_without_a_gpu(L):
    lib = L.load()
    for n in (0, 17, -3):
        assert lib.amhip_stereo_set_pairs_in_flight(None, n) == L.ERR_ARG
        assert "n must be in [1, 16]" in lib.amhip_last_error().decode()
    for n in (1, 16):   # (the value passes; the object is missing)
        assert lib.amhip_stereo_set_pairs_in_flight(None, n) == L.ERR_ARG
        assert "null stereo object" in lib.amhip_last_error().decode()


def test_python_signatures():
    import inspect
    import aerial_mapper_amd as A
    assert inspect.signature(A.Stereo.__init__).parameters["pairs_in_flight"].default == 1
    assert callable(A.Stereo.set_pairs_in_flight)
    # amhip_stereo_settings is untouched: the knob is not a field of it
    from aerial_mapper_amd import hip_lib
    assert C.sizeof(hip_lib.StereoSettings) == 104


# ---- the order in which errors win ------------------------------------------------------------------
def _two_faults(L, matcher, batched, width=W, left=0x1000, ls=W, ds=4 * W, batch=3, lb=None, q=None):
    """The text of a call with the given faults, through the one-pair or the batch export (no context)."""
    lib = L.load()
    p = L.SgbmParams() if matcher == "sgbm" else L.BmParams()
    getattr(lib, "amhip_%s_default_params" % matcher)(C.byref(p))
    p.num_disparities = 16
    for k, v in (q or {}).items():
        setattr(p, k, v)
    img, out = C.c_void_p(left), C.c_void_p(0x2000)   # (never dereferenced: refused first)
    right = C.c_void_p(0x1000)
    if batched:
        fn = getattr(lib, "amhip_%s_disparity_batch_dev" % matcher)
        rc = fn(None, C.byref(p), width, H, batch, img, ls, H * ls if lb is None else lb, right, W, H * W,
                None, 0, 0, out, ds, H * ds, None, 0, 0)
    else:
        fn = getattr(lib, "amhip_%s_disparity_dev" % matcher)
        rc = fn(None, C.byref(p), width, H, img, ls, right, W, None, 0, out, ds, None, 0)
    assert rc == L.ERR_ARG
    return lib.amhip_last_error().decode()


_BAD_BLOCK = {"sgbm": 13, "bm": 4}
_FEW_COLUMNS = dict(num_disparities=48, min_disparity=14)     # w1 = 64 - 62 = 2 <= 9 / 2
# (case, faults, {matcher: the text behind "amhip_<matcher>_disparity[_batch]_dev: "}); the texts are
# those of the commit before the checks were split into one rule each
_ORDER = [
    ("null left image + bad num_disparities", lambda m: dict(left=0, q=dict(num_disparities=72)),
     {"sgbm": "null argument", "bm": "null argument"}),
    ("bad width + bad block_size", lambda m: dict(width=0, q=dict(block_size=_BAD_BLOCK[m])),
     {"sgbm": "width must be in [3, 32767], height in [1, 32767]",
      "bm": "width and height must be in [1, 32767]"}),
    ("bad block_size + short row step", lambda m: dict(ls=W - 1, q=dict(block_size=_BAD_BLOCK[m])),
     {"sgbm": "block_size must be odd and <= 11 (0: OpenCV's 5)",
      "bm": "block_size must be odd, in [5, 31] and <= min(width, height)"}),
    ("short row step + misaligned disp_step", lambda m: dict(ls=W - 1, ds=4 * W + 2),
     {"sgbm": "a row step is smaller than the width", "bm": "a row step is smaller than the width"}),
    ("misaligned disp_step + too few matchable columns", lambda m: dict(ds=4 * W + 2, q=_FEW_COLUMNS),
     {"sgbm": "output steps must be multiples of the element size"}),
    ("too few matchable columns + batch 17", lambda m: dict(batch=17, q=_FEW_COLUMNS),
     {"sgbm": "fewer matchable columns than half the block"}),
]
_ORDER_BATCH = [
    ("batch 17 + short batch stride", dict(batch=17, lb=H * W - 1), "batch must be in [1, 16]"),
    ("batch 0 + null context", dict(batch=0), "batch must be in [1, 16]"),
    ("short batch stride + null context", dict(lb=H * W - 1), "a batch stride is smaller than height * row step"),
]


@pytest.mark.parametrize("matcher", ["sgbm", "bm"])
def test_a_call_with_two_faults_reports_the_same_one_as_before(L, matcher):
    for batched in (False, True):
        name = "amhip_%s_disparity_%sdev: " % (matcher, "batch_" if batched else "")
        for case, faults, want in _ORDER:
            if matcher not in want:
                continue
            kw = faults(matcher)
            if not batched and "batch" in kw:
                kw.pop("batch")     # (the one-pair call has the first fault alone)
            assert _two_faults(L, matcher, batched, **kw) == name + want[matcher], (case, batched)
    for case, kw, want in _ORDER_BATCH:
        assert _two_faults(L, matcher, True, **kw) == "amhip_%s_disparity_batch_dev: %s" % (matcher, want), case
    # without a fault, the missing context is what is left
    for batched in (False, True):
        assert _two_faults(L, matcher, batched) == "null context"
