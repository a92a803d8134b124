"""CPU: the blended mosaic's interface (the three exports and amhip_ortho_blend_opts in the public
header, the built library and hip_lib; OrthoSettings' two fields) and the sanity of the rule's numpy
statement (tests/ortho_blend_reference.py) that the GPU tests compare against."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle_ffi as O
import ortho_blend_reference as B
import ortho_blend_scenes as BS
import ortho_occlusion_scenes as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = ["amhip_ortho_backward_process_blend_dev", "amhip_ortho_backward_process_blend",
           "amhip_session_ortho_backward_process_blend"]


@pytest.fixture(scope="module")
def L(hip_built):
    from aerial_mapper_amd import hip_lib
    hip_lib.load()
    return hip_lib


def test_exports_and_opts_struct(L):
    hdr = open(os.path.join(ROOT, "include", "aerial_mapper_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"typedef struct amhip_ortho_blend_opts \{(.*?)\} amhip_ortho_blend_opts;", code, re.S)
    assert m, "amhip_ortho_blend_opts is not declared"
    fields = re.findall(r"(\w+)\s+(\w+);", m.group(1))
    assert fields == [("int32_t", "sharpness"), ("int32_t", "occlusion_test"), ("double", "occlusion_margin_m")]
    assert [(n, t) for n, t in L.OrthoBlendOpts._fields_] == \
        [("sharpness", C.c_int32), ("occlusion_test", C.c_int32), ("occlusion_margin_m", C.c_double)]
    assert C.sizeof(L.OrthoBlendOpts) == 16 and L.OrthoBlendOpts.occlusion_margin_m.offset == 8
    raw = C.CDLL(L.LIB_PATH)
    lib = L.load()
    plain = {"amhip_ortho_backward_process_blend_dev": "amhip_ortho_backward_process_dev",
             "amhip_ortho_backward_process_blend": "amhip_ortho_backward_process",
             "amhip_session_ortho_backward_process_blend": "amhip_session_ortho_backward_process"}
    for name in EXPORTS:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert hasattr(raw, name), name
        assert name in L.EXPORTS
        # the plain sibling's arguments plus const amhip_ortho_blend_opts*
        assert getattr(lib, name).argtypes == getattr(lib, plain[name]).argtypes + [C.POINTER(L.OrthoBlendOpts)]
        decl = re.search(r"\bint\s+%s\s*\((.*?)\);" % name, code, re.S).group(1)
        sibling = re.search(r"\bint\s+%s\s*\((.*?)\);" % plain[name], code, re.S).group(1)
        norm = lambda s: re.sub(r"\s+", " ", s).strip()
        assert norm(decl) == norm(sibling) + ", const amhip_ortho_blend_opts* opts"


def test_refusals_need_no_device(L):
    """null context / null options fail with AMHIP_ERR_ARG before any device work."""
    lib = L.load()
    opts = L.OrthoBlendOpts(2, 0, 0.0)
    assert lib.amhip_ortho_backward_process_blend_dev(None, None, None, 0, None, 0, 0, 1, 0, C.byref(opts)) == L.ERR_ARG
    assert lib.amhip_ortho_backward_process_blend(None, None, None, 0, None, None, 1, 0, None, None, None, None,
                                                  None, None, C.byref(opts)) == L.ERR_ARG
    assert lib.amhip_session_ortho_backward_process_blend(None, None, None, 0, None, None, 1, 0, None, None, None,
                                                          None, None, None, None) == L.ERR_ARG


def test_ortho_settings_carry_the_two_fields(L):
    import aerial_mapper_amd as A
    from aerial_mapper_amd import mapper
    st = A.OrthoSettings()
    assert st.blend is False and st.blend_sharpness == 2
    assert mapper._ortho_mode(st) == ("", ())
    st = A.OrthoSettings(blend=True, blend_sharpness=3, occlusion_test=True, occlusion_margin_m=0.25)
    mode, extra = mapper._ortho_mode(st)
    opts = extra[0]._obj
    assert mode == "_blend" and (opts.sharpness, opts.occlusion_test, opts.occlusion_margin_m) == (3, 1, 0.25)
    assert mapper._ortho_mode(A.OrthoSettings(occlusion_test=True, occlusion_margin_m=0.5)) == ("_occl", (0.5,))


# ---- the reference module's own sanity ----------------------------------------------------------
def _sparse_cells(step=5):
    cells = np.zeros((SC.COLS, SC.ROWS), bool)
    cells[::step, ::step] = True
    return cells


@pytest.fixture(scope="module")
def sparse_pairs():
    return B.probe(SC.grid(), BS.camera(), BS.T_G_C(), BS.elevation("block"), _sparse_cells())


@pytest.mark.parametrize("colored", [False, True], ids=["gray", "colored"])
@pytest.mark.parametrize("sharpness", [0, 2, 4])
def test_constant_frames_give_the_constant(sparse_pairs, colored, sharpness):
    value = (37, 140, 251) if colored else 93
    images = [np.full((54, 96, 3) if colored else (54, 96), value, np.uint8) for _ in range(BS.F_MAIN)]
    lay = SC.fresh_layers(BS.elevation("block"))
    count = B.process(BS.camera(), sparse_pairs, images, lay, B.new_sums(SC.grid(), colored), colored, sharpness)
    assert (count[_sparse_cells()] >= 3).mean() > 0.5 and count[~_sparse_cells()].sum() == 0
    init = O.new_layers(SC.grid())
    name = "colored_ortho" if colored else "ortho"
    want = O.color_value_bgr(*value) if colored else np.float32(value)
    seen = count > 0
    assert np.array_equal(lay[name][seen].view(np.uint32), np.full(seen.sum(), want, np.float32).view(np.uint32))
    assert np.array_equal(lay[name][~seen], init[name][~seen], equal_nan=True)
    assert np.array_equal(np.isnan(lay["observation_index"]), ~seen)


@pytest.mark.parametrize("colored", [False, True], ids=["gray", "colored"])
def test_one_contributing_view_gives_its_pixel(sparse_pairs, colored):
    """One frame per call onto a fresh map: w * I / w rounds back to I -- the plain mosaic."""
    import ortho_occlusion_reference as R
    from aerial_mapper_amd import synth
    images = BS.frames(colored)
    for f in (0, 3):
        lay = SC.fresh_layers(BS.elevation("block"))
        count = B.process(BS.camera(), sparse_pairs, images, lay, B.new_sums(SC.grid(), colored), colored, 2,
                          None, [f])
        assert count.max() == 1 and count.sum() > 50
        plain = SC.fresh_layers(BS.elevation("block"))
        R.process(SC.grid(), BS.camera(), BS.main_poses()[f:f + 1], synth.IDENTITY_POSE, images[f:f + 1], plain,
                  colored, None)
        seen = count > 0
        for n in B.LAYERS:
            assert np.array_equal(lay[n][seen].view(np.uint32), plain[n][seen].view(np.uint32)), n


def test_main_scene_is_not_a_one_view_scene():
    """At least half of the cells have three or more contributing views, without and with the
    occlusion test (what test_gpu_ortho_blend.py asserts of the counts it is handed)."""
    for occl in (False, True):
        _, count = BS.expected(occl=occl)
        assert (count >= 3).mean() >= 0.5, (occl, (count >= 3).mean())
    # the oblique frame contributes nothing to the ground the block hides from it
    vis, occ = BS.pairs()["visible"][0], BS.occluded()[0]
    assert (vis & occ).sum() >= 50
