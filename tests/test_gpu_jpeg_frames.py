"""GPU: the batched JPEG encoder (amhip_io_encode_jpeg_frames / amhip_io_write_jpeg_frames, the k_jpegf_*
kernels of amhip_jpeg.hip) byte for byte: against the files libjpeg wrote (tests/golden/jpeg/), against
tests/jpeg_reference.py from padded device stacks and host arrays, against the single-image call, across
frame borders (DC prediction, partial tiles, the top-level scan), across groupings, and back through the
project's own decoder.  No Pillow, nothing of the reference tree."""
import ctypes as C
import os

import numpy as np
import pytest

import jpeg_decode_reference as D
import jpeg_inputs as I
import jpeg_reference as J

pytestmark = pytest.mark.gpu

CASES = I.cases()
_full = {}


def full(case, q):
    """the restatement's file (and its tokens), computed once per image and quality"""
    key = (case.name, q)
    if key not in _full:
        _full[key] = J.encode_full(case.image(), q)
    return _full[key]


def want(case, q):
    return full(case, q).data


def _io():
    from aerial_mapper_amd import io as AIO
    return AIO


def stack_of(cases):
    return np.stack([c.image() for c in cases])


def padded_device(stack, row_pad=13, frame_pad=29):
    """the stack in the DeviceFrames layout with rows `row_pad` and frames `frame_pad` further bytes apart
    than they need to be, the gaps filled with 0xA5"""
    import torch
    n, h, w = stack.shape[:3]
    ch = 3 if stack.ndim == 4 else 1
    row_step = w * ch + row_pad
    frame_stride = h * row_step + frame_pad
    buf = torch.full((n * frame_stride,), 0xA5, dtype=torch.uint8, device="cuda")
    shape = (n, h, w) + ((3,) if ch == 3 else ())
    view = buf.as_strided(shape, (frame_stride, row_step) + ((3, 1) if ch == 3 else (1,)))
    view.copy_(torch.from_numpy(stack).cuda())
    assert int((buf == 0xA5).sum()) >= n * (h * row_pad + frame_pad)
    return view


def by_size(size, ch):
    return [c for c in CASES if (c.width, c.height) == size and c.channels == ch]


SIZE_IDS = ["%dx%d" % s for s in I.SIZES]


# ---- 1. libjpeg's own bytes ----------------------------------------------------------------------
@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("size", I.SIZES, ids=SIZE_IDS)
def test_batch_equals_the_files_libjpeg_wrote(size, ch):
    cases = [c for c in by_size(size, ch) if os.path.exists(I.golden_npz(c))]
    assert len(cases) >= 7
    stack = stack_of(cases)
    for q in I.QUALITIES:
        files = _io().encode_jpeg_frames(stack, q)
        assert len(files) == len(cases)
        for f, c in enumerate(cases):
            assert files[f] == open(I.golden_jpg(c, q), "rb").read(), (c, q)


# ---- 2. the restatement, from padded device stacks and from the host -------------------------------
@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("size", I.SIZES, ids=SIZE_IDS)
def test_batch_equals_the_restatement_from_device_and_host(size, ch):
    cases = by_size(size, ch)
    if size in I.CONTENT_SIZES:     # "stuffed" between unstuffed neighbours
        rest = [c for c in cases if c.content != "stuffed"]
        cases = rest[:3] + [c for c in cases if c.content == "stuffed"] + rest[3:]
        assert len(cases) == len(I.CONTENTS) and cases[3].content == "stuffed"
    stack = stack_of(cases)
    dev = padded_device(stack)
    for q in I.QUALITIES:
        ref = [want(c, q) for c in cases]
        assert _io().encode_jpeg_frames(dev, q) == ref, (size, ch, q, "padded device stack")
        assert _io().encode_jpeg_frames(stack, q) == ref, (size, ch, q, "host array")
    # F = 1
    assert _io().encode_jpeg_frames(dev[2:3], 95) == [want(cases[2], 95)]
    assert _io().encode_jpeg_frames(stack[-1:], 50) == [want(cases[-1], 50)]


def test_default_quality_is_95():
    case = I.Case("noise", 33, 15, 3)
    stack = stack_of([case, case])
    assert _io().encode_jpeg_frames(stack, 0) == _io().encode_jpeg_frames(stack) == [want(case, 95)] * 2


def test_a_tensor_strided_within_a_row_is_refused():
    import torch
    from aerial_mapper_amd import hip_lib as L
    t = torch.zeros((2, 16, 32), dtype=torch.uint8, device="cuda")
    with pytest.raises(L.AmhipError):
        _io().encode_jpeg_frames(t[:, :, ::2])
    with pytest.raises(L.AmhipError):
        _io().encode_jpeg_frames(torch.zeros((2, 16, 32, 4), dtype=torch.uint8, device="cuda")[..., :3])
    with pytest.raises(L.AmhipError):
        _io().encode_jpeg_frames(np.zeros((2, 16, 32), np.float32))


# ---- 3. every file equals the single-image call -----------------------------------------------------
@pytest.mark.parametrize("ch", [1, 3])
def test_every_file_equals_the_single_image_call(ch):
    import aerial_mapper_amd as A
    from aerial_mapper_amd import export as E
    cases = by_size((129, 47), ch)
    stack = stack_of(cases)
    files = _io().encode_jpeg_frames(stack, 95)
    with A.AerialGridMap(A.GridMapSettings(0.0, 0.0, 8.0, 8.0, 1.0), device=0) as gmap:
        for f, c in enumerate(cases):
            assert files[f] == E.encode_jpeg(gmap, stack[f], 95), c


# ---- 4. DC prediction does not leak across frames ----------------------------------------------------
@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("size", [(8, 8), (16, 16), (17, 17)], ids=lambda s: "%dx%d" % s)
def test_dc_prediction_restarts_at_every_frame(size, ch):
    cases = [I.Case(c, size[0], size[1], ch) for c in ("full", "zero", "full", "checker")]
    stack = stack_of(cases)
    for q in (100, 95):
        ref = [want(c, q) for c in cases]
        assert ref[0] == ref[2] and ref[0] != ref[1]
        assert _io().encode_jpeg_frames(padded_device(stack), q) == ref
        assert _io().encode_jpeg_frames(np.ascontiguousarray(stack[::-1]), q) == ref[::-1]


# ---- 5. partial tiles, several tiles per frame, the scan's second step -----------------------------
def _noise(n, w, h, ch, salt):
    rng = np.random.default_rng([11, w, h, ch, salt])
    return rng.integers(0, 256, (n, h, w) if ch == 1 else (n, h, w, 3), dtype=np.uint8)


@pytest.mark.parametrize("w,h,ch,blocks", [(264, 136, 1, 561), (136, 264, 3, 918)])
def test_frames_of_several_tiles_with_a_partial_last_tile(w, h, ch, blocks):
    """256 blocks per workgroup of the entropy passes: a frame's tiles are its own, the last is partial"""
    nb = ((w + 7) // 8) * ((h + 7) // 8) if ch == 1 else ((w + 15) // 16) * ((h + 15) // 16) * 6
    assert nb == blocks and nb % 256 != 0 and nb > 2 * 256
    stack = _noise(3, w, h, ch, 0)
    ref = [J.encode(stack[f], 95) for f in range(3)]
    assert len(set(ref)) == 3
    assert _io().encode_jpeg_frames(padded_device(stack), 95) == ref


def test_two_large_frames_cross_the_top_level_of_the_bit_count_scan():
    """1032 x 1024 gray = 16 512 blocks = 65 tile sums per frame: each frame's wave takes a second step"""
    w, h = I.LARGE_SIZE
    assert ((w + 7) // 8) * ((h + 7) // 8) > 64 * 256
    stack = np.stack([I.large_case().image(), _noise(1, w, h, 1, 1)[0]])
    ref = [J.encode(stack[f], 95) for f in range(2)]
    assert _io().encode_jpeg_frames(stack, 95) == ref


# ---- 6. a scan that ends exactly on a byte -----------------------------------------------------------
@pytest.mark.parametrize("ch", [1, 3])
def test_a_scan_that_ends_exactly_on_a_byte_gets_no_padding(ch):
    """flush_bits pads with 1-bits only when bits are pending.  (A scan that ends exactly on a 4096-byte
    chunk: none of the committed inputs has one at any quality -- tests/jpeg_inputs.py's "stuffed" seeds
    were searched for 0xFF at a chunk's last byte, not for a scan of that length -- so that case is not
    here.)"""
    picked = []
    for size in I.CONTENT_SIZES:
        for c in by_size(size, ch):
            for q in I.QUALITIES:
                if int(full(c, q).tokens.length.sum()) % 8 == 0 and c.content not in ("zero", "full", "mid"):
                    picked.append((c, q))
    assert picked, "no committed input ends on a byte"
    for c, q in picked[:4]:
        e = full(c, q)
        assert int(e.tokens.length.sum()) == 8 * len(e.raw_scan)        # the property itself
        other = I.Case("noise", c.width, c.height, ch)
        files = _io().encode_jpeg_frames(stack_of([other, c, other]), q)
        assert files == [want(other, q), e.data, want(other, q)], (c, q)


# ---- 7. groups ------------------------------------------------------------------------------------------
def _frame_cost(w, h, ch):
    """a frame's scratch as DESIGN 4.14 states it: 128 + 4 + 208 B per scan block (the packed words rounded
    up to a 4096-byte chunk), 8 B per tile of 256 blocks and per chunk, a 32-byte record and a size word"""
    nb = ((w + 7) // 8) * ((h + 7) // 8) if ch == 1 else ((w + 15) // 16) * ((h + 15) // 16) * 6
    pack = -(-(nb * 208 + 1) // 4096) * 4096
    return nb * 132 + pack + 8 * (-(-nb // 256) + pack // 4096) + 32 + 8


# (the device cases keep the ids they had before the writer's source became a parameter)
@pytest.mark.parametrize("budget_mb,groups,source", [
    pytest.param(b, g, s, id="%s-%s%s" % (b, g, "" if s == "device" else "-host"))
    for s in ("device", "host") for b, g in [(0.125, "2, 2, 1"), (0.01, "1 each"), (0.0, "1 each")]])
def test_groups_of_frames_equal_one_group(budget_mb, groups, source, tuning, tmp_path):
    """source "host": the writer uploads the host stack group by group, group_span bytes from each
    group's first frame"""
    cost = _frame_cost(129, 47, 3)
    budget = int(budget_mb * 1048576)
    assert (2 * cost <= budget < 3 * cost) if groups == "2, 2, 1" else budget < cost
    cases = [I.Case(c, 129, 47, 3) for c in ("noise", "stuffed", "zero", "checker", "ramp")]
    stack = stack_of(cases)
    dev = padded_device(stack)
    whole, whole_offsets = _raw_encode(dev, 100)
    names = [str(tmp_path / ("g_%d.jpg" % f)) for f in range(5)]
    tuning(jpege_scratch_budget_mb=budget_mb)
    got, offsets = _raw_encode(dev, 100)
    _io().write_jpeg_frames(dev if source == "device" else stack, names, 100)
    tuning(jpege_scratch_budget_mb=None)
    assert offsets == whole_offsets and got == whole
    ref = [want(c, 100) for c in cases]
    assert [got[offsets[f]:offsets[f + 1]] for f in range(5)] == ref
    assert [open(n, "rb").read() for n in names] == ref


# ---- 8. offsets -------------------------------------------------------------------------------------------
def _raw_encode(dev, q):
    """the C call itself on a strided CUDA tensor -> (the device buffer's bytes, offsets)"""
    from aerial_mapper_amd import hip_lib as L
    lib = L.load()
    n, h, w = dev.shape[:3]
    ch = 3 if dev.dim() == 4 else 1
    out = C.c_void_p()
    offsets = (C.c_size_t * (n + 1))(*([12345] * (n + 1)))
    L.check(lib.amhip_io_encode_jpeg_frames(0, C.c_void_p(dev.data_ptr()), n, w, h, ch, dev.stride(1), dev.stride(0),
                                            q, C.byref(out), offsets))
    assert out.value
    host = np.empty(offsets[n], np.uint8)
    L.check(lib.amhip_io_download_frames(out, host.size, C.c_void_p(host.ctypes.data)))
    L.check(lib.amhip_io_free(out))
    return host.tobytes(), list(offsets)


@pytest.mark.parametrize("ch", [1, 3])
def test_offsets_are_the_prefix_sums_of_the_file_lengths(ch):
    cases = by_size((17, 17), ch)
    data, offsets = _raw_encode(padded_device(stack_of(cases)), 100)
    ref = [want(c, 100) for c in cases]
    assert len({len(r) for r in ref}) > 3
    assert offsets[0] == 0 and len(offsets) == len(cases) + 1
    assert [offsets[f + 1] - offsets[f] for f in range(len(cases))] == [len(r) for r in ref]
    assert data == b"".join(ref)          # tight: no padding between files


# ---- 9. argument errors (with a device behind them this time) ----------------------------------------
def test_argument_errors_leave_a_null_result_and_a_text():
    import torch
    from aerial_mapper_amd import hip_lib as L
    lib = L.load()
    dev = torch.zeros((3, 17, 51), dtype=torch.uint8, device="cuda")
    good = dict(frames=dev.data_ptr(), F=3, width=17, height=17, channels=3, row_step=51, frame_stride=17 * 51,
                quality=95)
    refusals = [(dict(frames=None), "null"), (dict(F=0), "F = 0"), (dict(width=0), "width"),
                (dict(width=65536), "width"), (dict(height=0), "height"), (dict(height=65536), "height"),
                (dict(channels=2), "channels"), (dict(row_step=50), "row_step"),
                (dict(frame_stride=17 * 51 - 1), "frame_stride"), (dict(quality=-1), "quality"),
                (dict(quality=101), "quality")]
    for changed, word in refusals:
        a = dict(good, **changed)
        out = C.c_void_p(0xDEAD)
        offsets = (C.c_size_t * 4)()
        rc = lib.amhip_io_encode_jpeg_frames(0, C.c_void_p(a["frames"]), a["F"], a["width"], a["height"],
                                             a["channels"], a["row_step"], a["frame_stride"], a["quality"],
                                             C.byref(out), offsets)
        text = lib.amhip_last_error().decode()
        assert rc == L.ERR_ARG and text.startswith("amhip_io_encode_jpeg_frames: ") and word in text, (changed, text)
        assert out.value is None
        names = (C.c_char_p * 3)(b"/tmp/never_a.jpg", b"/tmp/never_b.jpg", b"/tmp/never_c.jpg")
        rc = lib.amhip_io_write_jpeg_frames(0, C.c_void_p(a["frames"]), 1, a["F"], a["width"], a["height"],
                                            a["channels"], a["row_step"], a["frame_stride"], a["quality"], names)
        text = lib.amhip_last_error().decode()
        assert rc == L.ERR_ARG and text.startswith("amhip_io_write_jpeg_frames: ") and word in text, (changed, text)
    out = C.c_void_p(0xDEAD)
    assert lib.amhip_io_encode_jpeg_frames(0, C.c_void_p(dev.data_ptr()), 3, 17, 17, 3, 51, 17 * 51, 95, C.byref(out),
                                           None) == L.ERR_ARG and out.value is None
    assert lib.amhip_io_encode_jpeg_frames(0, C.c_void_p(dev.data_ptr()), 3, 17, 17, 3, 51, 17 * 51, 95, None,
                                           (C.c_size_t * 4)()) == L.ERR_ARG
    names = (C.c_char_p * 3)(b"/tmp/never_a.jpg", None, b"/tmp/never_c.jpg")
    rc = lib.amhip_io_write_jpeg_frames(0, C.c_void_p(dev.data_ptr()), 1, 3, 17, 17, 3, 51, 17 * 51, 95, names)
    assert rc == L.ERR_ARG and "filenames[1]" in lib.amhip_last_error().decode()
    assert not os.path.exists("/tmp/never_a.jpg")
    assert lib.amhip_io_write_jpeg_frames(0, C.c_void_p(dev.data_ptr()), 1, 3, 17, 17, 3, 51, 17 * 51, 95,
                                          None) == L.ERR_ARG


# ---- 10. writing ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("source", ["device", "host"])
def test_written_files_equal_the_encoded_ones(source, tmp_path):
    cases = by_size((129, 47), 3)[:5]
    stack = stack_of(cases)
    frames = padded_device(stack) if source == "device" else stack
    files = _io().encode_jpeg_frames(frames, 50)
    names = [str(tmp_path / ("w_%d.jpg" % f)) for f in range(5)]
    _io().write_jpeg_frames(frames, names, 50)
    assert [open(n, "rb").read() for n in names] == files == [want(c, 50) for c in cases]


def test_files_beyond_one_download_slice_are_written_in_order(tmp_path):
    """the writing call brings a group's files down 8 MB at a time: more than two slices, cut between files"""
    w, h = I.LARGE_SIZE
    stack = _noise(11, w, h, 1, 3)
    files = _io().encode_jpeg_frames(stack, 100)
    sizes = [len(f) for f in files]
    assert sum(sizes) > 2 * (8 << 20) and max(sizes) < (8 << 20) // 2 and len(set(files)) == 11
    assert files[0] == J.encode(stack[0], 100)
    names = [str(tmp_path / ("s_%d.jpg" % f)) for f in range(11)]
    _io().write_jpeg_frames(stack, names, 100)
    assert [open(n, "rb").read() for n in names] == files


def test_a_file_that_cannot_be_written_stops_the_call_there(tmp_path):
    from aerial_mapper_amd import hip_lib as L
    cases = by_size((17, 17), 1)[:5]
    stack = stack_of(cases)
    names = [str(tmp_path / ("e_%d.jpg" % f)) for f in range(5)]
    names[2] = str(tmp_path / "no_such_directory" / "e_2.jpg")
    with pytest.raises(L.AmhipError) as err:
        _io().write_jpeg_frames(stack, names, 95)
    assert err.value.status == L.ERR_ARG and names[2] in str(err.value) and "No such file" in str(err.value)
    assert [open(n, "rb").read() for n in names[:2]] == [want(c, 95) for c in cases[:2]]
    assert not os.path.exists(names[3]) and not os.path.exists(names[4])


# ---- 11. round trip through the project's own decoder ---------------------------------------------------
@pytest.mark.parametrize("ch", [1, 3])
def test_round_trip_through_the_loader(ch, tmp_path):
    cases = [I.Case(c, 129, 47, ch) for c in ("noise", "ramp", "checker", "stuffed")]
    base = str(tmp_path / "image_")
    names = ["%s%d.jpg" % (base, f) for f in range(len(cases))]
    _io().write_jpeg_frames(padded_device(stack_of(cases)), names, 95)
    frames = _io().load_images(base, len(cases), colored=(ch == 3))
    try:
        got = frames.to_host()
    finally:
        frames.close()
    for f, n in enumerate(names):
        d = D.decode(open(n, "rb").read())
        assert np.array_equal(got[f], d.bgr if ch == 3 else d.gray), cases[f]
