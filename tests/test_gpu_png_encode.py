"""GPU: the PNG encoder (aerial_mapper_amd/csrc/amhip_png_encode.hip) byte for byte: every committed
file whose stream zlib wrote (tests/golden/png_encode/) and 20 seeded frames against
tests/png_encode_reference.py, through the single-image call, through one stack and one frame at a time;
across groupings; back through the project's own decoders without leaving HBM; the capacity rule; the
written files."""
import ctypes as C
import os

import numpy as np
import pytest

import jpeg_inputs as JI
import png_encode_inputs as I
import png_encode_reference as R

pytestmark = pytest.mark.gpu

NAMES = I.fixture_names()
_ref = {}


def want(px):
    """the restatement's file, computed once per frame"""
    key = (px.shape, px.tobytes())
    if key not in _ref:
        _ref[key] = R.encode(px)
    return _ref[key]


def _io():
    from aerial_mapper_amd import io as AIO
    return AIO


@pytest.fixture(scope="module")
def gmap():
    import aerial_mapper_amd as A
    with A.AerialGridMap(A.GridMapSettings(0.0, 0.0, 8.0, 8.0, 1.0), device=0) as m:
        yield m


def _where(got, ref):
    at = next((i for i in range(min(len(got), len(ref))) if got[i] != ref[i]), min(len(got), len(ref)))
    return "sizes %d / %d, first differing byte %d" % (len(got), len(ref), at)


def padded_device(stack, row_pad=13, frame_pad=29):
    """the stack in the DeviceFrames layout, rows and frames further apart than they need to be"""
    import torch
    n, h, w = stack.shape[:3]
    ch = 3 if stack.ndim == 4 else 1
    row_step = w * ch + row_pad
    frame_stride = h * row_step + frame_pad
    buf = torch.full((n * frame_stride,), 0xA5, dtype=torch.uint8, device="cuda")
    shape = (n, h, w) + ((3,) if ch == 3 else ())
    view = buf.as_strided(shape, (frame_stride, row_step) + ((3, 1) if ch == 3 else (1,)))
    view.copy_(torch.from_numpy(stack).cuda())
    return view


@pytest.mark.parametrize("name", NAMES)
def test_every_fixture_through_the_single_image_call_and_as_a_stack_of_one(name, gmap):
    from aerial_mapper_amd import export as E
    px, ref = I.fixture_pixels(name), I.fixture_bytes(name)
    assert want(px) == ref
    got = E.encode_png(gmap, px)
    assert got == ref, _where(got, ref)
    got = _io().encode_png_frames(px[None])[0]
    assert got == ref, _where(got, ref)


def test_fixtures_of_one_size_in_one_stack():
    """the two stream-length fixtures share no size; the 1 x 1 and the others do not either: the stack is
    built from the fixtures padded into one common frame, which the restatement encodes as well"""
    h = max(I.fixture_pixels(n).shape[0] for n in NAMES if I.fixture_pixels(n).ndim == 2 and I.fixture_pixels(n).shape[1] < 400)
    frames = []
    for n in NAMES:
        px = I.fixture_pixels(n)
        if px.ndim == 2 and px.shape[1] < 400:
            f = np.zeros((h, 400), np.uint8)
            f[:px.shape[0], :px.shape[1]] = px
            frames.append(f)
    assert len(frames) >= 3
    stack = np.stack(frames)
    assert _io().encode_png_frames(padded_device(stack)) == [want(f) for f in frames]


@pytest.mark.parametrize("colour", [False, True], ids=["gray", "colour"])
def test_twenty_random_frames_in_one_stack_and_one_at_a_time(colour, gmap):
    from aerial_mapper_amd import export as E
    frames = [f for f in I.random_frames(20) if (f.ndim == 3) == colour]
    assert len(frames) == 10
    stack = np.stack(frames)
    ref = [want(f) for f in frames]
    assert len(set(ref)) == 10
    got = _io().encode_png_frames(padded_device(stack))
    for f in range(10):
        assert got[f] == ref[f], (f, _where(got[f], ref[f]))
    assert _io().encode_png_frames(stack) == ref                        # from the host
    for f in range(10):
        assert _io().encode_png_frames(stack[f:f + 1]) == [ref[f]]
        assert E.encode_png(gmap, frames[f]) == ref[f]
    import torch
    dev = padded_device(stack)
    assert E.encode_png(gmap, dev[3]) == ref[3]                         # a device tensor with padded rows


def test_frames_of_several_blocks_and_tiles(gmap):
    """more than one block of 16383 symbols, more than 256 tiles of 4096 bytes (the scans' second step),
    a blank frame that is matches of 258 from end to end, and noise: blocks of every type side by side"""
    rng = np.random.default_rng(31)
    w, h = 1100, 401
    a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    b = np.zeros((h, w, 3), np.uint8)
    c = np.zeros((h, w, 3), np.uint8)
    c[100:200, 300:900] = rng.integers(0, 256, (100, 600, 3), dtype=np.uint8)
    c[250:, :500] = (np.arange(500)[None, :, None] // 2 + np.arange(151)[:, None, None]).astype(np.uint8)
    assert h * (1 + 3 * w) > 256 * 4096
    stack = np.stack([a, b, c])
    ref = [want(f) for f in stack]
    got = _io().encode_png_frames(stack)
    for f in range(3):
        assert got[f] == ref[f], (f, _where(got[f], ref[f]))


def _frame_cost(w, h, ch):
    """a frame's scratch as DESIGN 4.15 states it, every buffer rounded up to 256 bytes"""
    raw = h * (1 + w * ch)
    tiles = -(-raw // 4096)
    blocks = raw // 16383 + 1
    zwords = (raw + 5 * blocks + 7 + 3) // 4 + 2
    parts = [tiles * 4096, tiles * 8192] + [tiles * 4] * 4 + [tiles * 8] * 2 + \
        [(blocks + 1) * 8, blocks * 8, blocks * 1448, zwords * 4, 32, 8, 8]
    return sum(-(-p // 256) * 256 for p in parts)


# (the device cases keep the ids they had before the writer's source became a parameter)
@pytest.mark.parametrize("budget_mb,groups,source", [
    pytest.param(b, g, s, id="%s-%s%s" % (b, g, "" if s == "device" else "-host"))
    for s in ("device", "host") for b, g in [(0.15, "2, 2, 1"), (0.01, "1 each")]])
def test_groups_of_frames_equal_one_group(budget_mb, groups, source, tuning, tmp_path):
    """source "host": the writer uploads the host stack group by group, group_span bytes from each
    group's first frame"""
    frames = [f for f in I.random_frames(20) if f.ndim == 3][:5]
    cost = _frame_cost(83, 61, 3)
    budget = int(budget_mb * 1048576)
    assert (2 * cost <= budget < 3 * cost) if groups == "2, 2, 1" else budget < cost, (cost, budget)
    stack = np.stack(frames)
    dev = padded_device(stack)
    whole = _io().encode_png_frames(dev)
    names = [str(tmp_path / ("g_%d.png" % f)) for f in range(5)]
    tuning(pnge_scratch_budget_mb=budget_mb)
    got = _io().encode_png_frames(dev)
    _io().write_png_frames(dev if source == "device" else stack, names)
    tuning(pnge_scratch_budget_mb=None)
    ref = [want(f) for f in frames]
    assert got == whole == ref
    assert [open(n, "rb").read() for n in names] == ref


@pytest.mark.parametrize("colour", [False, True], ids=["gray", "colour"])
def test_the_decoder_gives_the_pixels_back_and_the_stack_stays_in_hbm(colour):
    """encode a stack, decode the files with amhip_io_decode_png_frames, encode the DeviceFrames it left
    (no host copy of the pixels in between) and get the same files; the pixels are the input's"""
    frames = [f for f in I.random_frames(20) if (f.ndim == 3) == colour][:6]
    stack = np.stack(frames)
    files = _io().encode_png_frames(stack)
    dec = _io().decode_png_frames(files, colored=colour)
    try:
        again = _io().encode_png_frames(dec)
        got = dec.to_host()
    finally:
        dec.close()
    assert np.array_equal(got, stack)
    assert again == files == [want(f) for f in frames]


def test_a_stack_from_the_jpeg_decoder_encodes_without_a_host_round_trip():
    import jpeg_reference as J
    cases = [JI.Case(c, 129, 47, 3) for c in ("noise", "ramp", "checker")]
    jpegs = [J.encode(c.image(), 95) for c in cases]
    dec = _io().decode_jpeg_frames(jpegs, colored=True)
    try:
        files = _io().encode_png_frames(dec)
        pixels = dec.to_host()
    finally:
        dec.close()
    assert files == [want(np.ascontiguousarray(pixels[f])) for f in range(3)]


def test_a_buffer_one_byte_too_small_is_refused_and_left_untouched(gmap):
    import torch
    from aerial_mapper_amd import hip_lib as L
    lib = L.load()
    for px in (I.fixture_pixels("noise_rgb_33x17"), I.fixture_pixels("idat_8193_gray_1row")):
        ref = want(px)
        size = len(ref)
        h, w = px.shape[:2]
        ch = 1 if px.ndim == 2 else 3
        dev = torch.from_numpy(px).cuda()
        n = C.c_size_t()
        out = torch.full((size + 64,), 0x5A, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        rc = lib.amhip_png_encode_dev(gmap._h, C.c_void_p(dev.data_ptr()), dev.stride(0), w, h, ch,
                                      C.c_void_p(out.data_ptr()), size - 1, C.byref(n))
        text = lib.amhip_last_error().decode()
        assert rc == L.ERR_ARG and "nothing written" in text, text
        assert n.value == size            # (the size it would have taken)
        assert bool((out == 0x5A).all()), "the buffer was written"
        rc = lib.amhip_png_encode_dev(gmap._h, C.c_void_p(dev.data_ptr()), dev.stride(0), w, h, ch,
                                      C.c_void_p(out.data_ptr()), size, C.byref(n))
        assert rc == L.OK and n.value == size
        got = out.cpu().numpy()
        assert got[:size].tobytes() == ref and (got[size:] == 0x5A).all()


@pytest.mark.parametrize("source", ["device", "host"])
def test_written_files_equal_the_encoded_ones(source, tmp_path, gmap):
    from aerial_mapper_amd import export as E
    frames = [f for f in I.random_frames(20) if f.ndim == 3][:4]
    stack = np.stack(frames)
    src = padded_device(stack) if source == "device" else stack
    names = [str(tmp_path / ("w_%d.png" % f)) for f in range(4)]
    _io().write_png_frames(src, names)
    assert [open(n, "rb").read() for n in names] == [want(f) for f in frames]
    one = str(tmp_path / "one.png")
    E.write_png(gmap, one, src[1])
    assert open(one, "rb").read() == want(frames[1])


def test_a_file_that_cannot_be_written_stops_the_call_there(tmp_path):
    """as the JPEG writer: AMHIP_ERR_ARG naming the file with errno's text, the files before it stay, none
    behind it is written"""
    from aerial_mapper_amd import hip_lib as L
    frames = [f for f in I.random_frames(20) if f.ndim == 2][:5]
    names = [str(tmp_path / ("e_%d.png" % f)) for f in range(5)]
    names[2] = str(tmp_path / "no_such_directory" / "e_2.png")
    with pytest.raises(L.AmhipError) as err:
        _io().write_png_frames(np.stack(frames), names)
    assert err.value.status == L.ERR_ARG and names[2] in str(err.value) and "No such file" in str(err.value)
    assert str(err.value).startswith("amhip_io_write_png_frames: ") or "amhip_io_write_png_frames: " in str(err.value)
    assert [open(n, "rb").read() for n in names[:2]] == [want(f) for f in frames[:2]]
    assert not os.path.exists(names[3]) and not os.path.exists(names[4])
