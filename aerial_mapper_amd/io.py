"""io::AerialMapperIO's loaders (aerial-mapper-io.cc:103-121,207-249,309-347).

`load_point_cloud_text` tokenises and parses the `x y z intensity` file on the
GPU (amhip_io.hip) and leaves the cloud in HBM, ready for Dsm.process /
OrthoFromPcl.process; `load_poses_text` reads the small pose file on the host;
`load_images` / `decode_jpeg_frames` decode the frames' JPEG files
(`<base><i>.jpg`, amhip_jpeg_decode.hip) and `load_images_named` /
`decode_png_frames` their PNG files (`<directory><name>.png`,
amhip_png_decode.hip) on the GPU; both leave them in HBM as one stack in the
same layout (DeviceFrames), ready for OrthoBackwardGrid.process,
OrthoForwardHomography.batch and Stereo.add_frames.  The other way,
`encode_jpeg_frames` / `write_jpeg_frames` turn such a stack into JPEG files
in one batched encode (amhip_jpeg.hip), `encode_png_frames` / `write_png_frames`
into PNG files without loss (amhip_png_encode.hip), and `to_standard_format` /
`export_pix4d_geofile` / `load_poses_ros` mirror the format converters built
on it (aerial-mapper-io.cc:58-101,123-205,272-307).  `geotiff_info` /
`decode_geotiff` / `layer_from_geotiff` / `session_layer_from_geotiff` read a
Deflate GeoTIFF -- a DEM, or what `layer_to_geotiff` wrote -- into a device
raster or under a map layer (amhip_tiff_decode.hip).
"""
import ctypes as C
import mmap
import os

import numpy as np

from . import hip_lib as L


def _device_view(owner, ptr, shape, typestr, strides, device):
    """A torch CUDA tensor over the library's allocation at `ptr` (strides None: packed); the tensor
    keeps `owner`, which frees the allocation, alive."""
    import torch

    class _Holder(object):
        pass

    h = _Holder()
    h.__cuda_array_interface__ = {"shape": shape, "typestr": typestr, "data": (int(ptr), False), "version": 2}
    if strides is not None:
        h.__cuda_array_interface__["strides"] = strides
    h._keepalive = owner
    return torch.as_tensor(h, device="cuda:%d" % device)


class DeviceCloud(object):
    """A point cloud resident in HBM: .xyz (n,3) float64 and .intensities (n,)
    int32 as torch CUDA tensors sharing the library's allocation."""

    def __init__(self, xyz_ptr, inten_ptr, n, device, strtod_tokens):
        self._xyz_ptr, self._inten_ptr = xyz_ptr, inten_ptr
        self.n = int(n)
        self.device = device
        self.strtod_tokens = int(strtod_tokens)

    @property
    def xyz(self):
        return _device_view(self, self._xyz_ptr, (self.n, 3), "<f8", None, self.device) if self.n else None

    @property
    def intensities(self):
        if not (self.n and self._inten_ptr):
            return None
        return _device_view(self, self._inten_ptr, (self.n,), "<i4", None, self.device)

    def to_host(self):
        xyz = np.empty((self.n, 3), np.float64)
        inten = np.empty(self.n, np.int32) if (self._inten_ptr or not self.n) else None
        if self.n:
            L.check(L.load().amhip_io_download_point_cloud(
                C.c_void_p(self._xyz_ptr), C.c_void_p(self._inten_ptr), self.n,
                C.c_void_p(xyz.ctypes.data),
                C.c_void_p(inten.ctypes.data) if inten is not None else None))
        return xyz, inten

    def close(self):
        if L is None or not (getattr(self, "_xyz_ptr", None) or getattr(self, "_inten_ptr", None)):
            return        # (nothing to free, or the interpreter is shutting down)
        lib = L.load()
        for name in ("_xyz_ptr", "_inten_ptr"):
            p = getattr(self, name, None)
            if p:
                lib.amhip_io_free(C.c_void_p(p))
                setattr(self, name, None)

    __del__ = close


def parse_point_cloud_text(text, device=0):
    """text: bytes-like content of a point-cloud file -> DeviceCloud."""
    lib = L.load()
    buf = bytes(text) if not isinstance(text, (bytes, mmap.mmap)) else text
    xyz, inten = C.c_void_p(), C.c_void_p()
    n, slow = C.c_size_t(), C.c_size_t()
    if isinstance(buf, mmap.mmap):
        addr = C.cast((C.c_char * len(buf)).from_buffer(buf), C.c_char_p)
    else:
        addr = buf
    L.check(lib.amhip_io_parse_point_cloud_text(int(device), addr, len(buf), C.byref(xyz),
                                                C.byref(inten), C.byref(n), C.byref(slow)))
    return DeviceCloud(xyz.value, inten.value, n.value, int(device), slow.value)


def load_point_cloud_text(filename, device=0):
    """io::AerialMapperIO::loadPointCloudFromFile -> DeviceCloud (CHECKs like the reference)."""
    if not filename:
        raise L.AmhipError(L.ERR_ARG, 'CHECK(filename_point_cloud != "")')
    if os.path.getsize(filename) == 0:
        raise L.AmhipError(L.ERR_ARG, "CHECK(point_cloud_xyz->size() > 0)")
    with open(filename, "rb") as f:
        data = f.read()
    cloud = parse_point_cloud_text(data, device)
    if cloud.n == 0:
        raise L.AmhipError(L.ERR_ARG, "CHECK(point_cloud_xyz->size() > 0)")
    return cloud


def load_poses_text(filename):
    """io::AerialMapperIO::loadPosesFromFileStandard: records x y z qw qx qy qz
    -> (F,7) float64 in the C boundary's layout."""
    if not filename:
        raise L.AmhipError(L.ERR_ARG, "Empty filename")
    vals = []
    with open(filename, "rb") as f:
        for tok in f.read().split():
            try:
                vals.append(float(tok))
            except ValueError:
                break
    n = len(vals) // 7
    if n == 0:
        raise L.AmhipError(L.ERR_ARG, "No poses loaded.")
    return np.asarray(vals[:7 * n], np.float64).reshape(n, 7)


class DeviceFrames(object):
    """A stack of decoded frames resident in HBM: .frames is a torch CUDA uint8 tensor (F, H, W)
    or (F, H, W, 3) (B, G, R) sharing the library's allocation."""

    def __init__(self, ptr, num_frames, width, height, channels, row_step, frame_stride, device):
        self._ptr = ptr
        self.num_frames, self.width, self.height, self.channels = int(num_frames), int(width), int(height), int(channels)
        self.row_step, self.frame_stride = int(row_step), int(frame_stride)
        self.device = device

    @property
    def frames(self):
        shape = (self.num_frames, self.height, self.width) + ((3,) if self.channels == 3 else ())
        strides = (self.frame_stride, self.row_step) + ((3, 1) if self.channels == 3 else (1,))
        return _device_view(self, self._ptr, shape, "|u1", strides, self.device)

    def to_host(self):
        """-> numpy uint8 (F, H, W) or (F, H, W, 3)"""
        shape = (self.num_frames, self.height, self.width) + ((3,) if self.channels == 3 else ())
        out = np.empty((self.num_frames, self.frame_stride), np.uint8)
        if out.size:
            L.check(L.load().amhip_io_download_frames(C.c_void_p(self._ptr), out.size, C.c_void_p(out.ctypes.data)))
        rows = out[:, :self.height * self.row_step].reshape(self.num_frames, self.height, self.row_step)
        return np.ascontiguousarray(rows[:, :, :self.width * self.channels]).reshape(shape)

    def close(self):
        if L is None or not getattr(self, "_ptr", None):
            return        # (nothing to free, or the interpreter is shutting down)
        L.load().amhip_io_free(C.c_void_p(self._ptr))
        self._ptr = None

    __del__ = close


def _image_info(symbol, data):
    data = bytes(data)
    w, h, ch = C.c_int(), C.c_int(), C.c_int()
    L.check(getattr(L.load(), symbol)(data, len(data), C.byref(w), C.byref(h), C.byref(ch)))
    return w.value, h.value, ch.value


def _decode_frames(symbol, files, colored, device):
    lib = L.load()
    files = [f if isinstance(f, bytes) else bytes(f) for f in files]
    n = len(files)
    ptrs = (C.c_char_p * max(n, 1))(*files)
    lens = (C.c_size_t * max(n, 1))(*[len(f) for f in files])
    out = C.c_void_p()
    w, h = C.c_int(), C.c_int()
    row, stride = C.c_size_t(), C.c_size_t()
    L.check(getattr(lib, symbol)(int(device), ptrs, lens, n, 1 if colored else 0, C.byref(out),
                                 C.byref(w), C.byref(h), C.byref(row), C.byref(stride)))
    return DeviceFrames(out.value, n, w.value, h.value, 3 if colored else 1, row.value, stride.value, int(device))


def jpeg_info(data):
    """-> (width, height, channels) of a JPEG file's bytes, baseline (SOF0) or progressive (SOF2); raises
    for a file the decoder refuses (of a progressive file the whole scan script is checked)."""
    return _image_info("amhip_jpeg_info", data)


def decode_jpeg_frames(files, colored=False, device=0):
    """files: list of bytes, each one baseline (SOF0) or progressive (SOF2) JPEG file of the same width
    and height, mixed in any order -> DeviceFrames (colored=False: 8UC1, of a colour file its Y plane;
    colored=True: 8UC3 B, G, R).  A progressive file must be complete: one whose scans leave a
    coefficient short of bit 0 is refused."""
    return _decode_frames("amhip_io_decode_jpeg_frames", files, colored, device)


def png_info(data):
    """-> (width, height, channels) of a PNG file's bytes (channels 1 for gray and gray + alpha, else 3);
    raises for a file the decoder refuses."""
    return _image_info("amhip_png_info", data)


def decode_png_frames(files, colored=False, device=0):
    """files: list of bytes, each one 8-bit non-interlaced PNG file of the same width and height ->
    DeviceFrames (colored=False: 8UC1; colored=True: 8UC3 B, G, R; alpha dropped)."""
    return _decode_frames("amhip_io_decode_png_frames", files, colored, device)


def load_images_named(directory, image_names, colored=False, device=0):
    """io::AerialMapperIO::loadImagesFromFile(directory, image_names, ..): reads <directory><name>.png
    for every name and decodes them on the GPU -> DeviceFrames.  A missing or refused file raises."""
    files = []
    for name in image_names:
        with open("%s%s.png" % (directory, name), "rb") as f:
            files.append(f.read())
    return decode_png_frames(files, colored, device)


_GEOTIFF_KIND_NAMES = {v: k for k, v in L.GEOTIFF_KINDS.items()}
_GEOTIFF_TYPESTR = {"f32": "<f4", "u8": "|u1", "rgb8": "|u1", "u16": "<u2", "i16": "<i2"}


def _file_bytes(data_or_path):
    if isinstance(data_or_path, (bytes, bytearray, memoryview)):
        return bytes(data_or_path)
    with open(os.fspath(data_or_path), "rb") as f:
        return f.read()


def geotiff_info(data_or_path):
    """amhip_geotiff_info (host only): a dict of the file's width, height, bands, kind ("f32", "u8",
    "rgb8", "u16", "i16"), tiled, tile_width, tile_height, rows_per_strip, compression, predictor, has_geo,
    geotransform (GDAL's six numbers, of pixel areas), epsg, raster_type and nodata (None: no tag).  Raises
    for a file the reader refuses; the text names the tag."""
    data = _file_bytes(data_or_path)
    d = L.GeotiffDesc()
    L.check(L.load().amhip_geotiff_info(data, len(data), C.byref(d)))
    return _desc_dict(d)


def _desc_dict(d):
    out = {n: int(getattr(d, n)) for n in ("width", "height", "bands", "tiled", "tile_width", "tile_height",
                                           "rows_per_strip", "compression", "predictor", "epsg", "raster_type")}
    out["kind"] = _GEOTIFF_KIND_NAMES[int(d.kind)]
    out["has_geo"] = bool(d.has_geo)
    out["geotransform"] = tuple(float(v) for v in d.geotransform)
    out["nodata"] = float(d.nodata) if d.has_nodata else None
    return out


def geotiff_levels(data_or_path):
    """amhip_geotiff_levels / amhip_geotiff_level_info (host only): geotiff_info's dict for level 0 and for
    every overview of the file, coarser and coarser.  A level's geotransform is the base's
    with the pixel size scaled by the ratio of the widths and of the heights; masks and pages of the IFD
    chain are passed over."""
    data = _file_bytes(data_or_path)
    lib = L.load()
    n = C.c_int()
    L.check(lib.amhip_geotiff_levels(data, len(data), C.byref(n)))
    out = []
    for k in range(n.value):
        d = L.GeotiffDesc()
        L.check(lib.amhip_geotiff_level_info(data, len(data), k, C.byref(d)))
        out.append(_desc_dict(d))
    return out


def _level_info(data, level):
    d = L.GeotiffDesc()
    L.check(L.load().amhip_geotiff_level_info(data, len(data), int(level), C.byref(d)))
    return _desc_dict(d)


def decode_geotiff(map_, data_or_path, window=None, step=None, level=0):
    """amhip_geotiff_decode_dev on the map's context: the pixel window (x0, y0, w, h) of the file (default:
    all of it) as a torch device tensor (h, w) of the file's dtype -- (h, w, 3) uint8 for three bands --
    and the info.  step: bytes between the tensor's rows (default: packed).  level: which level of the file
    (amhip_geotiff_decode_level_dev); window and info are that level's."""
    import torch
    data = _file_bytes(data_or_path)
    info = _level_info(data, level) if level else geotiff_info(data)
    x0, y0, w, h = (0, 0, info["width"], info["height"]) if window is None else [int(v) for v in window]
    kind = info["kind"]
    dtype = {"f32": torch.float32, "u8": torch.uint8, "rgb8": torch.uint8, "u16": torch.uint16,
             "i16": torch.int16}[kind]
    item = np.dtype(_GEOTIFF_TYPESTR[kind]).itemsize
    row = max(w, 0) * (3 if kind == "rgb8" else 1)          # samples per row
    step = row * item if step is None else int(step)
    buf = torch.zeros((max(h, 1), max(step, item)), dtype=torch.uint8, device="cuda:%d" % map_.device)
    map_.wait_for_torch(buf)
    if level:
        L.check(L.load().amhip_geotiff_decode_level_dev(map_._h, data, len(data), int(level), x0, y0, w, h,
                                                        C.c_void_p(buf.data_ptr()), step))
    else:
        L.check(L.load().amhip_geotiff_decode_dev(map_._h, data, len(data), x0, y0, w, h,
                                                  C.c_void_p(buf.data_ptr()), step))
    out = buf[:, :step - step % item].view(dtype)[:h, :row]
    return (out.unflatten(1, (w, 3)) if kind == "rgb8" else out), info


def layer_from_geotiff(map_, layer, data_or_path, level=0):
    """amhip_layer_decode_geotiff / amhip_layer_read_geotiff: the file under the map's window of `layer`.
    A cell takes the pixel its centre lies in (no resampling, no reprojection); cells outside the raster,
    on a nodata pixel or on a NaN keep what they hold.  On any error the layer is as it was.  level: which
    level of the file (amhip_layer_decode_geotiff_level / .._read_geotiff_level); -1: the coarsest level whose
    pixels are no larger than the map's cells."""
    lid = L.LAYER_NAMES.index(layer) if isinstance(layer, str) else int(layer)
    lib = L.load()
    map_._touched(L.LAYER_NAMES[lid] if 0 <= lid < len(L.LAYER_NAMES) else layer)
    if level:
        if isinstance(data_or_path, (bytes, bytearray, memoryview)):
            data = bytes(data_or_path)
            L.check(lib.amhip_layer_decode_geotiff_level(map_._h, lid, data, len(data), int(level)))
        else:
            L.check(lib.amhip_layer_read_geotiff_level(map_._h, lid, os.fsencode(data_or_path), int(level)))
        return
    if isinstance(data_or_path, (bytes, bytearray, memoryview)):
        data = bytes(data_or_path)
        L.check(lib.amhip_layer_decode_geotiff(map_._h, lid, data, len(data)))
    else:
        L.check(lib.amhip_layer_read_geotiff(map_._h, lid, os.fsencode(data_or_path)))


def session_layer_from_geotiff(session, layer, path, matrix, level=0):
    """amhip_session_layer_read_geotiff: the file under every window of a HostSession, then into `matrix`,
    the layer's host matrix as AerialGridMap.get() shapes it -- float32, shape (cols, rows), C-contiguous --,
    updated in place.  The next session call that is handed the same matrix uploads none of it."""
    lid = L.LAYER_NAMES.index(layer) if isinstance(layer, str) else int(layer)
    if not (isinstance(matrix, np.ndarray) and matrix.dtype == np.float32 and matrix.flags.c_contiguous and
            matrix.size == session.grid.rows * session.grid.cols):
        _refuse("session_layer_from_geotiff: matrix: a C-contiguous float32 array of rows * cols cells is expected")
    if level:
        L.check(L.load().amhip_session_layer_read_geotiff_level(session._h, lid, os.fsencode(path), int(level),
                                                                C.c_void_p(matrix.ctypes.data)))
        return
    L.check(L.load().amhip_session_layer_read_geotiff(session._h, lid, os.fsencode(path),
                                                      C.c_void_p(matrix.ctypes.data)))


def _refuse(text):
    raise L.AmhipError(L.ERR_ARG, text)


def _frames_arg(frames, device, to_device):
    """frames -> (pointer, on_device, F, width, height, channels, row_step, frame_stride, keepalive);
    to_device: a numpy array is uploaded first (the encode call takes device frames only)"""
    if isinstance(frames, DeviceFrames):
        return (frames._ptr, 1, frames.num_frames, frames.width, frames.height, frames.channels, frames.row_step,
                frames.frame_stride, frames)
    if isinstance(frames, np.ndarray):
        if frames.dtype != np.uint8 or frames.ndim not in (3, 4) or (frames.ndim == 4 and frames.shape[3] != 3):
            _refuse("frames: a uint8 array (F, H, W) or (F, H, W, 3) is expected")
        frames = np.ascontiguousarray(frames)
        if to_device:
            import torch
            return _frames_arg(torch.from_numpy(frames).to("cuda:%d" % device), device, False)
        n, h, w = frames.shape[:3]
        ch = 3 if frames.ndim == 4 else 1
        return frames.ctypes.data, 0, n, w, h, ch, w * ch, h * w * ch, frames
    import torch
    if not (isinstance(frames, torch.Tensor) and frames.is_cuda and frames.dtype == torch.uint8):
        _refuse("frames: a DeviceFrames, a CUDA uint8 tensor or a numpy uint8 array is expected")
    if frames.dim() not in (3, 4) or (frames.dim() == 4 and frames.shape[3] != 3):
        _refuse("frames: a tensor (F, H, W) or (F, H, W, 3) is expected")
    n, h, w = frames.shape[:3]
    ch = 3 if frames.dim() == 4 else 1
    # rows and frames may be padded; within a row the bytes are dense (a dimension of one element has
    # no stride to speak of)
    if (w > 1 and frames.stride(2) != ch) or (ch == 3 and frames.stride(3) != 1):
        _refuse("frames: only rows and frames may be strided, a row's pixels must be dense")
    row_step = frames.stride(1) if h > 1 else w * ch
    frame_stride = frames.stride(0) if n > 1 else h * row_step
    return frames.data_ptr(), 1, n, w, h, ch, row_step, frame_stride, frames


def _encode_frames(symbol, frames, device, *extra):
    """one amhip_io_encode_*_frames call (extra: the format's own arguments, behind frame_stride) -> the
    files, downloaded"""
    lib = L.load()
    ptr, _, n, w, h, ch, row, stride, keep = _frames_arg(frames, int(device), True)
    out = C.c_void_p()
    offsets = (C.c_size_t * (n + 1))()
    L.check(getattr(lib, symbol)(int(device), C.c_void_p(ptr), n, w, h, ch, row, stride, *(extra + (C.byref(out), offsets))))
    del keep
    try:
        host = np.empty(offsets[n], np.uint8)
        L.check(lib.amhip_io_download_frames(out, host.size, C.c_void_p(host.ctypes.data)))
    finally:
        lib.amhip_io_free(out)
    return [host[offsets[f]:offsets[f + 1]].tobytes() for f in range(n)]


def _write_frames(symbol, who, frames, filenames, device, *extra):
    """one amhip_io_write_*_frames call; who: the public function's name, for the refusal"""
    lib = L.load()
    ptr, on_device, n, w, h, ch, row, stride, keep = _frames_arg(frames, int(device), False)
    filenames = [os.fsencode(f) for f in filenames]
    if len(filenames) != n:
        _refuse("%s: %d frames, %d filenames" % (who, n, len(filenames)))
    names = (C.c_char_p * max(n, 1))(*filenames)
    L.check(getattr(lib, symbol)(int(device), C.c_void_p(ptr), on_device, n, w, h, ch, row, stride, *(extra + (names,))))
    del keep


def encode_jpeg_frames(frames, quality=95, device=0):
    """amhip_io_encode_jpeg_frames: every frame of a stack as the baseline JPEG file libjpeg writes at
    `quality` (8UC1 as one component, 8UC3 B, G, R as Y Cb Cr 4:2:0), all in one batched encode on the
    GPU -> list of bytes, file f what export.encode_jpeg gives for frame f.  frames: a DeviceFrames, a
    CUDA uint8 tensor (F, H, W) or (F, H, W, 3) whose rows and frames may be padded, or a numpy array."""
    return _encode_frames("amhip_io_encode_jpeg_frames", frames, device, int(quality))


def write_jpeg_frames(frames, filenames, quality=95, device=0):
    """amhip_io_write_jpeg_frames: the files of encode_jpeg_frames, written: frame f to filenames[f].  A
    file that cannot be written raises and names it; the files before it stay, none behind it is written."""
    _write_frames("amhip_io_write_jpeg_frames", "write_jpeg_frames", frames, filenames, device, int(quality))


def encode_png_frames(frames, device=0):
    """amhip_io_encode_png_frames: every frame of a stack as the PNG file cv::imwrite writes (filter Sub,
    zlib level 1 with Z_RLE; 8UC3 B, G, R stored R, G, B), all in one batched encode on the GPU -> list of
    bytes, file f what export.encode_png gives for frame f.  frames: as encode_jpeg_frames."""
    return _encode_frames("amhip_io_encode_png_frames", frames, device)


def write_png_frames(frames, filenames, device=0):
    """amhip_io_write_png_frames: the files of encode_png_frames, written: frame f to filenames[f].  A
    file that cannot be written raises and names it; the files before it stay, none behind it is written."""
    _write_frames("amhip_io_write_png_frames", "write_png_frames", frames, filenames, device)


def _leading_numbers(filename, per_record):
    """what a loop of `infile >> a >> b >> ..` reads: whole records of numbers up to the first token that
    is none"""
    vals = []
    with open(filename, "rb") as f:
        for tok in f.read().split():
            try:
                vals.append(float(tok))
            except ValueError:
                break
    n = len(vals) // per_record
    return np.asarray(vals[:per_record * n], np.float64).reshape(n, per_record)


def load_poses_ros(filename):
    """io::AerialMapperIO::loadPosesFromFileRos: records `time x y z qx qy qz qw` -> (poses (n,7) float64
    as x y z qw qx qy qz, timestamps (n,) int64: the time read as a double, then truncated)."""
    if not filename:
        _refuse("Empty filename")
    rec = _leading_numbers(filename, 8)
    if len(rec) == 0:
        _refuse("No poses loaded.")
    return np.ascontiguousarray(rec[:, [1, 2, 3, 7, 4, 5, 6]]), rec[:, 0].astype(np.int64)


def to_standard_format(directory, poses_csv, id_time_csv, new_directory, device=0):
    """io::AerialMapperIO::toStandardFormat: a simulated dataset (<directory><poses_csv>,
    <directory><id_time_csv>, <directory>cam0/<name>.png) -> <new_directory>opt_poses.txt and
    <new_directory>image_<i>.jpg.  The frames are decoded into HBM and encoded from there; only file
    bytes cross to the host.  An image without a pose raises.  Returns the associated poses (n,7)."""
    poses, stamps = load_poses_ros(directory + poses_csv)
    names, picked = [], []
    for _, name in _leading_numbers(directory + id_time_csv, 2):
        names.append(str(int(name)))
        hits = np.nonzero(stamps == int(name) - 1)[0]
        if len(hits) == 0:
            _refuse("toStandardFormat: CHECK(found_pose_for_image): no pose at timestamp %d for image %s.png"
                    % (int(name) - 1, names[-1]))
        picked.append(hits[-1])          # (the reference's loop has no break: the last match wins)
    associated = poses[picked] if picked else np.zeros((0, 7))
    with open(new_directory + "opt_poses.txt", "w") as f:
        for p in associated:
            f.write(" ".join("%g" % v for v in p) + "\n")
    frames = load_images_named(directory + "cam0/", names, False, device)
    write_jpeg_frames(frames, ["%simage_%d.jpg" % (new_directory, i) for i in range(len(names))], 95, device)
    frames.close()
    return associated


def export_pix4d_geofile(poses, frames, output_directory="/tmp/pix4d", device=0):
    """io::AerialMapperIO::exportPix4dGeofile: <output_directory>/image_%010d.jpeg, numbered from 1, in
    one batched encode, and <output_directory>/geofile.txt with a line `image_<n>.jpeg x y z` (%.15g) per
    image.  poses: (n,7) x y z qw qx qy qz; frames: as encode_jpeg_frames.  The directory is not created."""
    poses = np.asarray(poses, np.float64).reshape(-1, 7)
    n = _frames_arg(frames, int(device), False)[2]
    if n != len(poses):
        _refuse("exportPix4dGeofile: CHECK(images.size() == T_G_Cs.size()): %d images, %d poses" % (n, len(poses)))
    stems = ["image_%010d.jpeg" % (i + 1) for i in range(n)]
    write_jpeg_frames(frames, [output_directory + "/" + s for s in stems], 95, device)
    with open(output_directory + "/geofile.txt", "w") as geofile:
        for s, p in zip(stems, poses):
            geofile.write("%s %.15g %.15g %.15g\n" % (s, p[0], p[1], p[2]))


def load_images(filename_base, num_poses, colored=False, device=0):
    """io::AerialMapperIO::loadImagesFromFile: reads <filename_base><i>.jpg, i = 0..num_poses-1, and
    decodes them on the GPU -> DeviceFrames; baseline and progressive (SOF2) files alike.  A missing or
    refused file raises."""
    files = []
    for i in range(int(num_poses)):
        with open("%s%d.jpg" % (filename_base, i), "rb") as f:
            files.append(f.read())
    return decode_jpeg_frames(files, colored, device)
