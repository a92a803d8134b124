"""io::AerialMapperIO's loaders (aerial-mapper-io.cc:103-121,207-249,309-347).

`load_point_cloud_text` tokenises and parses the `x y z intensity` file on the
GPU (amhip_io.hip) and leaves the cloud in HBM, ready for Dsm.process /
OrthoFromPcl.process; `load_poses_text` reads the small pose file on the host;
`load_images` / `decode_jpeg_frames` decode the frames' JPEG files
(`<base><i>.jpg`, amhip_jpeg_decode.hip) and `load_images_named` /
`decode_png_frames` their PNG files (`<directory><name>.png`,
amhip_png_decode.hip) on the GPU; both leave them in HBM as one stack in the
same layout (DeviceFrames), ready for OrthoBackwardGrid.process,
OrthoForwardHomography.batch and Stereo.add_frames.
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


def load_images(filename_base, num_poses, colored=False, device=0):
    """io::AerialMapperIO::loadImagesFromFile: reads <filename_base><i>.jpg, i = 0..num_poses-1, and
    decodes them on the GPU -> DeviceFrames; baseline and progressive (SOF2) files alike.  A missing or
    refused file raises."""
    files = []
    for i in range(int(num_poses)):
        with open("%s%d.jpg" % (filename_base, i), "rb") as f:
            files.append(f.read())
    return decode_jpeg_frames(files, colored, device)
