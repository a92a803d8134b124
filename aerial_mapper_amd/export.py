"""What leaves the map: layer images in grid_map_cv's orientation, the
GeoTiff container of io::AerialMapperIO::toGeoTiff / writeDataToDEMGeoTiffColor
(aerial-mapper-io.cc:349-509), the grid_map_msgs/GridMap message of AerialGridMap::publishOnce
(aerial-mapper-grid-map.cc:66-72) and binary point clouds.  Thin ctypes wrappers over the C ABI
(amhip_export.hip, amhip_session.hip)."""
import ctypes as C

import numpy as np

from . import hip_lib as L
from .io import DeviceCloud

# AerialGridMap::initialize's layers in construction order (aerial-mapper-grid-map.cc:25-28) and
# the amhip layer behind each (-1: never touched by the path, NaN)
GRID_MAP_LAYERS = ["ortho", "elevation", "elevation_angle", "num_observations",
                   "elevation_angle_first_view", "delta", "observation_index",
                   "observation_index_first", "colored_ortho"]


def _layer_id(name):
    return L.LAYER_NAMES.index(name) if name in L.LAYER_NAMES else -1


def layer_to_image(map_, layer, lower=0.0, upper=255.0, bgr=False):
    """amhip_layer_to_image of an AerialGridMap (its window of the map): (rows, cols) uint8, or
    (rows, cols, 3) B, G, R for the packed colour layer."""
    lib = L.load()
    rows, cols = int(map_.window[2]), int(map_.window[3])
    lid = L.LAYER_NAMES.index(layer) if isinstance(layer, str) else int(layer)
    img = np.zeros((rows, cols, 3) if bgr else (rows, cols), np.uint8)
    L.check(lib.amhip_layer_to_image(map_._h, lid, int(bool(bgr)), float(lower), float(upper),
                                     C.c_void_p(img.ctypes.data), img.strides[0]))
    return img


def session_layer_to_image(session, layer, lower=0.0, upper=255.0, bgr=False):
    """amhip_session_layer_to_image: the whole map of a HostSession."""
    lib = L.load()
    g = session.grid
    lid = L.LAYER_NAMES.index(layer) if isinstance(layer, str) else int(layer)
    img = np.zeros((g.rows, g.cols, 3) if bgr else (g.rows, g.cols), np.uint8)
    L.check(lib.amhip_session_layer_to_image(session._h, lid, int(bool(bgr)), float(lower),
                                             float(upper), C.c_void_p(img.ctypes.data),
                                             img.strides[0]))
    return img


def _is_torch(x):
    return type(x).__module__.split(".")[0] == "torch"


def _encode_image(map_, image, cap, bound_symbol, encode_symbol, *extra):
    """image -> device tensor, the format's bound, one amhip_*_encode_dev call (extra: the format's own
    arguments, behind channels) -> the file's bytes"""
    import torch
    lib = L.load()
    if not _is_torch(image):
        image = torch.from_numpy(np.ascontiguousarray(image, np.uint8)).to("cuda:%d" % map_.device)
    assert image.is_cuda and image.dtype == torch.uint8 and image.dim() in (2, 3)
    ch = 1 if image.dim() == 2 else int(image.shape[2])
    assert image.stride(-1) == 1 and (image.dim() == 2 or image.stride(1) == ch)
    h, w = int(image.shape[0]), int(image.shape[1])
    bound = getattr(lib, bound_symbol)(w, h, ch)
    out = torch.empty(max(int(bound if cap is None else cap), 1), dtype=torch.uint8, device=image.device)
    map_.wait_for_torch(image)
    n = C.c_size_t()
    L.check(getattr(lib, encode_symbol)(map_._h, C.c_void_p(image.data_ptr()), int(image.stride(0)), w, h, ch,
                                        *(extra + (C.c_void_p(out.data_ptr()),
                                                   int(out.numel() if cap is None else cap), C.byref(n)))))
    return out[:n.value].cpu().numpy().tobytes()


def _write_image(map_, filename, image, symbol, *extra):
    """one amhip_*_write call from a torch device tensor or a numpy array (extra: behind channels)"""
    fn = getattr(L.load(), symbol)
    if _is_torch(image):
        assert image.is_cuda and image.element_size() == 1 and image.stride(-1) == 1
        ch = 1 if image.dim() == 2 else int(image.shape[2])
        map_.wait_for_torch(image)
        L.check(fn(map_._h, str(filename).encode(), C.c_void_p(image.data_ptr()), 1, int(image.stride(0)),
                   int(image.shape[1]), int(image.shape[0]), ch, *extra))
        return
    image = np.ascontiguousarray(image, np.uint8)
    ch = 1 if image.ndim == 2 else image.shape[2]
    L.check(fn(map_._h, str(filename).encode(), C.c_void_p(image.ctypes.data), 0, image.strides[0],
               image.shape[1], image.shape[0], ch, *extra))


def encode_jpeg(map_, image, quality=95, cap=None):
    """amhip_jpeg_encode_dev on the map's context: the baseline JPEG file libjpeg writes for
    cv::imwrite(name, image) at this quality (colour: 4:2:0), as bytes.  image: (H, W) or (H, W, 3)
    uint8 in B, G, R -- a numpy array, or a torch device tensor (rows may be padded: stride(0) is
    the step).  cap: bytes of the device buffer the file is encoded into (default
    amhip_jpeg_bound); a file that does not fit raises AMHIP_ERR_ARG."""
    return _encode_image(map_, image, cap, "amhip_jpeg_bound", "amhip_jpeg_encode_dev", int(quality))


def write_jpeg(map_, filename, image, quality=95):
    """amhip_jpeg_write: encode on the map's device, download, write `filename`."""
    _write_image(map_, filename, image, "amhip_jpeg_write", int(quality))


def layer_to_jpeg(map_, layer, filename, lower=0.0, upper=255.0, bgr=False, quality=95):
    """amhip_layer_write_jpeg: layer_to_image on the device, encoded there, written to `filename`."""
    lid = L.LAYER_NAMES.index(layer) if isinstance(layer, str) else int(layer)
    L.check(L.load().amhip_layer_write_jpeg(map_._h, lid, int(bool(bgr)), float(lower), float(upper),
                                            int(quality), str(filename).encode()))


def session_layer_to_jpeg(session, layer, filename, lower=0.0, upper=255.0, bgr=False, quality=95):
    """amhip_session_layer_write_jpeg: the whole map of a HostSession."""
    lid = L.LAYER_NAMES.index(layer) if isinstance(layer, str) else int(layer)
    L.check(L.load().amhip_session_layer_write_jpeg(session._h, lid, int(bool(bgr)), float(lower),
                                                    float(upper), int(quality), str(filename).encode()))


def encode_png(map_, image, cap=None):
    """amhip_png_encode_dev on the map's context: the PNG file cv::imwrite(name, image) writes for a
    name that ends in .png (filter Sub, zlib level 1 with Z_RLE), as bytes.  image and cap: as
    encode_jpeg's (cap defaults to amhip_png_bound)."""
    return _encode_image(map_, image, cap, "amhip_png_bound", "amhip_png_encode_dev")


def write_png(map_, filename, image):
    """amhip_png_write: encode on the map's device, download, write `filename`."""
    _write_image(map_, filename, image, "amhip_png_write")


def layer_to_png(map_, layer, filename, lower=0.0, upper=255.0, bgr=False):
    """amhip_layer_write_png: layer_to_image on the device, encoded there without loss, written to
    `filename`."""
    lid = L.LAYER_NAMES.index(layer) if isinstance(layer, str) else int(layer)
    L.check(L.load().amhip_layer_write_png(map_._h, lid, int(bool(bgr)), float(lower), float(upper),
                                           str(filename).encode()))


def session_layer_to_png(session, layer, filename, lower=0.0, upper=255.0, bgr=False):
    """amhip_session_layer_write_png: the whole map of a HostSession."""
    lid = L.LAYER_NAMES.index(layer) if isinstance(layer, str) else int(layer)
    L.check(L.load().amhip_session_layer_write_png(session._h, lid, int(bool(bgr)), float(lower),
                                                   float(upper), str(filename).encode()))


def write_geotiff(filename, image, geotransform, utm_zone=32, northern=True):
    """amhip_geotiff_write_u8: image (H, W) or (H, W, 3) uint8, bands written in the order given."""
    lib = L.load()
    image = np.asarray(image)
    assert image.dtype == np.uint8 and image.ndim in (2, 3)
    bands = 1 if image.ndim == 2 else image.shape[2]
    if image.strides[-1] != 1 or (image.ndim == 3 and image.strides[1] != bands):
        image = np.ascontiguousarray(image)
    gt = (C.c_double * 6)(*[float(v) for v in geotransform])
    L.check(lib.amhip_geotiff_write_u8(str(filename).encode(), C.c_void_p(image.ctypes.data),
                                       image.shape[1], image.shape[0], image.strides[0], bands, gt,
                                       int(utm_zone), int(bool(northern))))


def to_geotiff(orthomosaic, xy, filename):
    """io::AerialMapperIO::toGeoTiff (aerial-mapper-io.cc:349-431): one byte band; the
    geotransform is the one the reference hard-codes (`xy` is ignored there too)."""
    write_geotiff(filename, np.asarray(orthomosaic), (464499.00, 1.0, 0.0, 5.2727e+06, 0.0, -1.0))


def write_data_to_dem_geotiff_color(ortho_image, xy, filename):
    """io::AerialMapperIO::writeDataToDEMGeoTiffColor (:433-509): bands 1, 2, 3 = channels 2, 0, 1
    of the cv::Vec3b pixel (the reference's `TODO: Fix color bands`), unit pixels at `xy`."""
    img = np.asarray(ortho_image)
    write_geotiff(filename, np.ascontiguousarray(img[:, :, [2, 0, 1]]),
                  (float(xy[0]), 1.0, 0.0, float(xy[1]), 0.0, -1.0))


def _geotiff_raster(map_, raster):
    """-> (torch device tensor or numpy array, kind, height, width, step in bytes)"""
    if _is_torch(raster):
        import torch
        assert raster.is_cuda and raster.dim() in (2, 3) and raster.stride(-1) == 1
        if raster.dim() == 3:
            assert raster.dtype == torch.uint8 and raster.shape[2] == 3 and raster.stride(1) == 3
            kind = "rgb8"
        else:
            assert raster.dtype in (torch.float32, torch.uint8)
            kind = "f32" if raster.dtype == torch.float32 else "u8"
        step = int(raster.stride(0)) * raster.element_size()
    else:
        raster = np.asarray(raster)
        assert raster.ndim in (2, 3) and raster.dtype in (np.float32, np.uint8)
        if raster.ndim == 3:
            assert raster.dtype == np.uint8 and raster.shape[2] == 3
        raster = np.ascontiguousarray(raster)
        kind = "rgb8" if raster.ndim == 3 else "f32" if raster.dtype == np.float32 else "u8"
        step = raster.strides[0]
    return raster, L.GEOTIFF_KINDS[kind], int(raster.shape[0]), int(raster.shape[1]), int(step)


def encode_geotiff(map_, raster, geotransform, utm_zone=32, northern=True, tile=256, cap=None, overviews=0):
    """amhip_geotiff_encode_dev on the map's context: the tiled Deflate GeoTIFF of a north-up raster,
    as bytes.  raster: (H, W) float32 or uint8, or (H, W, 3) uint8 (bands in the order given) -- a
    numpy array, or a torch device tensor (rows may be padded: stride(0) is the step).  cap: bytes
    of the device buffer the file is encoded into (default amhip_geotiff_bound); a file that does
    not fit raises AMHIP_ERR_ARG.  overviews: levels behind level 0, each half the one before it
    (amhip_geotiff_encode_ovr_dev); -1: until a level fits one tile; 0: none."""
    import torch
    lib = L.load()
    raster, kind, h, w, step = _geotiff_raster(map_, raster)
    if not _is_torch(raster):
        raster = torch.from_numpy(raster).to("cuda:%d" % map_.device)
    overviews = int(overviews)
    bound = lib.amhip_geotiff_bound_ovr(w, h, kind, int(tile), overviews) if overviews else \
        lib.amhip_geotiff_bound(w, h, kind, int(tile))
    out = torch.empty(max(int(bound if cap is None else cap), 1), dtype=torch.uint8, device=raster.device)
    map_.wait_for_torch(raster)
    gt = (C.c_double * 6)(*[float(v) for v in geotransform])
    n = C.c_size_t()
    tail = (gt, int(utm_zone), int(bool(northern)), C.c_void_p(out.data_ptr()),
            int(out.numel() if cap is None else cap), C.byref(n))
    if overviews:
        L.check(lib.amhip_geotiff_encode_ovr_dev(map_._h, C.c_void_p(raster.data_ptr()), step, w, h, kind, int(tile),
                                                 overviews, *tail))
    else:
        L.check(lib.amhip_geotiff_encode_dev(map_._h, C.c_void_p(raster.data_ptr()), step, w, h, kind, int(tile),
                                             *tail))
    return out[:n.value].cpu().numpy().tobytes()


def write_geotiff_deflate(map_, filename, raster, geotransform, utm_zone=32, northern=True, tile=256, overviews=0):
    """amhip_geotiff_write (amhip_geotiff_write_ovr with overviews): encode on the map's device, download,
    write `filename`."""
    lib = L.load()
    raster, kind, h, w, step = _geotiff_raster(map_, raster)
    gt = (C.c_double * 6)(*[float(v) for v in geotransform])
    if _is_torch(raster):
        map_.wait_for_torch(raster)
        ptr, on_device = raster.data_ptr(), 1
    else:
        ptr, on_device = raster.ctypes.data, 0
    if int(overviews):
        L.check(lib.amhip_geotiff_write_ovr(map_._h, str(filename).encode(), C.c_void_p(ptr), on_device, step, w, h,
                                            kind, int(tile), int(overviews), gt, int(utm_zone), int(bool(northern))))
        return
    L.check(lib.amhip_geotiff_write(map_._h, str(filename).encode(), C.c_void_p(ptr), on_device, step, w, h, kind,
                                    int(tile), gt, int(utm_zone), int(bool(northern))))


def _geotiff_kind(kind):
    return L.GEOTIFF_KINDS[kind] if isinstance(kind, str) else int(kind)


def layer_to_geotiff(map_, layer, filename, kind="f32", lower=0.0, upper=255.0, utm_zone=32, northern=True,
                     tile=256, overviews=0):
    """amhip_layer_write_geotiff: the map's window of a layer as its north-up raster (x easting, y
    northing), georeferenced from the map's own geometry, tiled and Deflate-compressed on the device.
    kind: "f32" (the layer's floats, nodata NaN), "u8" (layer_to_image's rescale) or "rgb8" (the
    packed colour layer as R, G, B).  overviews: as encode_geotiff's; level 1 reduces the bytes of level 0."""
    lid = L.LAYER_NAMES.index(layer) if isinstance(layer, str) else int(layer)
    if int(overviews):
        L.check(L.load().amhip_layer_write_geotiff_ovr(map_._h, lid, _geotiff_kind(kind), float(lower), float(upper),
                                                       int(tile), int(overviews), int(utm_zone),
                                                       int(bool(northern)), str(filename).encode()))
        return
    L.check(L.load().amhip_layer_write_geotiff(map_._h, lid, _geotiff_kind(kind), float(lower), float(upper),
                                               int(tile), int(utm_zone), int(bool(northern)),
                                               str(filename).encode()))


def encode_layer_geotiff(map_, layer, kind="f32", lower=0.0, upper=255.0, utm_zone=32, northern=True, tile=256,
                         cap=None, overviews=0):
    """amhip_layer_encode_geotiff_dev: layer_to_geotiff's file, as bytes."""
    import torch
    lib = L.load()
    lid = L.LAYER_NAMES.index(layer) if isinstance(layer, str) else int(layer)
    k = _geotiff_kind(kind)
    overviews = int(overviews)
    bound = lib.amhip_geotiff_bound_ovr(int(map_.window[2]), int(map_.window[3]), k, int(tile), overviews) \
        if overviews else lib.amhip_geotiff_bound(int(map_.window[2]), int(map_.window[3]), k, int(tile))
    out = torch.empty(max(int(bound if cap is None else cap), 1), dtype=torch.uint8,
                      device="cuda:%d" % map_.device)
    n = C.c_size_t()
    tail = (int(utm_zone), int(bool(northern)), C.c_void_p(out.data_ptr()),
            int(out.numel() if cap is None else cap), C.byref(n))
    if overviews:
        L.check(lib.amhip_layer_encode_geotiff_ovr_dev(map_._h, lid, k, float(lower), float(upper), int(tile),
                                                       overviews, *tail))
    else:
        L.check(lib.amhip_layer_encode_geotiff_dev(map_._h, lid, k, float(lower), float(upper), int(tile), *tail))
    return out[:n.value].cpu().numpy().tobytes()


def session_layer_to_geotiff(session, layer, filename, kind="f32", lower=0.0, upper=255.0, utm_zone=32,
                             northern=True, tile=256, overviews=0):
    """amhip_session_layer_write_geotiff (.._ovr with overviews): the whole map of a HostSession."""
    lid = L.LAYER_NAMES.index(layer) if isinstance(layer, str) else int(layer)
    if int(overviews):
        L.check(L.load().amhip_session_layer_write_geotiff_ovr(session._h, lid, _geotiff_kind(kind), float(lower),
                                                               float(upper), int(tile), int(overviews),
                                                               int(utm_zone), int(bool(northern)),
                                                               str(filename).encode()))
        return
    L.check(L.load().amhip_session_layer_write_geotiff(session._h, lid, _geotiff_kind(kind), float(lower),
                                                       float(upper), int(tile), int(utm_zone),
                                                       int(bool(northern)), str(filename).encode()))


def grid_map_msg_layout(grid, stamp_ns, frame_id="world", layers=GRID_MAP_LAYERS):
    """(buffer, payload offsets): the message with empty payloads (host only)."""
    lib = L.load()
    names = (C.c_char_p * len(layers))(*[n.encode() for n in layers])
    n = lib.amhip_grid_map_msg_bytes(C.byref(grid), frame_id.encode(), len(layers), names)
    buf = np.zeros(n, np.uint8)
    offs = (C.c_size_t * len(layers))()
    L.check(lib.amhip_grid_map_msg_layout(C.byref(grid), int(stamp_ns), frame_id.encode(),
                                          len(layers), names, C.c_void_p(buf.ctypes.data), n, offs))
    return buf, list(offs)


def session_grid_map_msg(session, stamp_ns, frame_id="world", layers=GRID_MAP_LAYERS,
                         host_layers=None, out=None):
    """amhip_session_grid_map_msg: the serialized grid_map_msgs/GridMap of a HostSession's map,
    resident layers straight from the devices.  out: a uint8 buffer to reuse (a publisher's)."""
    lib = L.load()
    names = (C.c_char_p * len(layers))(*[n.encode() for n in layers])
    ids = (C.c_int32 * len(layers))(*[_layer_id(n) for n in layers])
    hosts = (C.c_void_p * len(layers))()
    keep = []
    for k, n in enumerate(layers):
        if host_layers and n in host_layers and ids[k] < 0:
            a = np.ascontiguousarray(host_layers[n], np.float32)
            keep.append(a)
            hosts[k] = a.ctypes.data
    n = lib.amhip_grid_map_msg_bytes(C.byref(session.grid), frame_id.encode(), len(layers), names)
    buf = np.empty(n, np.uint8) if out is None else out[:n]
    assert buf.dtype == np.uint8 and buf.shape[0] == n and buf.flags.c_contiguous
    written = C.c_size_t()
    L.check(lib.amhip_session_grid_map_msg(session._h, int(stamp_ns), frame_id.encode(),
                                           len(layers), names, ids, hosts,
                                           C.c_void_p(buf.ctypes.data), n, C.byref(written)))
    assert written.value == n
    return buf


def write_point_cloud_binary(filename, xyz, intensities=None):
    lib = L.load()
    xyz = np.ascontiguousarray(xyz, np.float64).reshape(-1, 3)
    inten = None if intensities is None else np.ascontiguousarray(intensities, np.int32)
    assert inten is None or inten.shape[0] == xyz.shape[0]
    L.check(lib.amhip_io_write_point_cloud_binary(
        str(filename).encode(), C.c_void_p(xyz.ctypes.data),
        C.c_void_p(inten.ctypes.data) if inten is not None else None, xyz.shape[0]))


def load_point_cloud_binary(filename, device=0):
    """-> DeviceCloud resident in HBM (pinned double-buffered staging)."""
    lib = L.load()
    xyz, inten, n = C.c_void_p(), C.c_void_p(), C.c_size_t()
    L.check(lib.amhip_io_load_point_cloud_binary(int(device), str(filename).encode(),
                                                 C.byref(xyz), C.byref(inten), C.byref(n)))
    return DeviceCloud(xyz.value, inten.value, n.value, int(device), 0)
