"""aerial_mapper_amd -- MI355X-native DSM rasterisation + grid-based orthomosaic.

The hot path of ethz-asl/aerial_mapper (dsm::Dsm::process and
ortho::OrthoBackwardGrid::process) as hand-written HIP kernels for gfx950 behind
a C ABI (include/aerial_mapper_hip.h), with host-side mirrors of the reference's
class API.  See DESIGN.md / INTEGRATION.md.
"""
from .hip_lib import (AmhipError, Camera, GridDesc, DIST_EQUIDISTANT, DIST_NONE,  # noqa: F401
                      DIST_RADTAN, LAYER_NAMES, make_grid, cell_position)
from .mapper import (AerialGridMap, Dsm, DsmSettings, GridMapSettings, HostSession, NCamera,  # noqa: F401
                     OrthoBackwardGrid, OrthoForwardHomography, OrthoForwardHomographySettings,
                     OrthoFromPcl, OrthoFromPclSettings, OrthoSettings, SgbmParameters, BmParameters,
                     BlockMatchingParameters, compose_T_G_C, compute_disparity_sgbm, compute_disparity_bm, densify, dense_cloud_from_stereo_pair, rectify_stereo_pair,
                     Stereo, StereoSettings)
from .export import encode_jpeg, write_jpeg, layer_to_jpeg, session_layer_to_jpeg  # noqa: F401
from .export import encode_png, write_png, layer_to_png, session_layer_to_png  # noqa: F401
from .export import (encode_geotiff, write_geotiff_deflate, layer_to_geotiff, encode_layer_geotiff,  # noqa: F401
                     session_layer_to_geotiff)
from .io import geotiff_info, geotiff_levels, decode_geotiff, layer_from_geotiff, session_layer_from_geotiff  # noqa: F401

__all__ = ["AerialGridMap", "GridMapSettings", "HostSession", "Dsm", "DsmSettings", "OrthoBackwardGrid",
           "OrthoSettings", "OrthoForwardHomography", "OrthoForwardHomographySettings", "OrthoFromPcl", "OrthoFromPclSettings", "NCamera", "compose_T_G_C", "densify", "rectify_stereo_pair", "SgbmParameters", "compute_disparity_sgbm", "BmParameters", "BlockMatchingParameters", "compute_disparity_bm", "dense_cloud_from_stereo_pair", "Stereo", "StereoSettings", "AmhipError", "Camera", "GridDesc",
           "make_grid", "cell_position", "encode_jpeg", "write_jpeg", "layer_to_jpeg", "session_layer_to_jpeg",
           "encode_png", "write_png", "layer_to_png", "session_layer_to_png",
           "encode_geotiff", "write_geotiff_deflate", "layer_to_geotiff", "encode_layer_geotiff",
           "session_layer_to_geotiff",
           "geotiff_info", "geotiff_levels", "decode_geotiff", "layer_from_geotiff", "session_layer_from_geotiff",
           "LAYER_NAMES", "DIST_NONE", "DIST_RADTAN",
           "DIST_EQUIDISTANT"]
