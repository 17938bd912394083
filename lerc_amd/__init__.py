"""lerc_amd -- MI355X-native LERC (Lerc2 v6) encode / decode.

Python host side of the C ABI in include/lerc_amd.h.  It mirrors the reference's own Python binding
(OtherLanguages/Python/lerc/_lerc.py: encode / decode / getLercBlobInfo / getLercDataRanges ...,
same argument meaning and return tuples) on top of liblerc_amd.so, and adds the device-pointer calls
used with torch tensors.  There is no CPU codec in this package: without the HIP library or without a
GPU every call fails loudly.
"""
from .api import (  # noqa: F401
    LercError,
    build_info,
    computeCompressedSize,
    decode,
    decode_device,
    decode_raster_tiles_device_depth_strided,
    decode_raster_tiles_device_nodata,
    decode_raster_window_device_depth,
    decode_raster_window_device_nodata,
    encode,
    encode_device,
    encode_raster_tile_range_device_depth,
    encode_raster_tiles_device_depth_strided,
    encode_raster_tiles_device_nodata,
    getLercBlobInfo,
    getLercDataRanges,
    library_path,
    load_library,
)

__all__ = ["encode", "decode", "computeCompressedSize", "getLercBlobInfo", "getLercDataRanges", "encode_device",
           "decode_device", "load_library", "library_path", "build_info", "LercError", "encode_raster_tiles_device_depth_strided",
           "decode_raster_tiles_device_depth_strided", "encode_raster_tile_range_device_depth", "decode_raster_window_device_depth",
           "encode_raster_tiles_device_nodata", "decode_raster_window_device_nodata", "decode_raster_tiles_device_nodata"]
