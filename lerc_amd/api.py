"""ctypes binding of liblerc_amd.so (see include/lerc_amd.h).

Host-pointer functions follow the reference wrapper OtherLanguages/Python/lerc/_lerc.py:
  encode(npArr, nValuesPerPixel, bHasMask, npValidMask, maxZErr, nBytesHint)  (_lerc.py:333-470)
      -> (result, nBytesWritten, npBuffer)       nBytesHint == 0: size query -> (result, nBytesNeeded)
  decode(lercBlob)                                                               (_lerc.py:610-700)
      -> (result, npArr, npValidMask)
  getLercBlobInfo(lercBlob)                                                      (_lerc.py:520-560)
      -> (result, codecVersion, dataType, nValuesPerPixel, nCols, nRows, nBands, nValidPixels, blobSize, nMasks,
          zMin, zMax, maxZErrUsed, nUsesNoData)
  getLercDataRanges(lercBlob, nValuesPerPixel, nBands) -> (result, npMins, npMaxs)  (_lerc.py:565-600)
Array layout as in the reference: [nBands,] nRows, nCols [, nValuesPerPixel].
"""
import ctypes as ct
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

_DT_NP = [np.int8, np.uint8, np.int16, np.uint16, np.int32, np.uint32, np.float32, np.float64]


class LercError(RuntimeError):
    pass


def library_path():
    # LERC_AMD_LIBRARY: another build of the same HIP sources (e.g. csrc/_probe/liblerc_amd_probe.so, the tuning build)
    return os.environ.get("LERC_AMD_LIBRARY") or os.path.join(_HERE, "csrc", "liblerc_amd.so")


def load_library():
    """Loads the HIP library; raises (never falls back) when it is missing."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = library_path()
    if not os.path.exists(path):
        raise LercError(f"{path} not built -- run `python -c 'import __graft_entry__ as g; g.build()'` "
                        "(there is no CPU fallback)")
    lib = ct.CDLL(path, mode=ct.RTLD_LOCAL)
    u32p, dblp = ct.POINTER(ct.c_uint), ct.POINTER(ct.c_double)
    enc = [ct.c_void_p, ct.c_uint, ct.c_int, ct.c_int, ct.c_int, ct.c_int, ct.c_int, ct.c_void_p, ct.c_double]
    lib.lerc_computeCompressedSize.argtypes = enc + [u32p]
    lib.lerc_encode.argtypes = enc + [ct.c_void_p, ct.c_uint, u32p]
    lib.lerc_getBlobInfo.argtypes = [ct.c_void_p, ct.c_uint, u32p, dblp, ct.c_int, ct.c_int]
    lib.lerc_getDataRanges.argtypes = [ct.c_void_p, ct.c_uint, ct.c_int, ct.c_int, dblp, dblp]
    lib.lerc_decode.argtypes = [ct.c_void_p, ct.c_uint, ct.c_int, ct.c_void_p, ct.c_int, ct.c_int, ct.c_int, ct.c_int,
                                ct.c_uint, ct.c_void_p]
    lib.lerc_amd_create.argtypes = [ct.c_void_p]
    lib.lerc_amd_create.restype = ct.c_void_p
    lib.lerc_amd_destroy.argtypes = [ct.c_void_p]
    lib.lerc_amd_set_stream.argtypes = [ct.c_void_p, ct.c_void_p]
    lib.lerc_amd_last_error.argtypes = [ct.c_void_p]
    lib.lerc_amd_last_error.restype = ct.c_char_p
    lib.lerc_amd_encode_device.argtypes = [ct.c_void_p] + enc + [ct.c_void_p, ct.c_uint, u32p]
    lib.lerc_amd_decode_device.argtypes = [ct.c_void_p, ct.c_void_p, ct.c_uint, ct.c_int, ct.c_void_p, ct.c_int, ct.c_int,
                                           ct.c_int, ct.c_int, ct.c_uint, ct.c_void_p]
    lib.lerc_amd_encode_tiles_device.argtypes = [ct.c_void_p, ct.c_void_p, ct.c_uint, ct.c_int, ct.c_int, ct.c_int, ct.c_double, ct.c_void_p,
                                                 ct.c_ulonglong, ct.c_void_p, ct.c_void_p, ct.POINTER(ct.c_ulonglong)]
    lib.lerc_amd_decode_tiles_device.argtypes = [ct.c_void_p, ct.c_void_p, ct.c_void_p, ct.c_void_p, ct.c_int, ct.c_int, ct.c_int, ct.c_uint,
                                                 ct.c_void_p]
    lib.lerc_amd_encode_tiles_device_slots.argtypes = [ct.c_void_p, ct.c_void_p, ct.c_uint, ct.c_int, ct.c_int, ct.c_int, ct.c_double, ct.c_void_p,
                                                       ct.c_ulonglong, ct.c_void_p]
    lib.lerc_amd_decode_tiles_device_slots.argtypes = [ct.c_void_p, ct.c_void_p, ct.c_ulonglong, ct.c_void_p, ct.c_int, ct.c_int, ct.c_int, ct.c_uint,
                                                       ct.c_void_p]
    lib.lerc_amd_build_info.restype = ct.c_char_p
    lib.lerc_amd_encode_tiles_device_masked.argtypes = [ct.c_void_p, ct.c_void_p, ct.c_uint, ct.c_int, ct.c_int, ct.c_int, ct.c_void_p, ct.c_double,
                                                        ct.c_void_p, ct.c_ulonglong, ct.c_ulonglong, ct.c_void_p, ct.c_void_p, ct.c_void_p]
    lib.lerc_amd_decode_tiles_device_masked.argtypes = [ct.c_void_p, ct.c_void_p, ct.c_void_p, ct.c_void_p, ct.c_int, ct.c_int, ct.c_int, ct.c_uint,
                                                        ct.c_void_p, ct.c_void_p]
    # (only a library named by LERC_AMD_LIBRARY may lack the band stack calls -- tools time against one built before them; the
    # package's own library without them fails here, at load)
    have_bands = not os.environ.get("LERC_AMD_LIBRARY") or hasattr(lib, "lerc_amd_encode_tiles_device_bands")
    if have_bands:
        lib.lerc_amd_encode_tiles_device_bands.argtypes = [ct.c_void_p, ct.c_void_p, ct.c_uint, ct.c_int, ct.c_int, ct.c_int, ct.c_int, ct.c_int,
                                                           ct.c_void_p, ct.c_double, ct.c_void_p, ct.c_ulonglong, ct.c_ulonglong, ct.c_void_p,
                                                           ct.c_void_p, ct.c_void_p]
        lib.lerc_amd_decode_tiles_device_bands.argtypes = [ct.c_void_p, ct.c_void_p, ct.c_void_p, ct.c_void_p, ct.c_int, ct.c_int, ct.c_int, ct.c_int,
                                                           ct.c_uint, ct.c_void_p, ct.c_int, ct.c_void_p]
    # (the raster tile calls: the same rule)
    have_raster = not os.environ.get("LERC_AMD_LIBRARY") or hasattr(lib, "lerc_amd_encode_raster_tiles_device")
    if have_raster:
        lib.lerc_amd_encode_raster_tiles_device.argtypes = [ct.c_void_p, ct.c_void_p, ct.c_uint, ct.c_int, ct.c_int, ct.c_int, ct.c_ulonglong,
                                                            ct.c_ulonglong, ct.c_int, ct.c_int, ct.c_int, ct.c_void_p, ct.c_ulonglong, ct.c_double,
                                                            ct.c_void_p, ct.c_ulonglong, ct.c_ulonglong, ct.c_void_p, ct.c_void_p, ct.c_void_p]
        lib.lerc_amd_decode_raster_tiles_device.argtypes = [ct.c_void_p, ct.c_void_p, ct.c_void_p, ct.c_void_p, ct.c_uint, ct.c_int, ct.c_int, ct.c_int,
                                                            ct.c_ulonglong, ct.c_ulonglong, ct.c_int, ct.c_int, ct.c_void_p, ct.c_int, ct.c_void_p,
                                                            ct.c_ulonglong]
        lib.lerc_amd_raster_tiles_counters.argtypes = [ct.c_void_p, ct.POINTER(ct.c_ulonglong)]
        lib.lerc_amd_raster_tiles_counters.restype = None
    # (the strided raster tile calls: the same rule)
    have_strided = not os.environ.get("LERC_AMD_LIBRARY") or hasattr(lib, "lerc_amd_encode_raster_tiles_device_strided")
    if have_strided:
        lib.lerc_amd_encode_raster_tiles_device_strided.argtypes = [ct.c_void_p, ct.c_void_p, ct.c_uint, ct.c_int, ct.c_int, ct.c_int,
                                                                    ct.c_ulonglong, ct.c_ulonglong, ct.c_ulonglong, ct.c_int, ct.c_int, ct.c_int,
                                                                    ct.c_void_p, ct.c_ulonglong, ct.c_double, ct.c_void_p, ct.c_ulonglong,
                                                                    ct.c_ulonglong, ct.c_void_p, ct.c_void_p, ct.c_void_p]
        lib.lerc_amd_decode_raster_tiles_device_strided.argtypes = [ct.c_void_p, ct.c_void_p, ct.c_void_p, ct.c_void_p, ct.c_uint, ct.c_int,
                                                                    ct.c_int, ct.c_int, ct.c_ulonglong, ct.c_ulonglong, ct.c_ulonglong, ct.c_int,
                                                                    ct.c_int, ct.c_void_p, ct.c_int, ct.c_void_p, ct.c_ulonglong]
    # (the tile range and window calls: the same rule)
    have_window = not os.environ.get("LERC_AMD_LIBRARY") or hasattr(lib, "lerc_amd_decode_raster_window_device")
    if have_window:
        lib.lerc_amd_encode_raster_tiles_device_range.argtypes = [ct.c_void_p, ct.c_void_p, ct.c_uint, ct.c_int, ct.c_int, ct.c_int,
                                                                  ct.c_ulonglong, ct.c_ulonglong, ct.c_ulonglong, ct.c_int, ct.c_int, ct.c_int,
                                                                  ct.c_int, ct.c_int, ct.c_int, ct.c_int, ct.c_void_p, ct.c_ulonglong, ct.c_double,
                                                                  ct.c_void_p, ct.c_ulonglong, ct.c_ulonglong, ct.c_void_p, ct.c_void_p, ct.c_void_p]
        lib.lerc_amd_decode_raster_window_device.argtypes = [ct.c_void_p, ct.c_void_p, ct.c_void_p, ct.c_void_p, ct.c_uint, ct.c_int, ct.c_int,
                                                             ct.c_int, ct.c_int, ct.c_int, ct.c_int, ct.c_int, ct.c_int, ct.c_int, ct.c_void_p,
                                                             ct.c_ulonglong, ct.c_ulonglong, ct.c_ulonglong, ct.c_int, ct.c_void_p, ct.c_ulonglong]
    # (the depth tile calls, include/lerc_amd_depth.h: the same rule)
    have_depth = not os.environ.get("LERC_AMD_LIBRARY") or hasattr(lib, "lerc_amd_encode_tiles_device_depth")
    if have_depth:
        lib.lerc_amd_encode_tiles_device_depth.argtypes = [ct.c_void_p, ct.c_void_p, ct.c_uint, ct.c_int, ct.c_int, ct.c_int, ct.c_int, ct.c_void_p,
                                                           ct.c_double, ct.c_void_p, ct.c_ulonglong, ct.c_ulonglong, ct.c_void_p, ct.c_void_p,
                                                           ct.c_void_p]
        lib.lerc_amd_decode_tiles_device_depth.argtypes = [ct.c_void_p, ct.c_void_p, ct.c_void_p, ct.c_void_p, ct.c_int, ct.c_int, ct.c_int, ct.c_int,
                                                           ct.c_uint, ct.c_void_p, ct.c_void_p]
        lib.lerc_amd_encode_raster_tiles_device_depth.argtypes = [ct.c_void_p, ct.c_void_p, ct.c_uint, ct.c_int, ct.c_int, ct.c_int, ct.c_ulonglong,
                                                                  ct.c_ulonglong, ct.c_int, ct.c_int, ct.c_int, ct.c_void_p, ct.c_ulonglong, ct.c_double,
                                                                  ct.c_void_p, ct.c_ulonglong, ct.c_ulonglong, ct.c_void_p, ct.c_void_p, ct.c_void_p]
        lib.lerc_amd_decode_raster_tiles_device_depth.argtypes = [ct.c_void_p, ct.c_void_p, ct.c_void_p, ct.c_void_p, ct.c_uint, ct.c_int, ct.c_int,
                                                                  ct.c_int, ct.c_ulonglong, ct.c_ulonglong, ct.c_int, ct.c_int, ct.c_void_p, ct.c_int,
                                                                  ct.c_void_p, ct.c_ulonglong]
    # (the depth raster calls that take a layout, a tile range or a window: the same rule)
    have_depth_layouts = not os.environ.get("LERC_AMD_LIBRARY") or hasattr(lib, "lerc_amd_encode_raster_tiles_device_depth_strided")
    if have_depth_layouts:
        lib.lerc_amd_encode_raster_tiles_device_depth_strided.argtypes = [ct.c_void_p, ct.c_void_p, ct.c_uint, ct.c_int, ct.c_int, ct.c_int,
                                                                          ct.c_ulonglong, ct.c_ulonglong, ct.c_ulonglong, ct.c_int, ct.c_int, ct.c_int,
                                                                          ct.c_void_p, ct.c_ulonglong, ct.c_double, ct.c_void_p, ct.c_ulonglong,
                                                                          ct.c_ulonglong, ct.c_void_p, ct.c_void_p, ct.c_void_p]
        lib.lerc_amd_decode_raster_tiles_device_depth_strided.argtypes = [ct.c_void_p, ct.c_void_p, ct.c_void_p, ct.c_void_p, ct.c_uint, ct.c_int,
                                                                          ct.c_int, ct.c_int, ct.c_ulonglong, ct.c_ulonglong, ct.c_ulonglong, ct.c_int,
                                                                          ct.c_int, ct.c_void_p, ct.c_int, ct.c_void_p, ct.c_ulonglong]
        lib.lerc_amd_encode_raster_tiles_device_depth_range.argtypes = [ct.c_void_p, ct.c_void_p, ct.c_uint, ct.c_int, ct.c_int, ct.c_int,
                                                                        ct.c_ulonglong, ct.c_ulonglong, ct.c_ulonglong, ct.c_int, ct.c_int, ct.c_int,
                                                                        ct.c_int, ct.c_int, ct.c_int, ct.c_int, ct.c_void_p, ct.c_ulonglong, ct.c_double,
                                                                        ct.c_void_p, ct.c_ulonglong, ct.c_ulonglong, ct.c_void_p, ct.c_void_p,
                                                                        ct.c_void_p]
        lib.lerc_amd_decode_raster_window_device_depth.argtypes = [ct.c_void_p, ct.c_void_p, ct.c_void_p, ct.c_void_p, ct.c_uint, ct.c_int, ct.c_int,
                                                                   ct.c_int, ct.c_int, ct.c_int, ct.c_int, ct.c_int, ct.c_int, ct.c_int, ct.c_void_p,
                                                                   ct.c_ulonglong, ct.c_ulonglong, ct.c_ulonglong, ct.c_int, ct.c_void_p,
                                                                   ct.c_ulonglong]
    # (the noData raster calls, include/lerc_amd_nodata.h: the same rule)
    have_nodata = not os.environ.get("LERC_AMD_LIBRARY") or hasattr(lib, "lerc_amd_encode_raster_tiles_device_nodata")
    if have_nodata:
        lib.lerc_amd_encode_raster_tiles_device_nodata.argtypes = [ct.c_void_p, ct.c_void_p, ct.c_uint, ct.c_int, ct.c_int, ct.c_ulonglong,
                                                                   ct.c_ulonglong, ct.c_int, ct.c_int, ct.c_int, ct.c_int, ct.c_int, ct.c_int,
                                                                   ct.c_double, ct.c_double, ct.c_void_p, ct.c_ulonglong, ct.c_ulonglong, ct.c_void_p,
                                                                   ct.c_void_p, ct.c_void_p]
        lib.lerc_amd_decode_raster_window_device_nodata.argtypes = [ct.c_void_p, ct.c_void_p, ct.c_void_p, ct.c_void_p, ct.c_uint, ct.c_int, ct.c_int,
                                                                    ct.c_int, ct.c_int, ct.c_int, ct.c_int, ct.c_int, ct.c_int, ct.c_void_p,
                                                                    ct.c_ulonglong, ct.c_ulonglong, ct.c_double, ct.c_void_p, ct.c_ulonglong]
        for n in ("lerc_amd_encode_raster_tiles_device_nodata", "lerc_amd_decode_raster_window_device_nodata"):
            getattr(lib, n).restype = ct.c_uint
    lib.lerc_amd_tile_batch_counters.argtypes = [ct.c_void_p, ct.POINTER(ct.c_ulonglong)]
    lib.lerc_amd_tile_batch_counters.restype = None
    lib.lerc_amd_encode_device_async.argtypes = [ct.c_void_p] + enc + [ct.c_void_p, ct.c_uint, u32p]
    lib.lerc_amd_decode_device_async.argtypes = [ct.c_void_p, ct.c_void_p, ct.c_uint, ct.c_int, ct.c_void_p, ct.c_int, ct.c_int,
                                                 ct.c_int, ct.c_int, ct.c_uint, ct.c_void_p, u32p]
    lib.lerc_amd_finish.argtypes = [ct.c_void_p, ct.c_uint, u32p]
    for n in ("lerc_computeCompressedSize", "lerc_encode", "lerc_getBlobInfo", "lerc_getDataRanges", "lerc_decode",
              "lerc_amd_encode_device", "lerc_amd_decode_device", "lerc_amd_encode_tiles_device", "lerc_amd_decode_tiles_device",
              "lerc_amd_encode_device_async", "lerc_amd_decode_device_async", "lerc_amd_finish", "lerc_amd_encode_tiles_device_slots",
              "lerc_amd_decode_tiles_device_slots", "lerc_amd_encode_tiles_device_masked", "lerc_amd_decode_tiles_device_masked") + \
            (("lerc_amd_encode_tiles_device_bands", "lerc_amd_decode_tiles_device_bands") if have_bands else ()) + \
            (("lerc_amd_encode_raster_tiles_device", "lerc_amd_decode_raster_tiles_device") if have_raster else ()) + \
            (("lerc_amd_encode_raster_tiles_device_strided", "lerc_amd_decode_raster_tiles_device_strided") if have_strided else ()) + \
            (("lerc_amd_encode_raster_tiles_device_range", "lerc_amd_decode_raster_window_device") if have_window else ()) + \
            (("lerc_amd_encode_tiles_device_depth", "lerc_amd_decode_tiles_device_depth", "lerc_amd_encode_raster_tiles_device_depth",
              "lerc_amd_decode_raster_tiles_device_depth") if have_depth else ()) + \
            (("lerc_amd_encode_raster_tiles_device_depth_strided", "lerc_amd_decode_raster_tiles_device_depth_strided",
              "lerc_amd_encode_raster_tiles_device_depth_range", "lerc_amd_decode_raster_window_device_depth") if have_depth_layouts else ()):
        getattr(lib, n).restype = ct.c_uint
    _LIB = lib
    return lib


def build_info():
    return load_library().lerc_amd_build_info().decode()


def _dt_code(dtype):
    dtype = np.dtype(dtype)
    for i, t in enumerate(_DT_NP):
        if np.dtype(t) == dtype:
            return i
    raise LercError(f"unsupported dtype {dtype}")


def _shape(arr, nValuesPerPixel):
    shape = list(arr.shape)
    n_depth = int(nValuesPerPixel)
    if n_depth > 1:
        if shape[-1] != n_depth:
            raise LercError("last axis must be nValuesPerPixel")
        shape = shape[:-1]
    if len(shape) == 2:
        return 1, shape[0], shape[1]
    if len(shape) == 3:
        return shape[0], shape[1], shape[2]
    raise LercError(f"unsupported array shape {arr.shape}")


def _mask_args(bHasMask, npValidMask, n_bands, n_rows, n_cols):
    if not bHasMask or npValidMask is None:
        return 0, None, None
    m = np.ascontiguousarray(npValidMask, dtype=np.uint8)
    n_masks = n_bands if (m.ndim == 3 and n_bands > 1 and m.shape[0] == n_bands) else 1
    if m.size != n_masks * n_rows * n_cols:
        raise LercError("mask shape does not match the raster")
    return n_masks, m.ctypes.data, m


def computeCompressedSize(npArr, nValuesPerPixel, bHasMask, npValidMask, maxZErr):
    lib = load_library()
    a = np.ascontiguousarray(npArr)
    n_bands, n_rows, n_cols = _shape(a, nValuesPerPixel)
    n_masks, mptr, _keep = _mask_args(bHasMask, npValidMask, n_bands, n_rows, n_cols)
    out = ct.c_uint(0)
    rc = lib.lerc_computeCompressedSize(a.ctypes.data, _dt_code(a.dtype), int(nValuesPerPixel), n_cols, n_rows, n_bands,
                                        n_masks, mptr, float(maxZErr), ct.byref(out))
    return rc, out.value


def encode(npArr, nValuesPerPixel, bHasMask, npValidMask, maxZErr, nBytesHint):
    if nBytesHint == 0:
        return computeCompressedSize(npArr, nValuesPerPixel, bHasMask, npValidMask, maxZErr)
    lib = load_library()
    a = np.ascontiguousarray(npArr)
    n_bands, n_rows, n_cols = _shape(a, nValuesPerPixel)
    n_masks, mptr, _keep = _mask_args(bHasMask, npValidMask, n_bands, n_rows, n_cols)
    buf = np.empty(int(nBytesHint), np.uint8)
    written = ct.c_uint(0)
    rc = lib.lerc_encode(a.ctypes.data, _dt_code(a.dtype), int(nValuesPerPixel), n_cols, n_rows, n_bands, n_masks, mptr,
                         float(maxZErr), buf.ctypes.data, int(nBytesHint), ct.byref(written))
    return rc, written.value, buf[:written.value]


def getLercBlobInfo(lercBlob):
    lib = load_library()
    b = np.frombuffer(lercBlob, np.uint8)
    info = (ct.c_uint * 11)()
    rng = (ct.c_double * 3)()
    rc = lib.lerc_getBlobInfo(b.ctypes.data, len(b), info, rng, 11, 3)
    if rc:
        return (rc,) + (0,) * 13
    return (rc, info[0], info[1], info[2], info[3], info[4], info[5], info[6], info[7], info[8], rng[0], rng[1], rng[2], info[10])


def getLercDataRanges(lercBlob, nValuesPerPixel, nBands):
    lib = load_library()
    b = np.frombuffer(lercBlob, np.uint8)
    n = int(nValuesPerPixel) * int(nBands)
    mins = (ct.c_double * n)()
    maxs = (ct.c_double * n)()
    rc = lib.lerc_getDataRanges(b.ctypes.data, len(b), int(nValuesPerPixel), int(nBands), mins, maxs)
    shape = (nBands, nValuesPerPixel)
    return rc, np.array(mins).reshape(shape), np.array(maxs).reshape(shape)


def decode(lercBlob):
    lib = load_library()
    r = getLercBlobInfo(lercBlob)
    if r[0]:
        return r[0], None, None
    _, _, dt, n_depth, n_cols, n_rows, n_bands, _, _, n_masks = r[:10]
    b = np.frombuffer(lercBlob, np.uint8)
    shape = ((n_bands,) if n_bands > 1 else ()) + (n_rows, n_cols) + ((n_depth,) if n_depth > 1 else ())
    out = np.empty(shape, _DT_NP[dt])
    mask = np.empty(((n_masks,) if n_masks > 1 else ()) + (n_rows, n_cols), np.uint8) if n_masks > 0 else None
    rc = lib.lerc_decode(b.ctypes.data, len(b), n_masks, mask.ctypes.data if mask is not None else None, n_depth, n_cols,
                         n_rows, n_bands, dt, out.ctypes.data)
    return rc, out, mask


# ---- device-pointer extension (torch tensors or raw device addresses) --------------------------------
class DeviceCodec:
    """One lerc_amd context bound to a HIP stream (None / 0 = the HIP default stream)."""

    def __init__(self, stream_ptr=None):
        self.lib = load_library()
        self.h = self.lib.lerc_amd_create(ct.c_void_p(stream_ptr) if stream_ptr else None)
        if not self.h:
            raise LercError("lerc_amd_create failed: no usable HIP device (this library has no CPU path)")

    def close(self):
        if self.h:
            self.lib.lerc_amd_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def path_counters(self):
        """[encodes by the streaming kernels, encodes by the general kernels, decodes streaming, decodes general] of this context"""
        out = (ct.c_ulonglong * 4)()
        self.lib.lerc_amd_path_counters.argtypes = [ct.c_void_p, ct.POINTER(ct.c_ulonglong)]
        self.lib.lerc_amd_path_counters.restype = None
        self.lib.lerc_amd_path_counters(self.h, out)
        return list(out)

    def decode_forms(self):
        """bands / tiles of this context decoded by [-, discovery + decode in two launches, the walking one-launch decoder, the scanning decoder]"""
        out = (ct.c_ulonglong * 4)()
        self.lib.lerc_amd_decode_forms.argtypes = [ct.c_void_p, ct.POINTER(ct.c_ulonglong)]
        self.lib.lerc_amd_decode_forms.restype = None
        self.lib.lerc_amd_decode_forms(self.h, out)
        return list(out)

    def decode_refusals(self):
        """attempts thrown away on the way down the tiers: [the decode kernels refused the masked scan's block offsets, the masked scan handed
        a band on, a streaming decode tier handed a band on, -]"""
        out = (ct.c_ulonglong * 4)()
        self.lib.lerc_amd_decode_refusals.argtypes = [ct.c_void_p, ct.POINTER(ct.c_ulonglong)]
        self.lib.lerc_amd_decode_refusals.restype = None
        self.lib.lerc_amd_decode_refusals(self.h, out)
        return list(out)

    def tile_batch_counters(self):
        """tiles of the batch calls of this context: [encoded by the batch's own launches, encoded one by one behind the batch, decoded by
        the batch's launches, decoded one by one]"""
        out = (ct.c_ulonglong * 4)()
        self.lib.lerc_amd_tile_batch_counters(self.h, out)
        return list(out)

    def encode_tiles_masked(self, d_tiles, dt_code, n_cols, n_rows, n_tiles, d_valid, max_z_err, d_arena, arena_cap, slot_bytes=0):
        """raw device addresses -> (status, offsets uint64[nTiles], sizes uint32[nTiles], arena bytes used); d_valid 0 / None: all valid"""
        offsets = np.zeros(n_tiles, np.uint64)
        sizes = np.zeros(n_tiles, np.uint32)
        used = ct.c_ulonglong(0)
        rc = self.lib.lerc_amd_encode_tiles_device_masked(self.h, d_tiles, dt_code, n_cols, n_rows, n_tiles, d_valid or None, float(max_z_err),
                                                          d_arena, int(arena_cap), int(slot_bytes), offsets.ctypes.data, sizes.ctypes.data,
                                                          ct.byref(used))
        return rc, offsets, sizes, int(used.value)

    def decode_tiles_masked(self, d_arena, offsets, sizes, n_tiles, n_cols, n_rows, dt_code, d_tiles, d_valid):
        offsets = np.ascontiguousarray(offsets, np.uint64)
        sizes = np.ascontiguousarray(sizes, np.uint32)
        return self.lib.lerc_amd_decode_tiles_device_masked(self.h, d_arena, offsets.ctypes.data, sizes.ctypes.data, n_tiles, n_cols, n_rows,
                                                            dt_code, d_tiles, d_valid or None)

    def encode_tiles_bands(self, d_tiles, dt_code, n_cols, n_rows, n_bands, n_tiles, n_masks, d_valid, max_z_err, d_arena, arena_cap, slot_bytes=0):
        """band stacks, raw device addresses: d_tiles [nTiles][nBands][nRows][nCols], d_valid [nTiles][nMasks][nRows][nCols] (n_masks 0: None)
        -> (status, offsets uint64[nTiles], sizes uint32[nTiles], arena bytes used), one blob a tile"""
        offsets = np.zeros(n_tiles, np.uint64)
        sizes = np.zeros(n_tiles, np.uint32)
        used = ct.c_ulonglong(0)
        rc = self.lib.lerc_amd_encode_tiles_device_bands(self.h, d_tiles, dt_code, n_cols, n_rows, n_bands, n_tiles, n_masks, d_valid or None,
                                                         float(max_z_err), d_arena, int(arena_cap), int(slot_bytes), offsets.ctypes.data,
                                                         sizes.ctypes.data, ct.byref(used))
        return rc, offsets, sizes, int(used.value)

    def decode_tiles_bands(self, d_arena, offsets, sizes, n_tiles, n_cols, n_rows, n_bands, dt_code, d_tiles, n_masks, d_valid):
        offsets = np.ascontiguousarray(offsets, np.uint64)
        sizes = np.ascontiguousarray(sizes, np.uint32)
        return self.lib.lerc_amd_decode_tiles_device_bands(self.h, d_arena, offsets.ctypes.data, sizes.ctypes.data, n_tiles, n_cols, n_rows,
                                                           n_bands, dt_code, d_tiles, n_masks, d_valid or None)

    def encode_tiles_depth(self, d_tiles, dt_code, n_cols, n_rows, n_depth, n_tiles, d_valid, max_z_err, d_arena, arena_cap, slot_bytes=0):
        """depth tiles, raw device addresses: d_tiles [nTiles][nRows][nCols][nDepth], d_valid [nTiles][nRows][nCols] or 0 / None
        -> (status, offsets uint64[nTiles], sizes uint32[nTiles], arena bytes used), one blob with the header's nDepth a tile"""
        offsets = np.zeros(n_tiles, np.uint64)
        sizes = np.zeros(n_tiles, np.uint32)
        used = ct.c_ulonglong(0)
        rc = self.lib.lerc_amd_encode_tiles_device_depth(self.h, d_tiles, dt_code, n_cols, n_rows, n_depth, n_tiles, d_valid or None, float(max_z_err),
                                                         d_arena, int(arena_cap), int(slot_bytes), offsets.ctypes.data, sizes.ctypes.data,
                                                         ct.byref(used))
        return rc, offsets, sizes, int(used.value)

    def decode_tiles_depth(self, d_arena, offsets, sizes, n_tiles, n_cols, n_rows, n_depth, dt_code, d_tiles, d_valid):
        offsets = np.ascontiguousarray(offsets, np.uint64)
        sizes = np.ascontiguousarray(sizes, np.uint32)
        return self.lib.lerc_amd_decode_tiles_device_depth(self.h, d_arena, offsets.ctypes.data, sizes.ctypes.data, n_tiles, n_cols, n_rows, n_depth,
                                                           dt_code, d_tiles, d_valid or None)

    def encode_raster_tiles_depth(self, d_raster, dt_code, n_cols, n_rows, n_depth, pixel_pitch, row_pitch, tile, d_valid, mask_row_pitch, max_z_err,
                                  d_arena, arena_cap, slot_bytes=0):
        """a raster of packed pixels of n_depth elements (pixel_pitch must equal n_depth; the library's check decides: status 2), coded as
        depth tiles in the order of raster_tile_grid -> (status, offsets, sizes, arena bytes used)"""
        n_tiles = len(raster_tile_grid(n_rows, n_cols, tile))
        offsets = np.zeros(n_tiles, np.uint64)
        sizes = np.zeros(n_tiles, np.uint32)
        used = ct.c_ulonglong(0)
        rc = self.lib.lerc_amd_encode_raster_tiles_device_depth(self.h, d_raster, dt_code, n_cols, n_rows, n_depth, int(pixel_pitch), int(row_pitch),
                                                                int(tile[1]), int(tile[0]), 1 if d_valid else 0, d_valid or None, int(mask_row_pitch),
                                                                float(max_z_err), d_arena, int(arena_cap), int(slot_bytes), offsets.ctypes.data,
                                                                sizes.ctypes.data, ct.byref(used))
        return rc, offsets, sizes, int(used.value)

    def decode_raster_tiles_depth(self, d_arena, offsets, sizes, dt_code, n_cols, n_rows, n_depth, pixel_pitch, row_pitch, tile, d_raster, d_valid,
                                  mask_row_pitch):
        offsets = np.ascontiguousarray(offsets, np.uint64)
        sizes = np.ascontiguousarray(sizes, np.uint32)
        assert len(offsets) == len(sizes) == len(raster_tile_grid(n_rows, n_cols, tile))
        return self.lib.lerc_amd_decode_raster_tiles_device_depth(self.h, d_arena, offsets.ctypes.data, sizes.ctypes.data, dt_code, n_cols, n_rows,
                                                                  n_depth, int(pixel_pitch), int(row_pitch), int(tile[1]), int(tile[0]), d_raster,
                                                                  1 if d_valid else 0, d_valid or None, int(mask_row_pitch))

    def encode_raster_tiles_depth_strided(self, d_raster, dt_code, n_cols, n_rows, n_depth, pixel_pitch, row_pitch, depth_pitch, tile, d_valid,
                                          mask_row_pitch, max_z_err, d_arena, arena_cap, slot_bytes=0, tile_range=None):
        """encode_raster_tiles_depth for a depth raster in any of the layouts of include/lerc_amd_depth.h: element (i, j, d) at i * row_pitch
        + j * pixel_pitch + d * depth_pitch -- packed or gapped pixels (depth_pitch 1), planes or lines (pixel_pitch 1); the library's
        check decides (status 2).  tile_range = (tileRow0, tileCol0, nTileRows, nTileCols): those tiles only, the tables full-grid and
        zero outside the range"""
        n_tiles = len(raster_tile_grid(n_rows, n_cols, tile))
        offsets = np.zeros(n_tiles, np.uint64)
        sizes = np.zeros(n_tiles, np.uint32)
        used = ct.c_ulonglong(0)
        head = (self.h, d_raster, dt_code, n_cols, n_rows, n_depth, int(pixel_pitch), int(row_pitch), int(depth_pitch), int(tile[1]), int(tile[0]))
        tail = (1 if d_valid else 0, d_valid or None, int(mask_row_pitch), float(max_z_err), d_arena, int(arena_cap), int(slot_bytes),
                offsets.ctypes.data, sizes.ctypes.data, ct.byref(used))
        if tile_range is None:
            rc = self.lib.lerc_amd_encode_raster_tiles_device_depth_strided(*head, *tail)
        else:
            rc = self.lib.lerc_amd_encode_raster_tiles_device_depth_range(*head, int(tile_range[1]), int(tile_range[0]), int(tile_range[3]),
                                                                          int(tile_range[2]), *tail)
        return rc, offsets, sizes, int(used.value)

    def encode_raster_tiles_depth_range(self, d_raster, dt_code, n_cols, n_rows, n_depth, pixel_pitch, row_pitch, depth_pitch, tile, tile_range,
                                        d_valid, mask_row_pitch, max_z_err, d_arena, arena_cap, slot_bytes=0):
        return self.encode_raster_tiles_depth_strided(d_raster, dt_code, n_cols, n_rows, n_depth, pixel_pitch, row_pitch, depth_pitch, tile, d_valid,
                                                      mask_row_pitch, max_z_err, d_arena, arena_cap, slot_bytes, tile_range=tile_range)

    def decode_raster_tiles_depth_strided(self, d_arena, offsets, sizes, dt_code, n_cols, n_rows, n_depth, pixel_pitch, row_pitch, depth_pitch, tile,
                                          d_raster, d_valid, mask_row_pitch):
        offsets = np.ascontiguousarray(offsets, np.uint64)
        sizes = np.ascontiguousarray(sizes, np.uint32)
        assert len(offsets) == len(sizes) == len(raster_tile_grid(n_rows, n_cols, tile))
        return self.lib.lerc_amd_decode_raster_tiles_device_depth_strided(self.h, d_arena, offsets.ctypes.data, sizes.ctypes.data, dt_code, n_cols,
                                                                          n_rows, n_depth, int(pixel_pitch), int(row_pitch), int(depth_pitch),
                                                                          int(tile[1]), int(tile[0]), d_raster, 1 if d_valid else 0, d_valid or None,
                                                                          int(mask_row_pitch))

    def decode_raster_window_depth(self, d_arena, offsets, sizes, dt_code, n_cols, n_rows, n_depth, tile, window_rect, d_window, pixel_pitch,
                                   row_pitch, depth_pitch, d_valid, mask_row_pitch):
        """window_rect = (row0, col0, rows, cols) of the depth mosaic n_rows x n_cols x n_depth into the buffer at d_window, which holds the
        window only, in any of the layouts; offsets / sizes: the full grid's tables, read at the window's tiles (raster_window_tiles)"""
        offsets = np.ascontiguousarray(offsets, np.uint64)
        sizes = np.ascontiguousarray(sizes, np.uint32)
        assert len(offsets) == len(sizes) == len(raster_tile_grid(n_rows, n_cols, tile))
        return self.lib.lerc_amd_decode_raster_window_device_depth(self.h, d_arena, offsets.ctypes.data, sizes.ctypes.data, dt_code, n_cols, n_rows,
                                                                   n_depth, int(tile[1]), int(tile[0]), int(window_rect[1]), int(window_rect[0]),
                                                                   int(window_rect[3]), int(window_rect[2]), d_window, int(pixel_pitch),
                                                                   int(row_pitch), int(depth_pitch), 1 if d_valid else 0, d_valid or None,
                                                                   int(mask_row_pitch))

    def raster_tiles_counters(self):
        """tiles of the raster tile calls of this context: [cut through the staging buffer, encoded where they lie, pasted from the staging
        buffer, decoded where they lie]"""
        out = (ct.c_ulonglong * 4)()
        self.lib.lerc_amd_raster_tiles_counters(self.h, out)
        return list(out)

    def encode_raster_tiles(self, d_raster, dt_code, n_cols, n_rows, n_bands, row_pitch, band_pitch, tile, d_valid, mask_row_pitch, max_z_err,
                            d_arena, arena_cap, slot_bytes=0):
        """a pitched raster, raw device addresses, pitches in elements; tile: (tileRows, tileCols); d_valid 0 / None: no mask
        -> (status, offsets uint64[nTiles], sizes uint32[nTiles], arena bytes used), tiles in the order of raster_tile_grid"""
        n_tiles = len(raster_tile_grid(n_rows, n_cols, tile))
        offsets = np.zeros(n_tiles, np.uint64)
        sizes = np.zeros(n_tiles, np.uint32)
        used = ct.c_ulonglong(0)
        rc = self.lib.lerc_amd_encode_raster_tiles_device(self.h, d_raster, dt_code, n_cols, n_rows, n_bands, int(row_pitch), int(band_pitch),
                                                          int(tile[1]), int(tile[0]), 1 if d_valid else 0, d_valid or None, int(mask_row_pitch),
                                                          float(max_z_err), d_arena, int(arena_cap), int(slot_bytes), offsets.ctypes.data,
                                                          sizes.ctypes.data, ct.byref(used))
        return rc, offsets, sizes, int(used.value)

    def decode_raster_tiles(self, d_arena, offsets, sizes, dt_code, n_cols, n_rows, n_bands, row_pitch, band_pitch, tile, d_raster, d_valid,
                            mask_row_pitch):
        offsets = np.ascontiguousarray(offsets, np.uint64)
        sizes = np.ascontiguousarray(sizes, np.uint32)
        assert len(offsets) == len(sizes) == len(raster_tile_grid(n_rows, n_cols, tile))
        return self.lib.lerc_amd_decode_raster_tiles_device(self.h, d_arena, offsets.ctypes.data, sizes.ctypes.data, dt_code, n_cols, n_rows, n_bands,
                                                            int(row_pitch), int(band_pitch), int(tile[1]), int(tile[0]), d_raster,
                                                            1 if d_valid else 0, d_valid or None, int(mask_row_pitch))

    def encode_raster_tiles_strided(self, d_raster, dt_code, n_cols, n_rows, n_bands, pixel_pitch, row_pitch, band_pitch, tile, d_valid,
                                    mask_row_pitch, max_z_err, d_arena, arena_cap, slot_bytes=0):
        """encode_raster_tiles with a pixel pitch: element (b, i, j) at b * band_pitch + i * row_pitch + j * pixel_pitch -- pixel-interleaved
        (pixel_pitch >= 2, band_pitch 1) and line-interleaved rasters; the library's check decides (status 2)"""
        n_tiles = len(raster_tile_grid(n_rows, n_cols, tile))
        offsets = np.zeros(n_tiles, np.uint64)
        sizes = np.zeros(n_tiles, np.uint32)
        used = ct.c_ulonglong(0)
        rc = self.lib.lerc_amd_encode_raster_tiles_device_strided(self.h, d_raster, dt_code, n_cols, n_rows, n_bands, int(pixel_pitch),
                                                                  int(row_pitch), int(band_pitch), int(tile[1]), int(tile[0]), 1 if d_valid else 0,
                                                                  d_valid or None, int(mask_row_pitch), float(max_z_err), d_arena, int(arena_cap),
                                                                  int(slot_bytes), offsets.ctypes.data, sizes.ctypes.data, ct.byref(used))
        return rc, offsets, sizes, int(used.value)

    def decode_raster_tiles_strided(self, d_arena, offsets, sizes, dt_code, n_cols, n_rows, n_bands, pixel_pitch, row_pitch, band_pitch, tile,
                                    d_raster, d_valid, mask_row_pitch):
        offsets = np.ascontiguousarray(offsets, np.uint64)
        sizes = np.ascontiguousarray(sizes, np.uint32)
        assert len(offsets) == len(sizes) == len(raster_tile_grid(n_rows, n_cols, tile))
        return self.lib.lerc_amd_decode_raster_tiles_device_strided(self.h, d_arena, offsets.ctypes.data, sizes.ctypes.data, dt_code, n_cols, n_rows,
                                                                    n_bands, int(pixel_pitch), int(row_pitch), int(band_pitch), int(tile[1]),
                                                                    int(tile[0]), d_raster, 1 if d_valid else 0, d_valid or None,
                                                                    int(mask_row_pitch))

    def encode_raster_tiles_range(self, d_raster, dt_code, n_cols, n_rows, n_bands, pixel_pitch, row_pitch, band_pitch, tile, tile_range,
                                  d_valid, mask_row_pitch, max_z_err, d_arena, arena_cap, slot_bytes=0):
        """encode_raster_tiles_strided for the tiles of tile_range = (tileRow0, tileCol0, nTileRows, nTileCols) only: offsets / sizes are
        the full grid's tables, zero outside the range; offsets are relative to d_arena, arena bytes used count the range only"""
        n_tiles = len(raster_tile_grid(n_rows, n_cols, tile))
        offsets = np.zeros(n_tiles, np.uint64)
        sizes = np.zeros(n_tiles, np.uint32)
        used = ct.c_ulonglong(0)
        rc = self.lib.lerc_amd_encode_raster_tiles_device_range(self.h, d_raster, dt_code, n_cols, n_rows, n_bands, int(pixel_pitch),
                                                                int(row_pitch), int(band_pitch), int(tile[1]), int(tile[0]), int(tile_range[1]),
                                                                int(tile_range[0]), int(tile_range[3]), int(tile_range[2]), 1 if d_valid else 0,
                                                                d_valid or None, int(mask_row_pitch), float(max_z_err), d_arena, int(arena_cap),
                                                                int(slot_bytes), offsets.ctypes.data, sizes.ctypes.data, ct.byref(used))
        return rc, offsets, sizes, int(used.value)

    def decode_raster_window(self, d_arena, offsets, sizes, dt_code, n_cols, n_rows, n_bands, tile, window_rect, d_window, pixel_pitch,
                             row_pitch, band_pitch, d_valid, mask_row_pitch):
        """window_rect = (row0, col0, rows, cols) of the mosaic n_rows x n_cols into the buffer at d_window, which holds the window only;
        offsets / sizes: the full grid's tables, read at the window's tiles (raster_window_tiles)"""
        offsets = np.ascontiguousarray(offsets, np.uint64)
        sizes = np.ascontiguousarray(sizes, np.uint32)
        assert len(offsets) == len(sizes) == len(raster_tile_grid(n_rows, n_cols, tile))
        return self.lib.lerc_amd_decode_raster_window_device(self.h, d_arena, offsets.ctypes.data, sizes.ctypes.data, dt_code, n_cols, n_rows,
                                                             n_bands, int(tile[1]), int(tile[0]), int(window_rect[1]), int(window_rect[0]),
                                                             int(window_rect[3]), int(window_rect[2]), d_window, int(pixel_pitch),
                                                             int(row_pitch), int(band_pitch), 1 if d_valid else 0, d_valid or None,
                                                             int(mask_row_pitch))

    def encode_raster_tiles_nodata(self, d_raster, dt_code, n_cols, n_rows, pixel_pitch, row_pitch, tile, tile_range, no_data, max_z_err, d_arena,
                                   arena_cap, slot_bytes=0):
        """one band whose validity is the value no_data (include/lerc_amd_nodata.h); tile_range = (tileRow0, tileCol0, nTileRows, nTileCols),
        (0, 0, -1, -1): the whole grid; offsets / sizes are the full grid's tables, zero outside the range"""
        n_tiles = len(raster_tile_grid(n_rows, n_cols, tile))
        offsets = np.zeros(n_tiles, np.uint64)
        sizes = np.zeros(n_tiles, np.uint32)
        used = ct.c_ulonglong(0)
        rc = self.lib.lerc_amd_encode_raster_tiles_device_nodata(self.h, d_raster, dt_code, n_cols, n_rows, int(pixel_pitch), int(row_pitch),
                                                                 int(tile[1]), int(tile[0]), int(tile_range[1]), int(tile_range[0]),
                                                                 int(tile_range[3]), int(tile_range[2]), float(no_data), float(max_z_err), d_arena,
                                                                 int(arena_cap), int(slot_bytes), offsets.ctypes.data, sizes.ctypes.data,
                                                                 ct.byref(used))
        return rc, offsets, sizes, int(used.value)

    def decode_raster_window_nodata(self, d_arena, offsets, sizes, dt_code, n_cols, n_rows, tile, window_rect, d_window, pixel_pitch, row_pitch,
                                    no_data, d_valid, mask_row_pitch):
        """decode_raster_window for one band with no_data written at invalid pixels; d_valid: the window's valid bytes, or 0 for none"""
        offsets = np.ascontiguousarray(offsets, np.uint64)
        sizes = np.ascontiguousarray(sizes, np.uint32)
        assert len(offsets) == len(sizes) == len(raster_tile_grid(n_rows, n_cols, tile))
        return self.lib.lerc_amd_decode_raster_window_device_nodata(self.h, d_arena, offsets.ctypes.data, sizes.ctypes.data, dt_code, n_cols,
                                                                    n_rows, int(tile[1]), int(tile[0]), int(window_rect[1]), int(window_rect[0]),
                                                                    int(window_rect[3]), int(window_rect[2]), d_window, int(pixel_pitch),
                                                                    int(row_pitch), float(no_data), d_valid or None, int(mask_row_pitch))

    def raster_tile_grid(self, n_rows, n_cols, tile):
        return raster_tile_grid(n_rows, n_cols, tile)

    def last_note(self):
        """why the last call that left the streaming kernels (or went down a streaming tier) did so; "" if none did"""
        self.lib.lerc_amd_last_note.argtypes = [ct.c_void_p]
        self.lib.lerc_amd_last_note.restype = ct.c_char_p
        return self.lib.lerc_amd_last_note(self.h).decode()

    def last_error(self):
        return self.lib.lerc_amd_last_error(self.h).decode()

    def encode(self, d_data, dt_code, n_depth, n_cols, n_rows, n_bands, max_z_err, d_out, out_cap, d_mask=0, n_masks=0):
        written = ct.c_uint(0)
        rc = self.lib.lerc_amd_encode_device(self.h, d_data, dt_code, n_depth, n_cols, n_rows, n_bands, n_masks,
                                             d_mask or None, float(max_z_err), d_out or None, out_cap, ct.byref(written))
        return rc, written.value

    def encode_async(self, d_data, dt_code, n_depth, n_cols, n_rows, n_bands, max_z_err, d_out, out_cap, d_mask=0, n_masks=0):
        """-> (status, ticket): enqueued on the context's stream; finish(ticket) waits and returns (status, nBytes)"""
        ticket = ct.c_uint(0)
        rc = self.lib.lerc_amd_encode_device_async(self.h, d_data, dt_code, n_depth, n_cols, n_rows, n_bands, n_masks,
                                                   d_mask or None, float(max_z_err), d_out or None, out_cap, ct.byref(ticket))
        return rc, ticket.value

    def decode_async(self, d_blob, size_bound, dt_code, n_depth, n_cols, n_rows, n_bands, d_out, d_mask=0, n_masks=0):
        ticket = ct.c_uint(0)
        rc = self.lib.lerc_amd_decode_device_async(self.h, d_blob, size_bound, n_masks, d_mask or None, n_depth, n_cols, n_rows,
                                                   n_bands, dt_code, d_out, ct.byref(ticket))
        return rc, ticket.value

    def finish(self, ticket=0):
        n = ct.c_uint(0)
        rc = self.lib.lerc_amd_finish(self.h, int(ticket), ct.byref(n))
        return rc, n.value

    def decode(self, d_blob, blob_size, dt_code, n_depth, n_cols, n_rows, n_bands, d_out, d_mask=0, n_masks=0):
        return self.lib.lerc_amd_decode_device(self.h, d_blob, blob_size, n_masks, d_mask or None, n_depth, n_cols, n_rows,
                                               n_bands, dt_code, d_out)


_TORCH_DT = None


def _torch_dt_code(t):
    import torch
    global _TORCH_DT
    if _TORCH_DT is None:
        _TORCH_DT = {torch.int8: 0, torch.uint8: 1, torch.int16: 2, torch.int32: 4, torch.float32: 6, torch.float64: 7}
        if hasattr(torch, "uint16"):
            _TORCH_DT[torch.uint16] = 3
        if hasattr(torch, "uint32"):
            _TORCH_DT[torch.uint32] = 5
    return _TORCH_DT[t.dtype]


def encode_device(codec, tensor, max_z_err, out, n_depth=1):
    """tensor: CUDA(HIP) tensor [nRows, nCols] (or [nRows, nCols, nDepth]); out: uint8 CUDA tensor.  -> (status, nBytes)"""
    n_rows, n_cols = int(tensor.shape[0]), int(tensor.shape[1])
    return codec.encode(tensor.data_ptr(), _torch_dt_code(tensor), n_depth, n_cols, n_rows, 1, max_z_err, out.data_ptr(), out.numel())


def decode_device(codec, blob, n_bytes, out, n_depth=1):
    n_rows, n_cols = int(out.shape[0]), int(out.shape[1])
    return codec.decode(blob.data_ptr(), int(n_bytes), _torch_dt_code(out), n_depth, n_cols, n_rows, 1, out.data_ptr())


def encode_device_async(codec, tensor, max_z_err, out, n_depth=1):
    """Like encode_device, without the wait -> (status, ticket); codec.finish(ticket) -> (status, nBytes)."""
    n_rows, n_cols = int(tensor.shape[0]), int(tensor.shape[1])
    return codec.encode_async(tensor.data_ptr(), _torch_dt_code(tensor), n_depth, n_cols, n_rows, 1, max_z_err, out.data_ptr(), out.numel())


def decode_device_async(codec, blob, size_bound, out, n_depth=1):
    """Like decode_device, without the wait; size_bound: the blob's size or the capacity of its buffer."""
    n_rows, n_cols = int(out.shape[0]), int(out.shape[1])
    return codec.decode_async(blob.data_ptr(), int(size_bound), _torch_dt_code(out), n_depth, n_cols, n_rows, 1, out.data_ptr())


def encode_tiles_device(codec, tiles, max_z_err, arena):
    """tiles: CUDA(HIP) tensor [nTiles, nRows, nCols]; arena: uint8 CUDA tensor.  One blob per tile, each exactly what
    encode() makes of that tile.  -> (status, offsets uint64[nTiles], sizes uint32[nTiles], arena bytes used)"""
    n_tiles, n_rows, n_cols = (int(v) for v in tiles.shape)
    offsets = np.zeros(n_tiles, np.uint64)
    sizes = np.zeros(n_tiles, np.uint32)
    used = ct.c_ulonglong(0)
    rc = codec.lib.lerc_amd_encode_tiles_device(codec.h, tiles.data_ptr(), _torch_dt_code(tiles), n_cols, n_rows, n_tiles, float(max_z_err),
                                                arena.data_ptr(), arena.numel(), offsets.ctypes.data, sizes.ctypes.data, ct.byref(used))
    return rc, offsets, sizes, int(used.value)


def encode_tiles_device_slots(codec, tiles, max_z_err, slots, slot_bytes):
    """The same with a slot per tile: tile t's blob at slots[t * slot_bytes :] (slot_bytes: a multiple of 16), nothing is packed
    afterwards -- the way a caller of lerc_encode() hands every tile a buffer of its own.  -> (status, sizes uint32[nTiles])"""
    n_tiles, n_rows, n_cols = (int(v) for v in tiles.shape)
    assert slots.numel() >= n_tiles * slot_bytes
    sizes = np.zeros(n_tiles, np.uint32)
    rc = codec.lib.lerc_amd_encode_tiles_device_slots(codec.h, tiles.data_ptr(), _torch_dt_code(tiles), n_cols, n_rows, n_tiles, float(max_z_err),
                                                      slots.data_ptr(), int(slot_bytes), sizes.ctypes.data)
    return rc, sizes


def decode_tiles_device_slots(codec, slots, slot_bytes, sizes, out):
    n_tiles, n_rows, n_cols = (int(v) for v in out.shape)
    sizes = np.ascontiguousarray(sizes, np.uint32)
    return codec.lib.lerc_amd_decode_tiles_device_slots(codec.h, slots.data_ptr(), int(slot_bytes), sizes.ctypes.data, n_tiles, n_cols, n_rows,
                                                        _torch_dt_code(out), out.data_ptr())


def decode_tiles_device(codec, arena, offsets, sizes, out):
    """out: CUDA(HIP) tensor [nTiles, nRows, nCols] to fill from the blobs arena[offsets[t] : offsets[t] + sizes[t]]."""
    n_tiles, n_rows, n_cols = (int(v) for v in out.shape)
    offsets = np.ascontiguousarray(offsets, np.uint64)
    sizes = np.ascontiguousarray(sizes, np.uint32)
    return codec.lib.lerc_amd_decode_tiles_device(codec.h, arena.data_ptr(), offsets.ctypes.data, sizes.ctypes.data, n_tiles, n_cols, n_rows,
                                                  _torch_dt_code(out), out.data_ptr())


def encode_tiles_device_masked(codec, tiles, valid, max_z_err, arena, slot_bytes=0):
    """tiles: CUDA(HIP) tensor [nTiles, nRows, nCols]; valid: uint8 CUDA tensor of the same shape (0 = invalid) or None; arena: uint8
    CUDA tensor.  One blob per tile, each exactly what encode() makes of that tile with its mask; slot_bytes != 0 (a multiple of 16):
    tile t's blob at arena[t * slot_bytes :].  -> (status, offsets uint64[nTiles], sizes uint32[nTiles], arena bytes used)"""
    n_tiles, n_rows, n_cols = (int(v) for v in tiles.shape)
    if valid is not None:
        assert tuple(valid.shape) == tuple(tiles.shape) and valid.element_size() == 1 and valid.is_contiguous()
    return codec.encode_tiles_masked(tiles.data_ptr(), _torch_dt_code(tiles), n_cols, n_rows, n_tiles, valid.data_ptr() if valid is not None else 0,
                                     max_z_err, arena.data_ptr(), arena.numel(), slot_bytes)


def decode_tiles_device_masked(codec, arena, offsets, sizes, out, valid_out):
    """out: CUDA(HIP) tensor [nTiles, nRows, nCols]; valid_out: uint8 CUDA tensor of the same shape, written 1 / 0 for every tile (None:
    decode_tiles_device, which refuses blobs with a mask).  A tile whose blob fails is left zeroed, mask too."""
    n_tiles, n_rows, n_cols = (int(v) for v in out.shape)
    return codec.decode_tiles_masked(arena.data_ptr(), offsets, sizes, n_tiles, n_cols, n_rows, _torch_dt_code(out), out.data_ptr(),
                                     valid_out.data_ptr() if valid_out is not None else 0)


def _band_masks(valid, n_tiles, n_bands, n_rows, n_cols):
    """-> (nMasks, device address) of a valid tensor [nTiles, nRows, nCols], [nTiles, 1 | nBands, nRows, nCols] or None"""
    if valid is None:
        return 0, 0
    assert valid.element_size() == 1 and valid.is_contiguous()
    shape = tuple(int(v) for v in valid.shape)
    if shape in ((n_tiles, n_rows, n_cols), (n_tiles, 1, n_rows, n_cols)):
        return 1, valid.data_ptr()
    assert shape == (n_tiles, n_bands, n_rows, n_cols), "valid: a mask a tile or a mask a band"
    return n_bands, valid.data_ptr()


def encode_tiles_device_bands(codec, tiles, valid, max_z_err, arena, slot_bytes=0):
    """tiles: CUDA(HIP) tensor [nTiles, nBands, nRows, nCols]; valid: uint8 CUDA tensor [nTiles, nRows, nCols] (one mask a tile),
    [nTiles, nBands, nRows, nCols] (a mask a band) or None; arena: uint8 CUDA tensor.  One blob per tile, each exactly what encode() makes
    of that band stack.  -> (status, offsets uint64[nTiles], sizes uint32[nTiles], arena bytes used)"""
    n_tiles, n_bands, n_rows, n_cols = (int(v) for v in tiles.shape)
    assert tiles.is_contiguous()
    n_masks, d_valid = _band_masks(valid, n_tiles, n_bands, n_rows, n_cols)
    return codec.encode_tiles_bands(tiles.data_ptr(), _torch_dt_code(tiles), n_cols, n_rows, n_bands, n_tiles, n_masks, d_valid, max_z_err,
                                    arena.data_ptr(), arena.numel(), slot_bytes)


def decode_tiles_device_bands(codec, arena, offsets, sizes, out, valid_out):
    """out: CUDA(HIP) tensor [nTiles, nBands, nRows, nCols]; valid_out as `valid` above, written 1 / 0 for every tile, or None (a blob
    with an invalid pixel is then refused).  A tile whose blob fails is left zeroed, all bands and mask."""
    n_tiles, n_bands, n_rows, n_cols = (int(v) for v in out.shape)
    assert out.is_contiguous()
    n_masks, d_valid = _band_masks(valid_out, n_tiles, n_bands, n_rows, n_cols)
    return codec.decode_tiles_bands(arena.data_ptr(), offsets, sizes, n_tiles, n_cols, n_rows, n_bands, _torch_dt_code(out), out.data_ptr(),
                                    n_masks, d_valid)


def encode_tiles_device_depth(codec, tiles, valid, max_z_err, arena, slot_bytes=0):
    """tiles: CUDA(HIP) tensor [nTiles, nRows, nCols, nDepth]; valid: uint8 CUDA tensor [nTiles, nRows, nCols] (0 = invalid) or None;
    arena: uint8 CUDA tensor.  One blob per tile, each exactly what encode() makes of that tile with nValuesPerPixel = nDepth and its
    mask.  -> (status, offsets uint64[nTiles], sizes uint32[nTiles], arena bytes used)"""
    n_tiles, n_rows, n_cols, n_depth = (int(v) for v in tiles.shape)
    assert tiles.is_contiguous()
    if valid is not None:
        assert tuple(valid.shape) == (n_tiles, n_rows, n_cols) and valid.element_size() == 1 and valid.is_contiguous()
    return codec.encode_tiles_depth(tiles.data_ptr(), _torch_dt_code(tiles), n_cols, n_rows, n_depth, n_tiles, valid.data_ptr() if valid is not None else 0,
                                    max_z_err, arena.data_ptr(), arena.numel(), slot_bytes)


def decode_tiles_device_depth(codec, arena, offsets, sizes, out, valid_out):
    """out: CUDA(HIP) tensor [nTiles, nRows, nCols, nDepth]; valid_out: uint8 CUDA tensor [nTiles, nRows, nCols], written 1 / 0 for every
    tile, or None (a blob with an invalid pixel is then refused).  A tile whose blob fails is left zeroed, mask too."""
    n_tiles, n_rows, n_cols, n_depth = (int(v) for v in out.shape)
    assert out.is_contiguous()
    if valid_out is not None:
        assert tuple(valid_out.shape) == (n_tiles, n_rows, n_cols) and valid_out.element_size() == 1 and valid_out.is_contiguous()
    return codec.decode_tiles_depth(arena.data_ptr(), offsets, sizes, n_tiles, n_cols, n_rows, n_depth, _torch_dt_code(out), out.data_ptr(),
                                    valid_out.data_ptr() if valid_out is not None else 0)


def _raster_depth_view(raster, valid):
    """-> (nRows, nCols, nDepth, pixelPitch, rowPitch, mask address, mask row pitch) of an [H, W, C] tensor or a view of one whose
    channels are contiguous; which pitches are taken is the library's to say (status 2)"""
    assert raster.dim() == 3, "raster: [H, W, C]"
    n_rows, n_cols, n_depth = (int(v) for v in raster.shape)
    assert n_depth == 1 or raster.stride(2) == 1, "raster: contiguous channels"
    pixel_pitch = int(raster.stride(1)) if n_cols > 1 else n_depth
    row_pitch = int(raster.stride(0)) if n_rows > 1 else n_cols * pixel_pitch
    if valid is None:
        return n_rows, n_cols, n_depth, pixel_pitch, row_pitch, 0, 0
    assert valid.element_size() == 1 and tuple(valid.shape) == (n_rows, n_cols) and valid.stride(-1) == 1, "valid: uint8 [H, W] with dense rows"
    return n_rows, n_cols, n_depth, pixel_pitch, row_pitch, valid.data_ptr(), int(valid.stride(0)) if n_rows > 1 else n_cols


def encode_raster_tiles_device_depth(codec, raster, valid, max_z_err, tile, arena, slot_bytes=0):
    """raster: CUDA(HIP) tensor [H, W, C] or a view of one with contiguous channels and packed pixels (big[:, a:b]); valid: uint8 tensor
    [H, W] with dense rows or None; tile: (tileRows, tileCols).  The raster is cut into the grid of raster_tile_grid and every tile becomes
    one blob of nValuesPerPixel = C.  -> (status, offsets uint64[nTiles], sizes uint32[nTiles], arena bytes used)"""
    n_rows, n_cols, n_depth, pixel_pitch, row_pitch, d_valid, mask_pitch = _raster_depth_view(raster, valid)
    return codec.encode_raster_tiles_depth(raster.data_ptr(), _torch_dt_code(raster), n_cols, n_rows, n_depth, pixel_pitch, row_pitch, tile, d_valid,
                                           mask_pitch, max_z_err, arena.data_ptr(), arena.numel(), slot_bytes)


def decode_raster_tiles_device_depth(codec, arena, offsets, sizes, out, valid_out, tile):
    """the way back: out as `raster` above, valid_out as `valid` (written 1 / 0) or None; everything beside a view is left alone"""
    n_rows, n_cols, n_depth, pixel_pitch, row_pitch, d_valid, mask_pitch = _raster_depth_view(out, valid_out)
    return codec.decode_raster_tiles_depth(arena.data_ptr(), offsets, sizes, _torch_dt_code(out), n_cols, n_rows, n_depth, pixel_pitch, row_pitch, tile,
                                           out.data_ptr(), d_valid, mask_pitch)


def _raster_depth_strides(raster, valid):
    """-> (nRows, nCols, nDepth, pixelPitch, rowPitch, depthPitch, mask address, mask row pitch) of an [H, W, C] tensor with ANY strides:
    the pitches are its strides -- chw.permute(1, 2, 0) (planes), rgba[..., :3] (gapped pixels), big[a:b, c:d] (packed pixels, longer
    rows), a line-interleaved buffer.  Which layouts are taken is the library's to say (status 2); an axis of one element, whose
    stride says nothing, gets the pitch a dense tensor would have"""
    assert raster.dim() == 3, "raster: [H, W, C]"
    n_rows, n_cols, n_depth = (int(v) for v in raster.shape)
    depth_pitch = int(raster.stride(2)) if n_depth > 1 else 1
    pixel_pitch = int(raster.stride(1)) if n_cols > 1 else (n_depth if depth_pitch == 1 else 1)
    if n_rows > 1:
        row_pitch = int(raster.stride(0))
    else:
        row_pitch = (n_cols - 1) * pixel_pitch + n_depth if depth_pitch == 1 else n_cols
    if valid is None:
        return n_rows, n_cols, n_depth, pixel_pitch, row_pitch, depth_pitch, 0, 0
    assert valid.element_size() == 1 and tuple(valid.shape) == (n_rows, n_cols) and valid.stride(-1) == 1, "valid: uint8 [H, W] with dense rows"
    return n_rows, n_cols, n_depth, pixel_pitch, row_pitch, depth_pitch, valid.data_ptr(), int(valid.stride(0)) if n_rows > 1 else n_cols


def encode_raster_tiles_device_depth_strided(codec, raster, valid, max_z_err, tile, arena, slot_bytes=0):
    """encode_raster_tiles_device_depth for an [H, W, C] tensor with any strides, without a copy: chw.permute(1, 2, 0), rgba[..., :3],
    big[a:b, c:d], a line-interleaved buffer; a layout the library does not take comes back as status 2.  The blobs are those of the
    packed call on raster.contiguous().  -> (status, offsets uint64[nTiles], sizes uint32[nTiles], arena bytes used)"""
    n_rows, n_cols, n_depth, pixel_pitch, row_pitch, depth_pitch, d_valid, mask_pitch = _raster_depth_strides(raster, valid)
    return codec.encode_raster_tiles_depth_strided(raster.data_ptr(), _torch_dt_code(raster), n_cols, n_rows, n_depth, pixel_pitch, row_pitch,
                                                   depth_pitch, tile, d_valid, mask_pitch, max_z_err, arena.data_ptr(), arena.numel(), slot_bytes)


def decode_raster_tiles_device_depth_strided(codec, arena, offsets, sizes, out, valid_out, tile):
    """the way back: out as `raster` above, written where it lies -- the channels a gapped view leaves out (alpha) and everything
    beside a view untouched --, valid_out as `valid` (written 1 / 0) or None"""
    n_rows, n_cols, n_depth, pixel_pitch, row_pitch, depth_pitch, d_valid, mask_pitch = _raster_depth_strides(out, valid_out)
    return codec.decode_raster_tiles_depth_strided(arena.data_ptr(), offsets, sizes, _torch_dt_code(out), n_cols, n_rows, n_depth, pixel_pitch,
                                                   row_pitch, depth_pitch, tile, out.data_ptr(), d_valid, mask_pitch)


def encode_raster_tile_range_device_depth(codec, raster, valid, max_z_err, tile, tile_range, arena, slot_bytes=0):
    """encode_raster_tiles_device_depth_strided for a rectangle of the grid's tiles, tile_range = (tileRow0, tileCol0, nTileRows,
    nTileCols), as encode_raster_tile_range_device: raster and valid are the WHOLE raster, every blob is what the whole-raster call
    makes of that tile, and slotted the range takes the first rooms of the arena.
    -> (status, offsets, sizes, arena bytes used): full-grid tables, zero outside the range"""
    n_rows, n_cols, n_depth, pixel_pitch, row_pitch, depth_pitch, d_valid, mask_pitch = _raster_depth_strides(raster, valid)
    return codec.encode_raster_tiles_depth_range(raster.data_ptr(), _torch_dt_code(raster), n_cols, n_rows, n_depth, pixel_pitch, row_pitch,
                                                 depth_pitch, tile, tile_range, d_valid, mask_pitch, max_z_err, arena.data_ptr(), arena.numel(),
                                                 slot_bytes)


def decode_raster_window_device_depth(codec, arena, offsets, sizes, raster_shape, tile, window, out, valid_out):
    """a window of a depth mosaic, as decode_raster_window_device: raster_shape = (nRows, nCols) of the raster the grid of `tile` was cut
    from, offsets / sizes its full-grid tables, window = (row0, col0) the raster position of out's first pixel; out an [h, w, C] tensor
    with any strides whose size is the window's, valid_out uint8 [h, w] with dense rows or None.  Only the tiles of
    raster_window_tiles are read and decoded; nothing beside out's elements is written; a tile whose blob fails leaves its part zeroed"""
    rows, cols, n_depth, pixel_pitch, row_pitch, depth_pitch, d_valid, mask_pitch = _raster_depth_strides(out, valid_out)
    return codec.decode_raster_window_depth(arena.data_ptr(), offsets, sizes, _torch_dt_code(out), int(raster_shape[1]), int(raster_shape[0]),
                                            n_depth, tile, (int(window[0]), int(window[1]), rows, cols), out.data_ptr(), pixel_pitch, row_pitch,
                                            depth_pitch, d_valid, mask_pitch)


def raster_tile_grid(n_rows, n_cols, tile):
    """the tiles a raster of n_rows x n_cols is cut into, tile = (tileRows, tileCols): [(row0, row1, col0, col1)] in tile order, row by
    row of the grid -- the order of the raster tile calls' offsets and sizes; the last row and column of tiles are smaller where the
    raster is no multiple of the tile"""
    tile_rows, tile_cols = int(tile[0]), int(tile[1])
    assert n_rows > 0 and n_cols > 0 and tile_rows > 0 and tile_cols > 0
    return [(r0, min(n_rows, r0 + tile_rows), c0, min(n_cols, c0 + tile_cols))
            for r0 in range(0, n_rows, tile_rows) for c0 in range(0, n_cols, tile_cols)]


def _raster_view(raster, valid):
    """-> (nBands, nRows, nCols, pixelPitch, rowPitch, bandPitch, mask address, mask row pitch) of a raster tensor [R, C] or [B, R, C] with
    ANY strides -- a view into a larger tensor, a permuted [H, W, C] tensor, a slice of its channel axis: the pitches are its strides.
    Dense rows (stride(-1) == 1) are checked here, as ever; for any other layout the library's own check decides (status 2)."""
    assert raster.dim() in (2, 3), "raster: [R, C] or [B, R, C]"
    n_rows, n_cols = int(raster.shape[-2]), int(raster.shape[-1])
    n_bands = int(raster.shape[0]) if raster.dim() == 3 else 1
    pixel_pitch = int(raster.stride(-1)) if n_cols > 1 else 1
    band_pitch = int(raster.stride(0)) if (raster.dim() == 3 and n_bands > 1) else 0
    if pixel_pitch == 1:
        row_pitch = int(raster.stride(-2)) if n_rows > 1 else n_cols
        assert row_pitch >= n_cols and (n_bands == 1 or band_pitch >= (n_rows - 1) * row_pitch + n_cols), "raster: rows and bands must not overlap"
    else:
        row_pitch = int(raster.stride(-2)) if n_rows > 1 else (n_cols - 1) * pixel_pitch + n_bands
    if valid is None:
        return n_bands, n_rows, n_cols, pixel_pitch, row_pitch, band_pitch, 0, 0
    assert valid.element_size() == 1 and tuple(valid.shape) == (n_rows, n_cols) and valid.stride(-1) == 1, "valid: uint8 [R, C] with dense rows"
    mask_pitch = int(valid.stride(0)) if n_rows > 1 else n_cols
    assert mask_pitch >= n_cols
    return n_bands, n_rows, n_cols, pixel_pitch, row_pitch, band_pitch, valid.data_ptr(), mask_pitch


def encode_raster_tiles_device(codec, raster, valid, max_z_err, tile, arena, slot_bytes=0):
    """raster: CUDA(HIP) tensor [R, C] or [B, R, C], a view with any strides: band-sequential (stride(-1) == 1) goes to the raster tile
    call as ever; anything else -- hwc.permute(2, 0, 1), rgba[..., :3].permute(2, 0, 1), one channel of an interleaved image -- goes to
    the strided call with pixelPitch = stride(-1), bandPitch = stride(0), without a copy; a layout the library does not take comes back
    as status 2.  valid: uint8 tensor [R, C] with dense rows (0 = invalid, one mask for all bands) or None; tile: (tileRows, tileCols);
    arena: uint8 CUDA tensor.  The raster is cut into the grid of
    raster_tile_grid and every tile becomes one blob, exactly what encode() makes of that rectangle (all bands, its part of the mask);
    slot_bytes != 0 (a multiple of 16): every blob in a room of its own, offsets says which.
    -> (status, offsets uint64[nTiles], sizes uint32[nTiles], arena bytes used)"""
    n_bands, n_rows, n_cols, pixel_pitch, row_pitch, band_pitch, d_valid, mask_pitch = _raster_view(raster, valid)
    if pixel_pitch == 1:
        return codec.encode_raster_tiles(raster.data_ptr(), _torch_dt_code(raster), n_cols, n_rows, n_bands, row_pitch, band_pitch, tile, d_valid,
                                         mask_pitch, max_z_err, arena.data_ptr(), arena.numel(), slot_bytes)
    return codec.encode_raster_tiles_strided(raster.data_ptr(), _torch_dt_code(raster), n_cols, n_rows, n_bands, pixel_pitch, row_pitch, band_pitch,
                                             tile, d_valid, mask_pitch, max_z_err, arena.data_ptr(), arena.numel(), slot_bytes)


def decode_raster_tiles_device(codec, arena, offsets, sizes, out, valid_out, tile):
    """the way back: out a tensor as `raster` above (any strides: a pixel-interleaved view is written in place, its uncoded channels and
    everything beside it untouched), valid_out as `valid` (written 1 / 0) or None.  A tile whose blob fails leaves its
    rectangle zeroed, all bands and mask; elements outside the rows of `out` (a view's surroundings) are not touched."""
    n_bands, n_rows, n_cols, pixel_pitch, row_pitch, band_pitch, d_valid, mask_pitch = _raster_view(out, valid_out)
    if pixel_pitch == 1:
        return codec.decode_raster_tiles(arena.data_ptr(), offsets, sizes, _torch_dt_code(out), n_cols, n_rows, n_bands, row_pitch, band_pitch, tile,
                                         out.data_ptr(), d_valid, mask_pitch)
    return codec.decode_raster_tiles_strided(arena.data_ptr(), offsets, sizes, _torch_dt_code(out), n_cols, n_rows, n_bands, pixel_pitch, row_pitch,
                                             band_pitch, tile, out.data_ptr(), d_valid, mask_pitch)


def raster_window_tiles(n_rows, n_cols, tile, window_rect):
    """the indices, in the order of raster_tile_grid, of the tiles the window window_rect = (row0, col0, rows, cols) of a raster of
    n_rows x n_cols touches: the entries of offsets / sizes decode_raster_window_device reads"""
    tile_rows, tile_cols = int(tile[0]), int(tile[1])
    row0, col0, rows, cols = (int(v) for v in window_rect)
    assert n_rows > 0 and n_cols > 0 and tile_rows > 0 and tile_cols > 0
    assert rows > 0 and cols > 0 and 0 <= row0 and row0 + rows <= n_rows and 0 <= col0 and col0 + cols <= n_cols, "the window lies inside the raster"
    n_tx = -(-n_cols // tile_cols)
    return [ty * n_tx + tx for ty in range(row0 // tile_rows, (row0 + rows - 1) // tile_rows + 1)
            for tx in range(col0 // tile_cols, (col0 + cols - 1) // tile_cols + 1)]


def encode_raster_tile_range_device(codec, raster, valid, max_z_err, tile, tile_range, arena, slot_bytes=0):
    """encode_raster_tiles_device for a rectangle of the grid's tiles: tile_range = (tileRow0, tileCol0, nTileRows, nTileCols) -- the tiles
    a dirty region touches, a rank's rows of tiles (shard.raster_tile_rows).  raster and valid are the WHOLE raster, as there (any
    strides).  Only the range's tiles are cut and coded, each blob what the whole-raster call makes of that tile; slotted, they take
    the first nTileRows * nTileCols rooms of the arena.
    -> (status, offsets uint64[nTiles], sizes uint32[nTiles], arena bytes used): full-grid tables, zero outside the range"""
    n_bands, n_rows, n_cols, pixel_pitch, row_pitch, band_pitch, d_valid, mask_pitch = _raster_view(raster, valid)
    return codec.encode_raster_tiles_range(raster.data_ptr(), _torch_dt_code(raster), n_cols, n_rows, n_bands, pixel_pitch, row_pitch, band_pitch,
                                           tile, tile_range, d_valid, mask_pitch, max_z_err, arena.data_ptr(), arena.numel(), slot_bytes)


def decode_raster_window_device(codec, arena, offsets, sizes, raster_shape, tile, window, out, valid_out):
    """a window of a mosaic: raster_shape = (nRows, nCols) of the raster the grid of `tile` was cut from, offsets / sizes its full-grid
    tables, window = (row0, col0) the raster position of out's first pixel; out a tensor [h, w] or [B, h, w] with any strides (as
    decode_raster_tiles_device's), whose size is the window's; valid_out uint8 [h, w] with dense rows, or None.  Only the tiles of
    raster_window_tiles are read and decoded; nothing beside out's elements is written.  A tile whose blob fails leaves its part of
    the window zeroed."""
    n_bands, rows, cols, pixel_pitch, row_pitch, band_pitch, d_valid, mask_pitch = _raster_view(out, valid_out)
    return codec.decode_raster_window(arena.data_ptr(), offsets, sizes, _torch_dt_code(out), int(raster_shape[1]), int(raster_shape[0]), n_bands,
                                      tile, (int(window[0]), int(window[1]), rows, cols), out.data_ptr(), pixel_pitch, row_pitch, band_pitch,
                                      d_valid, mask_pitch)


def _nodata_view(t):
    """-> (nRows, nCols, pixelPitch, rowPitch) of an [H, W] tensor with any strides: a pitched raster, a view into a larger tensor, one
    channel of an interleaved image (hwc[..., k]); what the library does not take comes back as status 2"""
    assert t.dim() == 2, "an [H, W] tensor"
    n_rows, n_cols = int(t.shape[0]), int(t.shape[1])
    pixel_pitch = int(t.stride(1)) if n_cols > 1 else 1
    row_pitch = int(t.stride(0)) if n_rows > 1 else (n_cols - 1) * pixel_pitch + 1
    return n_rows, n_cols, pixel_pitch, row_pitch


def encode_raster_tiles_device_nodata(codec, raster, no_data, max_z_err, tile, arena, slot_bytes=0, tile_range=None):
    """encode_raster_tiles_device for an [H, W] raster (any strides) whose validity is a VALUE (include/lerc_amd_nodata.h): a pixel is
    invalid when it equals no_data by the type's own ==, or is a NaN where no_data is NaN; no_data must be an element of the raster's
    type (else status 2).  Every blob is what the masked call makes of the raster and the mask `raster != no_data` (`~isnan`), which is
    made in the staging pass and never exists as a tensor; values at invalid pixels, NaN included, never influence a byte.
    tile_range = (tileRow0, tileCol0, nTileRows, nTileCols) or None for the whole grid, as encode_raster_tile_range_device.
    -> (status, offsets uint64[nTiles], sizes uint32[nTiles], arena bytes used): full-grid tables, zero outside the range"""
    n_rows, n_cols, pixel_pitch, row_pitch = _nodata_view(raster)
    ty0, tx0, nty, ntx = (0, 0, -1, -1) if tile_range is None else (int(v) for v in tile_range)
    return codec.encode_raster_tiles_nodata(raster.data_ptr(), _torch_dt_code(raster), n_cols, n_rows, pixel_pitch, row_pitch, tile,
                                            (ty0, tx0, nty, ntx), no_data, max_z_err, arena.data_ptr(), arena.numel(), slot_bytes)


def decode_raster_window_device_nodata(codec, arena, offsets, sizes, raster_shape, tile, window, out, no_data, valid_out=None):
    """a window of a mosaic as decode_raster_window_device, into an [h, w] tensor with any strides: a valid pixel holds what that call
    writes, an invalid one no_data (a quiet NaN where no_data is NaN), and so does the part of a tile whose blob fails (the first such
    status comes back).  valid_out: uint8 [h, w] with dense rows, written 1 / 0, or None.  window = (row0, col0)."""
    rows, cols, pixel_pitch, row_pitch = _nodata_view(out)
    d_valid, mask_pitch = 0, 0
    if valid_out is not None:
        assert valid_out.element_size() == 1 and tuple(valid_out.shape) == (rows, cols) and valid_out.stride(-1) == 1, "valid_out: uint8 [h, w] with dense rows"
        d_valid, mask_pitch = valid_out.data_ptr(), (int(valid_out.stride(0)) if rows > 1 else cols)
    return codec.decode_raster_window_nodata(arena.data_ptr(), offsets, sizes, _torch_dt_code(out), int(raster_shape[1]), int(raster_shape[0]), tile,
                                             (int(window[0]), int(window[1]), rows, cols), out.data_ptr(), pixel_pitch, row_pitch, no_data, d_valid,
                                             mask_pitch)


def decode_raster_tiles_device_nodata(codec, arena, offsets, sizes, out, no_data, tile, valid_out=None):
    """the whole raster back: decode_raster_window_device_nodata with the window that covers everything"""
    return decode_raster_window_device_nodata(codec, arena, offsets, sizes, tuple(out.shape), tile, (0, 0), out, no_data, valid_out)
