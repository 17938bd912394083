"""Shared by test_sim_capi_boundary.py (CPU emulator library) and test_gpu_capi_boundary.py (MI355X): what every status-returning
entry point of include/lerc_amd.h and include/lerc_amd_device.h answers at the C boundary (lerc_amd/csrc/capi.cpp).

SPECS describes each entry point: its arguments in header order, each with a role, and how the smallest valid call is made (an
8 x 16 float32 raster, two tiles of 8 x 16, a 24 x 40 raster in tiles of 16 x 16).  rows_of() derives the variations from the roles --
every pointer nulled, every count at 0 and -1, dataType 8, maxZErr -1, slotBytes 8 and 0, the mask rules, dimensions beyond INT_MAX --
and TABLE records, row by row, the status the library returned when the table was made and what a refusing call left in its
out-parameters (0, or kept: the sentinel it was handed).  A refused call launches nothing; the valid ones are a few small launches.
`python tests/capi_boundary_common.py` prints the table anew from the emulator library.
"""
import ctypes as ct

import numpy as np

import capi
import tiles_masked_common as M

CT = {"vp": ct.c_void_p, "u32": ct.c_uint, "i": ct.c_int, "d": ct.c_double, "u64": ct.c_ulonglong}
SENT32, SENT64 = 0xEEEEEEEE, 0xEEEEEEEEEEEEEEEE
E = 0.01                       # maxZErr of every valid call
R, C = 8, 16                   # the raster of the single-raster calls and the tiles of the batches
RR, RC, TILE = 24, 40, 16      # the raster of the raster-tile calls: 2 x 3 tiles, the right column 8 wide, the bottom row 8 high
ROW_PITCH, MASK_PITCH = RC + 5, RC + 3
BAND_PITCH = RR * ROW_PITCH + 7
WINDOW = (5, 7, 13, 21)        # row0, col0, rows, cols: not aligned to tiles
WIN_PITCH = 21 + 5
RANGE = (1, 1, 1, 2)           # tileRow0, tileCol0, nTileRows, nTileCols: not from (0, 0)
BIG = 50000                    # BIG * BIG pixels are more than INT_MAX
TOL = E + 2.0 ** -14           # a decoded value is rounded to float32: half an ulp below 1024 on top of maxZErr


def A(name, ctype, role="v"):
    """roles: ptr (may not be NULL), cnt (a count: 0 and -1), nz (unsigned, may not be 0), dt, err, slot, o32 / o64 (a scalar the
    call writes: handed a sentinel), v (not varied by its role)"""
    return (name, ctype, role)


# ---- argument lists, in header order ----------------------------------------------------------------------------------------------
def _raster(p):
    return [A(p + "Data", "vp", "ptr"), A("dataType", "u32", "dt"), A("nDepth", "i", "cnt"), A("nCols", "i", "cnt"), A("nRows", "i", "cnt"),
            A("nBands", "i", "cnt"), A("nMasks", "i"), A(p + "ValidBytes", "vp"), A("maxZErr", "d", "err")]


def _blob(p, size="blobSize"):
    return [A(p + "LercBlob", "vp", "ptr"), A(size, "u32", "nz"), A("nMasks", "i"), A(p + "ValidBytes", "vp"), A("nDepth", "i", "cnt"),
            A("nCols", "i", "cnt"), A("nRows", "i", "cnt"), A("nBands", "i", "cnt")]


CTX = A("ctx", "vp", "ptr")
OUT_BUF = [A("pOutBuffer", "vp", "ptr"), A("outBufferSize", "u32", "nz"), A("nBytesWritten", "vp", "o32")]
NODATA = [A("pUsesNoData", "vp"), A("noDataValues", "vp")]
VERSION = A("codecVersion", "i")
TILE_DIMS = [A("nCols", "i", "cnt"), A("nRows", "i", "cnt"), A("nTiles", "i", "cnt")]
ARENA_OUT = [A("offsets", "vp", "ptr"), A("sizes", "vp", "ptr"), A("arenaUsed", "vp", "o64")]
ARENA_IN = [A("dArena", "vp", "ptr"), A("offsets", "vp", "ptr"), A("sizes", "vp", "ptr")]
TILES_BACK = [A("nTiles", "i", "cnt"), A("nCols", "i", "cnt"), A("nRows", "i", "cnt")]
PITCHES = [A("rowPitch", "u64"), A("bandPitch", "u64")]
PX_PITCHES = [A("pixelPitch", "u64")] + PITCHES
RT_DIMS = [A("dataType", "u32", "dt"), A("nCols", "i", "cnt"), A("nRows", "i", "cnt"), A("nBands", "i", "cnt")]
RT_TILE = [A("tileCols", "i", "cnt"), A("tileRows", "i", "cnt")]
RT_MASK = [A("nMasks", "i"), A("dValidBytes", "vp"), A("maskRowPitch", "u64")]
RT_ARENA_OUT = [A("maxZErr", "d", "err"), A("dArena", "vp", "ptr"), A("arenaCapacity", "u64"), A("slotBytes", "u64", "slot")] + ARENA_OUT
RT_RANGE = [A("tileCol0", "i"), A("tileRow0", "i"), A("nTileCols", "i", "cnt"), A("nTileRows", "i", "cnt")]
RT_WINDOW = [A("winCol0", "i"), A("winRow0", "i"), A("winCols", "i", "cnt"), A("winRows", "i", "cnt")]


class Env:
    """one library, one context, the inputs of the valid calls (made once, only read by the calls) and their output buffers"""

    def __init__(self, L, mem):
        self.L, self.mem, self.keep = L, mem, []
        L.lerc_amd_create.restype = ct.c_void_p
        L.lerc_amd_create.argtypes = [ct.c_void_p]
        L.lerc_amd_destroy.argtypes = [ct.c_void_p]
        L.lerc_amd_destroy.restype = None
        for name, spec in SPECS.items():
            f = getattr(L, name.split("@")[0])
            f.restype, f.argtypes = ct.c_uint, [CT[c] for _, c, _ in spec["args"]]
        self.h = L.lerc_amd_create(None)
        assert self.h
        rng = np.random.default_rng(11)
        yy, xx = np.mgrid[0:RR, 0:RC]
        land = (700 + 90 * np.sin(yy / 5.0) * np.cos(xx / 7.0)).astype(np.float32)
        self.stack = np.stack([land[:R, :C] + 3 * k + rng.normal(0, 2, (R, C)).astype(np.float32) for k in range(3)])      # [3, R, C]
        self.masks = (rng.random((3, R, C)) < 0.8).astype(np.uint8)
        self.tiles = np.stack([self.stack + 10 * t for t in range(2)]).astype(np.float32)                                   # [2, 3, R, C]
        self.tile_masks = np.stack([self.masks, self.masks[::-1]])
        self.raster = (land + rng.normal(0, 2, (RR, RC))).astype(np.float32)
        self.d_stack, self.d_masks = self.up(self.stack), self.up(self.masks)
        self.d_tiles, self.d_tile_masks = self.up(self.tiles), self.up(self.tile_masks)
        self.bits = self.up(np.packbits(rng.random(512) < 0.7))                                                             # 64 mask bytes
        pitched = np.zeros((3, BAND_PITCH), np.float32)
        for k in range(3):
            rows = np.lib.stride_tricks.as_strided(pitched[k], (RR, RC), (ROW_PITCH * 4, 4))
            rows[...] = self.raster + k
        self.d_raster = self.up(pitched)
        self.d_raster_mask = self.up(np.ones((RR, MASK_PITCH), np.uint8))
        self.blob = self.d_blob = self.arena = self.slots = self.rt_arena = self.rle = None

    def close(self):
        if self.h:
            self.L.lerc_amd_destroy(self.h)
            self.h = None

    def up(self, a):
        k, p = self.mem.up(a)
        self.keep.append(k)
        return p

    def out(self, nbytes):
        """a device buffer a call writes -> (key for down(), address)"""
        k, p = self.mem.empty(nbytes)
        self.keep.append(k)
        return k, p

    def host(self, a):
        self.keep.append(a)
        return a.ctypes.data

    def call(self, name, args):
        return int(getattr(self.L, name.split("@")[0])(*args))

    # -- what the decode directions need: made by the valid encode calls of the same library
    def need_blob(self):
        if self.blob is None:
            buf, n = np.zeros(4096, np.uint8), ct.c_uint(0)
            a = np.ascontiguousarray(self.stack[0])
            assert self.L.lerc_encode(a.ctypes.data, 6, 1, C, R, 1, 0, None, E, buf.ctypes.data, 4096, ct.byref(n)) == 0
            self.blob = buf[:n.value].copy()
            self.d_blob = self.up(np.concatenate([self.blob, np.zeros(64, np.uint8)]))
        return self.blob

    def need_arena(self):
        if self.arena is None:
            _, pa = self.out(8192)
            offs, sizes = np.zeros(2, np.uint64), np.zeros(2, np.uint32)
            flat = self.up(self.tiles[:, 0])
            assert self.L.lerc_amd_encode_tiles_device(self.h, flat, 6, C, R, 2, E, pa, 8192, self.host(offs), self.host(sizes), None) == 0
            self.arena = (pa, offs, sizes, flat)
        return self.arena

    def need_slots(self):
        if self.slots is None:
            _, ps = self.out(2 * 2048)
            sizes = np.zeros(2, np.uint32)
            assert self.L.lerc_amd_encode_tiles_device_slots(self.h, self.need_arena()[3], 6, C, R, 2, E, ps, 2048, self.host(sizes)) == 0
            self.slots = (ps, sizes)
        return self.slots

    def need_rt_arena(self):
        if self.rt_arena is None:
            _, pa = self.out(6 * 2048)
            offs, sizes = np.zeros(6, np.uint64), np.zeros(6, np.uint32)
            assert self.L.lerc_amd_encode_raster_tiles_device(self.h, self.d_raster, 6, RC, RR, 1, ROW_PITCH, BAND_PITCH, TILE, TILE, 0, None, 0, E, pa,
                                                              6 * 2048, 0, self.host(offs), self.host(sizes), None) == 0
            self.rt_arena = (pa, offs, sizes)
        return self.rt_arena

    def need_rle(self):
        if self.rle is None:
            _, po = self.out(256)
            n = ct.c_uint(0)
            assert self.L.lerc_amd_mask_rle_device(self.h, self.bits, 64, po, 256, ct.byref(n)) == 0
            self.rle = (po, n.value)
        return self.rle

    def near(self, key, shape, want):
        got = self.mem.down(key)[:int(np.prod(shape)) * 4].view(np.float32).reshape(shape)
        assert np.abs(got.astype(np.float64) - want).max() <= TOL, "decoded pixels are further than maxZErr from the input"


# ---- the valid calls: name -> values by argument name (out scalars are made per call); "_mask": the pointer of the mask rows; "_check":
# called after the valid call
def v_encode_host(env, name):
    out = np.zeros(4096, np.uint8)
    return dict(pData=env.host(np.ascontiguousarray(env.stack)), dataType=6, nDepth=1, nCols=C, nRows=R, nBands=1, nMasks=0, pValidBytes=None,
                maxZErr=E, pOutBuffer=env.host(out), outBufferSize=4096, pUsesNoData=None, noDataValues=None, codecVersion=3 if "@v3" in name else -1,
                _mask=env.host(env.masks.copy()))


def v_decode_host(env, name):
    blob = env.need_blob()
    wide = "ToDouble" in name
    out = np.zeros((3, R, C), np.float64 if wide else np.float32)

    def check():
        assert np.abs(out[0].astype(np.float64) - env.stack[0]).max() <= TOL
    return dict(pLercBlob=env.host(blob), blobSize=len(blob), nMasks=0, pValidBytes=None, nDepth=1, nCols=C, nRows=R, nBands=1, dataType=6,
                pData=env.host(out), pUsesNoData=None, noDataValues=None, _mask=env.host(np.zeros((3, R, C), np.uint8)), _check=check)


def v_blob_info(env, name):
    blob = env.need_blob()
    return dict(pLercBlob=env.host(blob), blobSize=len(blob), infoArray=env.host(np.zeros(11, np.uint32)), dataRangeArray=env.host(np.zeros(3)),
                infoArraySize=11, dataRangeArraySize=3, nDepth=1, nBands=1, pMins=env.host(np.zeros(3)), pMaxs=env.host(np.zeros(3)))


def v_encode_device(env, name):
    _, po = env.out(4096)
    return dict(ctx=env.h, dData=env.d_stack, dataType=6, nDepth=1, nCols=C, nRows=R, nBands=1, nMasks=0, dValidBytes=None, maxZErr=E,
                dOutBuffer=po, outBufferSize=4096, _mask=env.d_masks)


def v_decode_device(env, name):
    blob = env.need_blob()
    ko, po = env.out(3 * R * C * 4)
    _, pm = env.out(3 * R * C)
    sync = "async" not in name
    return dict(ctx=env.h, dLercBlob=env.d_blob, blobSize=len(blob), blobSizeBound=len(blob), nMasks=0, dValidBytes=None, nDepth=1, nCols=C, nRows=R,
                nBands=1, dataType=6, dData=po, _mask=pm, _check=(lambda: env.near(ko, (R, C), env.stack[0])) if sync else None)


def v_finish(env, name):
    """(made anew for every row: a ticket is handed out once)"""
    _, po = env.out(4096)
    t = ct.c_uint(0)
    assert env.L.lerc_amd_encode_device_async(env.h, env.d_stack, 6, 1, C, R, 1, 0, None, E, po, 4096, ct.byref(t)) == 0 and t.value
    return dict(ctx=env.h, ticket=t.value)


def v_tiles_encode(env, name):
    bands = name.endswith("_bands")
    _, pa = env.out(8192)
    return dict(ctx=env.h, dTiles=env.d_tiles if bands else env.need_arena()[3], dataType=6, nCols=C, nRows=R, nBands=1, nTiles=2, nMasks=0,
                dValidBytes=None, maxZErr=E, dArena=pa, dSlots=pa, arenaCapacity=8192, slotBytes=2048 if name.endswith("_slots") else 0,
                offsets=env.host(np.zeros(2, np.uint64)), sizes=env.host(np.zeros(2, np.uint32)), _mask=env.d_tile_masks)


def v_tiles_decode(env, name):
    pa, offs, sizes, _ = env.need_arena()
    ko, po = env.out(2 * 3 * R * C * 4)
    _, pm = env.out(2 * 3 * R * C)
    d = dict(ctx=env.h, dArena=pa, offsets=offs.ctypes.data, sizes=sizes.ctypes.data, nTiles=2, nCols=C, nRows=R, nBands=1, dataType=6, dTiles=po,
             nMasks=0, dValidBytes=None, _mask=pm, _check=lambda: env.near(ko, (2, R, C), env.tiles[:, 0]))
    if name.endswith("_slots"):
        ps, ssizes = env.need_slots()
        d.update(dSlots=ps, slotBytes=2048, sizes=ssizes.ctypes.data)
    return d


def v_raster_encode(env, name):
    _, pa = env.out(6 * 2048)
    return dict(ctx=env.h, dRaster=env.d_raster, dataType=6, nCols=RC, nRows=RR, nBands=1, pixelPitch=1, rowPitch=ROW_PITCH, bandPitch=BAND_PITCH,
                tileCols=TILE, tileRows=TILE, tileCol0=RANGE[1], tileRow0=RANGE[0], nTileCols=RANGE[3], nTileRows=RANGE[2], nMasks=0, dValidBytes=None,
                maskRowPitch=0, maxZErr=E, dArena=pa, arenaCapacity=6 * 2048, slotBytes=0, offsets=env.host(np.zeros(6, np.uint64)),
                sizes=env.host(np.zeros(6, np.uint32)), _mask=env.d_raster_mask, _mask_with=dict(maskRowPitch=MASK_PITCH))


def v_raster_decode(env, name):
    pa, offs, sizes = env.need_rt_arena()
    window = name.endswith("_window_device")
    r0, c0, h, w = WINDOW if window else (0, 0, RR, RC)
    pitch = WIN_PITCH if window else ROW_PITCH
    band_pitch = h * pitch + 7
    ko, po = env.out(3 * band_pitch * 4)
    _, pm = env.out(RR * MASK_PITCH)

    def check():
        got = env.mem.down(ko)[:band_pitch * 4].view(np.float32)
        rows = np.lib.stride_tricks.as_strided(got, (h, w), (pitch * 4, 4))
        assert np.abs(rows.astype(np.float64) - env.raster[r0:r0 + h, c0:c0 + w]).max() <= TOL, "decoded pixels are not the raster's"
    return dict(ctx=env.h, dArena=pa, offsets=offs.ctypes.data, sizes=sizes.ctypes.data, dataType=6, nCols=RC, nRows=RR, nBands=1, pixelPitch=1,
                rowPitch=pitch, bandPitch=band_pitch, tileCols=TILE, tileRows=TILE, winCol0=c0, winRow0=r0, winCols=w, winRows=h, dRaster=po, dWindow=po,
                nMasks=0, dValidBytes=None, maskRowPitch=0, _mask=pm, _mask_with=dict(maskRowPitch=MASK_PITCH), _check=check)


def v_mask_rle(env, name):
    _, po = env.out(256)
    return dict(ctx=env.h, dBits=env.bits, nBytes=64, dOut=po, cap=256)


def v_mask_rle_decode(env, name):
    pr, n = env.need_rle()
    _, pb = env.out(64)
    return dict(ctx=env.h, dRle=pr, rleBytes=n, dBits=pb, nBytes=64)


def v_gather(env, name):
    """(no valid call: that takes an RCCL communicator; the rows are the two refusals in front of it)"""
    return dict(ctx=env.h, ncclComm=1, root=0, dMessage=None, nBytes=0, dRootBuffer=None, rootCapacity=0, hLengths=None, hOffsets=None, stream=None)


def S(args, valid, extra=(), cached=True, no_valid=False, drain=False):
    return dict(args=args, valid=valid, extra=list(extra), cached=cached, no_valid=no_valid, drain=drain)


VERSIONS = [("codecVersion=7", dict(codecVersion=7)), ("codecVersion=1", dict(codecVersion=1)), ("codecVersion=0", dict(codecVersion=0))]
FLAGGED = ("pUsesNoData,noDataValues=NULL", dict(pUsesNoData="_flags", noDataValues=None))
SIZE_QUERY = ("dOutBuffer=NULL", dict(dOutBuffer=None))
WITH_MASK = ("dValidBytes", dict(dValidBytes="_mask"))
INFO = [("infoArray=NULL", dict(infoArray=None)), ("dataRangeArray=NULL", dict(dataRangeArray=None)),
        ("infoArray,dataRangeArray=NULL", dict(infoArray=None, dataRangeArray=None)), ("bothSizes=0", dict(infoArraySize=0, dataRangeArraySize=0))]
RT_ENC = [CTX, A("dRaster", "vp", "ptr")] + RT_DIMS
RT_DEC = [CTX] + ARENA_IN + RT_DIMS

SPECS = {
    "lerc_computeCompressedSize": S(_raster("p") + [A("numBytes", "vp", "o32")], v_encode_host),
    "lerc_encode": S(_raster("p") + OUT_BUF, v_encode_host),
    "lerc_computeCompressedSize_4D": S(_raster("p") + [A("numBytes", "vp", "o32")] + NODATA, v_encode_host, [FLAGGED]),
    "lerc_encode_4D": S(_raster("p") + OUT_BUF + NODATA, v_encode_host, [FLAGGED]),
    "lerc_computeCompressedSizeForVersion": S(_raster("p")[:1] + [VERSION] + _raster("p")[1:] + [A("numBytes", "vp", "o32")], v_encode_host, VERSIONS),
    "lerc_computeCompressedSizeForVersion@v3": S(_raster("p")[:1] + [VERSION] + _raster("p")[1:] + [A("numBytes", "vp", "o32")], v_encode_host),
    "lerc_encodeForVersion": S(_raster("p")[:1] + [VERSION] + _raster("p")[1:] + OUT_BUF, v_encode_host, VERSIONS),
    "lerc_encodeForVersion@v3": S(_raster("p")[:1] + [VERSION] + _raster("p")[1:] + OUT_BUF, v_encode_host),
    "lerc_getBlobInfo": S([A("pLercBlob", "vp", "ptr"), A("blobSize", "u32", "nz"), A("infoArray", "vp"), A("dataRangeArray", "vp"),
                           A("infoArraySize", "i", "cnt"), A("dataRangeArraySize", "i", "cnt")], v_blob_info, INFO),
    "lerc_getDataRanges": S([A("pLercBlob", "vp", "ptr"), A("blobSize", "u32", "nz"), A("nDepth", "i", "cnt"), A("nBands", "i", "cnt"),
                             A("pMins", "vp", "ptr"), A("pMaxs", "vp", "ptr")], v_blob_info),
    "lerc_decode": S(_blob("p") + [A("dataType", "u32", "dt"), A("pData", "vp", "ptr")], v_decode_host),
    "lerc_decode_4D": S(_blob("p") + [A("dataType", "u32", "dt"), A("pData", "vp", "ptr")] + NODATA, v_decode_host),
    "lerc_decodeToDouble": S(_blob("p") + [A("pData", "vp", "ptr")], v_decode_host),
    "lerc_decodeToDouble_4D": S(_blob("p") + [A("pData", "vp", "ptr")] + NODATA, v_decode_host),
    "lerc_amd_encode_device": S([CTX] + _raster("d") + [A("dOutBuffer", "vp"), A("outBufferSize", "u32"), A("nBytesWritten", "vp", "o32")],
                                v_encode_device, [SIZE_QUERY]),
    "lerc_amd_decode_device": S([CTX] + _blob("d") + [A("dataType", "u32", "dt"), A("dData", "vp", "ptr")], v_decode_device),
    "lerc_amd_encode_device_async": S([CTX] + _raster("d") + [A("dOutBuffer", "vp"), A("outBufferSize", "u32"), A("ticket", "vp", "o32")],
                                      v_encode_device, [SIZE_QUERY], drain=True),
    "lerc_amd_decode_device_async": S([CTX] + _blob("d", "blobSizeBound") + [A("dataType", "u32", "dt"), A("dData", "vp", "ptr"), A("ticket", "vp", "o32")],
                                      v_decode_device, drain=True),
    "lerc_amd_finish": S([CTX, A("ticket", "u32"), A("nBytes", "vp", "o32")], v_finish, [("ticket=unknown", dict(ticket=0x7FFFFFF0))], cached=False,
                         drain=True),
    "lerc_amd_encode_tiles_device": S([CTX, A("dTiles", "vp", "ptr"), A("dataType", "u32", "dt")] + TILE_DIMS + [A("maxZErr", "d", "err"),
                                      A("dArena", "vp", "ptr"), A("arenaCapacity", "u64")] + ARENA_OUT, v_tiles_encode),
    "lerc_amd_decode_tiles_device": S([CTX] + ARENA_IN + TILES_BACK + [A("dataType", "u32", "dt"), A("dTiles", "vp", "ptr")], v_tiles_decode),
    "lerc_amd_encode_tiles_device_slots": S([CTX, A("dTiles", "vp", "ptr"), A("dataType", "u32", "dt")] + TILE_DIMS + [A("maxZErr", "d", "err"),
                                            A("dSlots", "vp", "ptr"), A("slotBytes", "u64", "slot"), A("sizes", "vp", "ptr")], v_tiles_encode),
    "lerc_amd_decode_tiles_device_slots": S([CTX, A("dSlots", "vp", "ptr"), A("slotBytes", "u64", "slot"), A("sizes", "vp", "ptr")] + TILES_BACK
                                            + [A("dataType", "u32", "dt"), A("dTiles", "vp", "ptr")], v_tiles_decode),
    "lerc_amd_encode_tiles_device_masked": S([CTX, A("dTiles", "vp", "ptr"), A("dataType", "u32", "dt")] + TILE_DIMS + [A("dValidBytes", "vp"),
                                             A("maxZErr", "d", "err"), A("dArena", "vp", "ptr"), A("arenaCapacity", "u64"), A("slotBytes", "u64", "slot")]
                                             + ARENA_OUT, v_tiles_encode, [WITH_MASK]),
    "lerc_amd_decode_tiles_device_masked": S([CTX] + ARENA_IN + TILES_BACK + [A("dataType", "u32", "dt"), A("dTiles", "vp", "ptr"), A("dValidBytes", "vp")],
                                             v_tiles_decode, [WITH_MASK]),
    "lerc_amd_encode_tiles_device_bands": S([CTX, A("dTiles", "vp", "ptr"), A("dataType", "u32", "dt"), A("nCols", "i", "cnt"), A("nRows", "i", "cnt"),
                                            A("nBands", "i", "cnt"), A("nTiles", "i", "cnt"), A("nMasks", "i"), A("dValidBytes", "vp"),
                                            A("maxZErr", "d", "err"), A("dArena", "vp", "ptr"), A("arenaCapacity", "u64"), A("slotBytes", "u64", "slot")]
                                            + ARENA_OUT, v_tiles_encode),
    "lerc_amd_decode_tiles_device_bands": S([CTX] + ARENA_IN + TILES_BACK + [A("nBands", "i", "cnt"), A("dataType", "u32", "dt"), A("dTiles", "vp", "ptr"),
                                            A("nMasks", "i"), A("dValidBytes", "vp")], v_tiles_decode),
    "lerc_amd_encode_raster_tiles_device": S(RT_ENC + PITCHES + RT_TILE + RT_MASK + RT_ARENA_OUT, v_raster_encode),
    "lerc_amd_decode_raster_tiles_device": S(RT_DEC + PITCHES + RT_TILE + [A("dRaster", "vp", "ptr")] + RT_MASK, v_raster_decode),
    "lerc_amd_encode_raster_tiles_device_strided": S(RT_ENC + PX_PITCHES + RT_TILE + RT_MASK + RT_ARENA_OUT, v_raster_encode),
    "lerc_amd_decode_raster_tiles_device_strided": S(RT_DEC + PX_PITCHES + RT_TILE + [A("dRaster", "vp", "ptr")] + RT_MASK, v_raster_decode),
    "lerc_amd_encode_raster_tiles_device_range": S(RT_ENC + PX_PITCHES + RT_TILE + RT_RANGE + RT_MASK + RT_ARENA_OUT, v_raster_encode,
                                                   [("tileCol0=-1", dict(tileCol0=-1)), ("tileRow0=-1", dict(tileRow0=-1))]),
    "lerc_amd_decode_raster_window_device": S(RT_DEC + RT_TILE + RT_WINDOW + [A("dWindow", "vp", "ptr")] + PX_PITCHES + RT_MASK, v_raster_decode),
    "lerc_amd_gather_blobs": S([CTX, A("ncclComm", "vp", "ptr"), A("root", "i"), A("dMessage", "vp"), A("nBytes", "u64"), A("dRootBuffer", "vp"),
                                A("rootCapacity", "u64"), A("hLengths", "vp"), A("hOffsets", "vp"), A("stream", "vp")], v_gather, no_valid=True),
    "lerc_amd_mask_rle_device": S([CTX, A("dBits", "vp", "ptr"), A("nBytes", "u32", "nz"), A("dOut", "vp", "ptr"), A("cap", "u32"), A("size", "vp", "o32")],
                                  v_mask_rle, [("dBits=misaligned", dict(dBits="_plus1"))]),
    "lerc_amd_mask_rle_decode_device": S([CTX, A("dRle", "vp", "ptr"), A("rleBytes", "u32", "nz"), A("dBits", "vp", "ptr"), A("nBytes", "u32", "nz")],
                                         v_mask_rle_decode, [("rleBytes=1", dict(rleBytes=1))]),
}

BY_ROLE = {"ptr": [None], "o32": [None], "o64": [None], "cnt": [0, -1], "nz": [0], "dt": [8], "err": [-1.0], "slot": [8, 0], "v": []}


def rows_of(name):
    """[(label, {argument: value})]: the valid call, one variation per role value, the mask rules and the dimensions beyond INT_MAX"""
    spec = SPECS[name]
    names = [a for a, _, _ in spec["args"]]
    rows = [] if spec["no_valid"] else [("valid", {})]
    for arg, _, role in spec["args"]:
        rows += [("%s=%s" % (arg, "NULL" if v is None else ("%g" % v)), {arg: v}) for v in BY_ROLE[role]]
    mask = next((a for a in names if a.endswith("ValidBytes")), None)
    if "nMasks" in names:
        if "nBands" in names:
            rows.append(("nMasks=2,nBands=3", {"nMasks": 2, "nBands": 3, mask: "_mask"}))
        rows.append(("nMasks=1,%s=NULL" % mask, {"nMasks": 1, mask: None}))
        rows.append(("nMasks=0,%s" % mask, {"nMasks": 0, mask: "_mask"}))
        rows.append(("nMasks=1,%s" % mask, {"nMasks": 1, mask: "_mask"}))
    if "nCols" in names and "nRows" in names:
        rows.append(("dims>INT_MAX", {k: BIG for k in ("nCols", "nRows", "tileCols", "tileRows") if k in names}))
    return rows + spec["extra"]


def run_rows(env, name):
    """-> ["label status out=0|kept|set ..."], the out facts for calls that refuse"""
    spec = SPECS[name]
    got, valid = [], None
    for label, change in rows_of(name):
        if valid is None or not spec["cached"]:
            valid = spec["valid"](env, name)
        vals = dict(valid)
        for k, v in change.items():
            if v == "_mask":
                vals.update(valid.get("_mask_with", {}))
                v = valid["_mask"]
            elif v == "_flags":
                v = env.host(np.array([1, 0, 0], np.uint8))
            elif v == "_plus1":
                v = valid[k] + 1
            vals[k] = v
        outs, args = {}, []
        for arg, ctype, role in spec["args"]:
            if role in ("o32", "o64") and arg not in change:
                outs[arg] = ct.c_uint(SENT32) if role == "o32" else ct.c_ulonglong(SENT64)
                args.append(ct.byref(outs[arg]))
            else:
                args.append(vals[arg])
        rc = env.call(name, args)
        if spec["drain"]:
            assert env.L.lerc_amd_finish(env.h, 0, None) == 0
        facts = []
        if rc != 0:
            for arg, o in outs.items():
                facts.append("%s=%s" % (arg, "0" if o.value == 0 else "kept" if o.value in (SENT32, SENT64) else "set"))
        elif label == "valid":
            assert all(o.value not in (SENT32, SENT64) for o in outs.values()), "a valid call left an out-parameter unwritten"
            if valid.get("_check"):
                valid["_check"]()
        got.append(" ".join([label, str(rc)] + facts))
    return got


def check(env, name):
    got, want = run_rows(env, name), [r.strip() for r in TABLE[name].split("|")]
    assert got == want, "\n".join("%-50s recorded: %s" % (g, w) for g, w in zip(got, want) if g != w) or (len(got), len(want))


def check_names_every_symbol():
    """every declared symbol that returns a status has rows, so has every SPECS entry, and the table names nothing else"""
    import os
    import re
    import test_capi_symbols
    hdrs = "".join(open(os.path.join(capi.ROOT, "include", h)).read() for h in ("lerc_amd.h", "lerc_amd_device.h"))
    status = set(re.findall(r"LERC_AMD_API\s+(?:lerc_status|unsigned\s+int)\s+(lerc_\w+)\s*\(", hdrs))
    assert status <= set(test_capi_symbols.declared_symbols())
    others = set(test_capi_symbols.declared_symbols()) - status
    assert all(re.search(r"LERC_AMD_API\s+(?:void|int|const\s+char\s*\*|lerc_amd_context\s*\*)\s*%s\s*\(" % s, hdrs) for s in others), others
    assert {n.split("@")[0] for n in TABLE} == status == {n.split("@")[0] for n in SPECS} and set(TABLE) == set(SPECS)


def n_rows():
    return sum(len(t.split("|")) for t in TABLE.values())


TABLE = {
    "lerc_computeCompressedSize":
        "valid 0 | pData=NULL 2 numBytes=0 | dataType=8 2 numBytes=0 | nDepth=0 2 numBytes=0 | nDepth=-1 2 numBytes=0 | nCols=0 2 numBytes=0 "
        "| nCols=-1 2 numBytes=0 | nRows=0 2 numBytes=0 | nRows=-1 2 numBytes=0 | nBands=0 2 numBytes=0 | nBands=-1 2 numBytes=0 | maxZErr=-1 "
        "2 numBytes=0 | numBytes=NULL 2 | nMasks=2,nBands=3 2 numBytes=0 | nMasks=1,pValidBytes=NULL 2 numBytes=0 | nMasks=0,pValidBytes 0 | "
        "nMasks=1,pValidBytes 0 | dims>INT_MAX 6 numBytes=0",
    "lerc_encode":
        "valid 0 | pData=NULL 2 nBytesWritten=0 | dataType=8 2 nBytesWritten=0 | nDepth=0 2 nBytesWritten=0 | nDepth=-1 2 nBytesWritten=0 | "
        "nCols=0 2 nBytesWritten=0 | nCols=-1 2 nBytesWritten=0 | nRows=0 2 nBytesWritten=0 | nRows=-1 2 nBytesWritten=0 | nBands=0 2 "
        "nBytesWritten=0 | nBands=-1 2 nBytesWritten=0 | maxZErr=-1 2 nBytesWritten=0 | pOutBuffer=NULL 2 nBytesWritten=0 | outBufferSize=0 2 "
        "nBytesWritten=0 | nBytesWritten=NULL 2 | nMasks=2,nBands=3 2 nBytesWritten=0 | nMasks=1,pValidBytes=NULL 2 nBytesWritten=0 | "
        "nMasks=0,pValidBytes 0 | nMasks=1,pValidBytes 0 | dims>INT_MAX 6 nBytesWritten=0",
    "lerc_computeCompressedSize_4D":
        "valid 0 | pData=NULL 2 numBytes=0 | dataType=8 2 numBytes=0 | nDepth=0 2 numBytes=0 | nDepth=-1 2 numBytes=0 | nCols=0 2 numBytes=0 "
        "| nCols=-1 2 numBytes=0 | nRows=0 2 numBytes=0 | nRows=-1 2 numBytes=0 | nBands=0 2 numBytes=0 | nBands=-1 2 numBytes=0 | maxZErr=-1 "
        "2 numBytes=0 | numBytes=NULL 2 | nMasks=2,nBands=3 2 numBytes=0 | nMasks=1,pValidBytes=NULL 2 numBytes=0 | nMasks=0,pValidBytes 0 | "
        "nMasks=1,pValidBytes 0 | dims>INT_MAX 6 numBytes=0 | pUsesNoData,noDataValues=NULL 2 numBytes=0",
    "lerc_encode_4D":
        "valid 0 | pData=NULL 2 nBytesWritten=0 | dataType=8 2 nBytesWritten=0 | nDepth=0 2 nBytesWritten=0 | nDepth=-1 2 nBytesWritten=0 | "
        "nCols=0 2 nBytesWritten=0 | nCols=-1 2 nBytesWritten=0 | nRows=0 2 nBytesWritten=0 | nRows=-1 2 nBytesWritten=0 | nBands=0 2 "
        "nBytesWritten=0 | nBands=-1 2 nBytesWritten=0 | maxZErr=-1 2 nBytesWritten=0 | pOutBuffer=NULL 2 nBytesWritten=0 | outBufferSize=0 2 "
        "nBytesWritten=0 | nBytesWritten=NULL 2 | nMasks=2,nBands=3 2 nBytesWritten=0 | nMasks=1,pValidBytes=NULL 2 nBytesWritten=0 | "
        "nMasks=0,pValidBytes 0 | nMasks=1,pValidBytes 0 | dims>INT_MAX 6 nBytesWritten=0 | pUsesNoData,noDataValues=NULL 2 nBytesWritten=0",
    "lerc_computeCompressedSizeForVersion":
        "valid 0 | pData=NULL 2 numBytes=0 | dataType=8 2 numBytes=0 | nDepth=0 2 numBytes=0 | nDepth=-1 2 numBytes=0 | nCols=0 2 numBytes=0 "
        "| nCols=-1 2 numBytes=0 | nRows=0 2 numBytes=0 | nRows=-1 2 numBytes=0 | nBands=0 2 numBytes=0 | nBands=-1 2 numBytes=0 | maxZErr=-1 "
        "2 numBytes=0 | numBytes=NULL 2 | nMasks=2,nBands=3 2 numBytes=0 | nMasks=1,pValidBytes=NULL 2 numBytes=0 | nMasks=0,pValidBytes 0 | "
        "nMasks=1,pValidBytes 0 | dims>INT_MAX 6 numBytes=0 | codecVersion=7 2 numBytes=0 | codecVersion=1 2 numBytes=0 | codecVersion=0 2 "
        "numBytes=0",
    "lerc_computeCompressedSizeForVersion@v3":
        "valid 0 | pData=NULL 2 numBytes=0 | dataType=8 2 numBytes=0 | nDepth=0 2 numBytes=0 | nDepth=-1 2 numBytes=0 | nCols=0 2 numBytes=0 "
        "| nCols=-1 2 numBytes=0 | nRows=0 2 numBytes=0 | nRows=-1 2 numBytes=0 | nBands=0 2 numBytes=0 | nBands=-1 2 numBytes=0 | maxZErr=-1 "
        "2 numBytes=0 | numBytes=NULL 2 | nMasks=2,nBands=3 2 numBytes=0 | nMasks=1,pValidBytes=NULL 2 numBytes=0 | nMasks=0,pValidBytes 0 | "
        "nMasks=1,pValidBytes 0 | dims>INT_MAX 6 numBytes=0",
    "lerc_encodeForVersion":
        "valid 0 | pData=NULL 2 nBytesWritten=0 | dataType=8 2 nBytesWritten=0 | nDepth=0 2 nBytesWritten=0 | nDepth=-1 2 nBytesWritten=0 | "
        "nCols=0 2 nBytesWritten=0 | nCols=-1 2 nBytesWritten=0 | nRows=0 2 nBytesWritten=0 | nRows=-1 2 nBytesWritten=0 | nBands=0 2 "
        "nBytesWritten=0 | nBands=-1 2 nBytesWritten=0 | maxZErr=-1 2 nBytesWritten=0 | pOutBuffer=NULL 2 nBytesWritten=0 | outBufferSize=0 2 "
        "nBytesWritten=0 | nBytesWritten=NULL 2 | nMasks=2,nBands=3 2 nBytesWritten=0 | nMasks=1,pValidBytes=NULL 2 nBytesWritten=0 | "
        "nMasks=0,pValidBytes 0 | nMasks=1,pValidBytes 0 | dims>INT_MAX 6 nBytesWritten=0 | codecVersion=7 2 nBytesWritten=0 | codecVersion=1 "
        "2 nBytesWritten=0 | codecVersion=0 2 nBytesWritten=0",
    "lerc_encodeForVersion@v3":
        "valid 0 | pData=NULL 2 nBytesWritten=0 | dataType=8 2 nBytesWritten=0 | nDepth=0 2 nBytesWritten=0 | nDepth=-1 2 nBytesWritten=0 | "
        "nCols=0 2 nBytesWritten=0 | nCols=-1 2 nBytesWritten=0 | nRows=0 2 nBytesWritten=0 | nRows=-1 2 nBytesWritten=0 | nBands=0 2 "
        "nBytesWritten=0 | nBands=-1 2 nBytesWritten=0 | maxZErr=-1 2 nBytesWritten=0 | pOutBuffer=NULL 2 nBytesWritten=0 | outBufferSize=0 2 "
        "nBytesWritten=0 | nBytesWritten=NULL 2 | nMasks=2,nBands=3 2 nBytesWritten=0 | nMasks=1,pValidBytes=NULL 2 nBytesWritten=0 | "
        "nMasks=0,pValidBytes 0 | nMasks=1,pValidBytes 0 | dims>INT_MAX 6 nBytesWritten=0",
    "lerc_getBlobInfo":
        "valid 0 | pLercBlob=NULL 2 | blobSize=0 2 | infoArraySize=0 0 | infoArraySize=-1 0 | dataRangeArraySize=0 0 | dataRangeArraySize=-1 "
        "0 | infoArray=NULL 0 | dataRangeArray=NULL 0 | infoArray,dataRangeArray=NULL 2 | bothSizes=0 2",
    "lerc_getDataRanges":
        "valid 0 | pLercBlob=NULL 2 | blobSize=0 2 | nDepth=0 2 | nDepth=-1 2 | nBands=0 2 | nBands=-1 2 | pMins=NULL 2 | pMaxs=NULL 2",
    "lerc_decode":
        "valid 0 | pLercBlob=NULL 2 | blobSize=0 2 | nDepth=0 2 | nDepth=-1 2 | nCols=0 2 | nCols=-1 2 | nRows=0 2 | nRows=-1 2 | nBands=0 2 "
        "| nBands=-1 2 | dataType=8 2 | pData=NULL 2 | nMasks=2,nBands=3 2 | nMasks=1,pValidBytes=NULL 2 | nMasks=0,pValidBytes 0 | "
        "nMasks=1,pValidBytes 0 | dims>INT_MAX 6",
    "lerc_decode_4D":
        "valid 0 | pLercBlob=NULL 2 | blobSize=0 2 | nDepth=0 2 | nDepth=-1 2 | nCols=0 2 | nCols=-1 2 | nRows=0 2 | nRows=-1 2 | nBands=0 2 "
        "| nBands=-1 2 | dataType=8 2 | pData=NULL 2 | nMasks=2,nBands=3 2 | nMasks=1,pValidBytes=NULL 2 | nMasks=0,pValidBytes 0 | "
        "nMasks=1,pValidBytes 0 | dims>INT_MAX 6",
    "lerc_decodeToDouble":
        "valid 0 | pLercBlob=NULL 2 | blobSize=0 2 | nDepth=0 2 | nDepth=-1 2 | nCols=0 2 | nCols=-1 2 | nRows=0 2 | nRows=-1 2 | nBands=0 2 "
        "| nBands=-1 2 | pData=NULL 2 | nMasks=2,nBands=3 2 | nMasks=1,pValidBytes=NULL 2 | nMasks=0,pValidBytes 0 | nMasks=1,pValidBytes 0 | "
        "dims>INT_MAX 1",
    "lerc_decodeToDouble_4D":
        "valid 0 | pLercBlob=NULL 2 | blobSize=0 2 | nDepth=0 2 | nDepth=-1 2 | nCols=0 2 | nCols=-1 2 | nRows=0 2 | nRows=-1 2 | nBands=0 2 "
        "| nBands=-1 2 | pData=NULL 2 | nMasks=2,nBands=3 2 | nMasks=1,pValidBytes=NULL 2 | nMasks=0,pValidBytes 0 | nMasks=1,pValidBytes 0 | "
        "dims>INT_MAX 1",
    "lerc_amd_encode_device":
        "valid 0 | ctx=NULL 2 nBytesWritten=kept | dData=NULL 2 nBytesWritten=0 | dataType=8 2 nBytesWritten=0 | nDepth=0 2 nBytesWritten=0 | "
        "nDepth=-1 2 nBytesWritten=0 | nCols=0 2 nBytesWritten=0 | nCols=-1 2 nBytesWritten=0 | nRows=0 2 nBytesWritten=0 | nRows=-1 2 "
        "nBytesWritten=0 | nBands=0 2 nBytesWritten=0 | nBands=-1 2 nBytesWritten=0 | maxZErr=-1 2 nBytesWritten=0 | nBytesWritten=NULL 2 | "
        "nMasks=2,nBands=3 2 nBytesWritten=0 | nMasks=1,dValidBytes=NULL 2 nBytesWritten=0 | nMasks=0,dValidBytes 0 | nMasks=1,dValidBytes 0 "
        "| dims>INT_MAX 6 nBytesWritten=0 | dOutBuffer=NULL 0",
    "lerc_amd_decode_device":
        "valid 0 | ctx=NULL 2 | dLercBlob=NULL 2 | blobSize=0 2 | nDepth=0 2 | nDepth=-1 2 | nCols=0 2 | nCols=-1 2 | nRows=0 2 | nRows=-1 2 "
        "| nBands=0 2 | nBands=-1 2 | dataType=8 2 | dData=NULL 2 | nMasks=2,nBands=3 2 | nMasks=1,dValidBytes=NULL 2 | nMasks=0,dValidBytes "
        "0 | nMasks=1,dValidBytes 0 | dims>INT_MAX 6",
    "lerc_amd_encode_device_async":
        "valid 0 | ctx=NULL 2 ticket=kept | dData=NULL 2 ticket=0 | dataType=8 2 ticket=0 | nDepth=0 2 ticket=0 | nDepth=-1 2 ticket=0 | "
        "nCols=0 2 ticket=0 | nCols=-1 2 ticket=0 | nRows=0 2 ticket=0 | nRows=-1 2 ticket=0 | nBands=0 2 ticket=0 | nBands=-1 2 ticket=0 | "
        "maxZErr=-1 2 ticket=0 | ticket=NULL 2 | nMasks=2,nBands=3 2 ticket=0 | nMasks=1,dValidBytes=NULL 2 ticket=0 | nMasks=0,dValidBytes 0 "
        "| nMasks=1,dValidBytes 0 | dims>INT_MAX 6 ticket=0 | dOutBuffer=NULL 0",
    "lerc_amd_decode_device_async":
        "valid 0 | ctx=NULL 2 ticket=kept | dLercBlob=NULL 2 ticket=0 | blobSizeBound=0 2 ticket=0 | nDepth=0 2 ticket=0 | nDepth=-1 2 "
        "ticket=0 | nCols=0 2 ticket=0 | nCols=-1 2 ticket=0 | nRows=0 2 ticket=0 | nRows=-1 2 ticket=0 | nBands=0 2 ticket=0 | nBands=-1 2 "
        "ticket=0 | dataType=8 2 ticket=0 | dData=NULL 2 ticket=0 | ticket=NULL 2 | nMasks=2,nBands=3 2 ticket=0 | nMasks=1,dValidBytes=NULL "
        "2 ticket=0 | nMasks=0,dValidBytes 0 | nMasks=1,dValidBytes 0 | dims>INT_MAX 6 ticket=0",
    "lerc_amd_finish":
        "valid 0 | ctx=NULL 2 nBytes=kept | nBytes=NULL 0 | ticket=unknown 2 nBytes=0",
    "lerc_amd_encode_tiles_device":
        "valid 0 | ctx=NULL 2 arenaUsed=kept | dTiles=NULL 2 arenaUsed=kept | dataType=8 2 arenaUsed=kept | nCols=0 2 arenaUsed=kept | "
        "nCols=-1 2 arenaUsed=kept | nRows=0 2 arenaUsed=kept | nRows=-1 2 arenaUsed=kept | nTiles=0 2 arenaUsed=kept | nTiles=-1 2 "
        "arenaUsed=kept | maxZErr=-1 2 arenaUsed=kept | dArena=NULL 2 arenaUsed=kept | offsets=NULL 2 arenaUsed=kept | sizes=NULL 2 "
        "arenaUsed=kept | arenaUsed=NULL 0 | dims>INT_MAX 6 arenaUsed=kept",
    "lerc_amd_decode_tiles_device":
        "valid 0 | ctx=NULL 2 | dArena=NULL 2 | offsets=NULL 2 | sizes=NULL 2 | nTiles=0 2 | nTiles=-1 2 | nCols=0 2 | nCols=-1 2 | nRows=0 2 "
        "| nRows=-1 2 | dataType=8 2 | dTiles=NULL 2 | dims>INT_MAX 6",
    "lerc_amd_encode_tiles_device_slots":
        "valid 0 | ctx=NULL 2 | dTiles=NULL 2 | dataType=8 2 | nCols=0 2 | nCols=-1 2 | nRows=0 2 | nRows=-1 2 | nTiles=0 2 | nTiles=-1 2 | "
        "maxZErr=-1 2 | dSlots=NULL 2 | slotBytes=8 2 | slotBytes=0 2 | sizes=NULL 2 | dims>INT_MAX 6",
    "lerc_amd_decode_tiles_device_slots":
        "valid 0 | ctx=NULL 2 | dSlots=NULL 2 | slotBytes=8 2 | slotBytes=0 2 | sizes=NULL 2 | nTiles=0 2 | nTiles=-1 2 | nCols=0 2 | "
        "nCols=-1 2 | nRows=0 2 | nRows=-1 2 | dataType=8 2 | dTiles=NULL 2 | dims>INT_MAX 6",
    "lerc_amd_encode_tiles_device_masked":
        "valid 0 | ctx=NULL 2 arenaUsed=kept | dTiles=NULL 2 arenaUsed=kept | dataType=8 2 arenaUsed=kept | nCols=0 2 arenaUsed=kept | "
        "nCols=-1 2 arenaUsed=kept | nRows=0 2 arenaUsed=kept | nRows=-1 2 arenaUsed=kept | nTiles=0 2 arenaUsed=kept | nTiles=-1 2 "
        "arenaUsed=kept | maxZErr=-1 2 arenaUsed=kept | dArena=NULL 2 arenaUsed=kept | slotBytes=8 2 arenaUsed=kept | slotBytes=0 0 | "
        "offsets=NULL 2 arenaUsed=kept | sizes=NULL 2 arenaUsed=kept | arenaUsed=NULL 0 | dims>INT_MAX 6 arenaUsed=kept | dValidBytes 0",
    "lerc_amd_decode_tiles_device_masked":
        "valid 0 | ctx=NULL 2 | dArena=NULL 2 | offsets=NULL 2 | sizes=NULL 2 | nTiles=0 2 | nTiles=-1 2 | nCols=0 2 | nCols=-1 2 | nRows=0 2 "
        "| nRows=-1 2 | dataType=8 2 | dTiles=NULL 2 | dims>INT_MAX 6 | dValidBytes 0",
    "lerc_amd_encode_tiles_device_bands":
        "valid 0 | ctx=NULL 2 arenaUsed=kept | dTiles=NULL 2 arenaUsed=kept | dataType=8 2 arenaUsed=kept | nCols=0 2 arenaUsed=kept | "
        "nCols=-1 2 arenaUsed=kept | nRows=0 2 arenaUsed=kept | nRows=-1 2 arenaUsed=kept | nBands=0 2 arenaUsed=kept | nBands=-1 2 "
        "arenaUsed=kept | nTiles=0 2 arenaUsed=kept | nTiles=-1 2 arenaUsed=kept | maxZErr=-1 2 arenaUsed=kept | dArena=NULL 2 arenaUsed=kept "
        "| slotBytes=8 2 arenaUsed=kept | slotBytes=0 0 | offsets=NULL 2 arenaUsed=kept | sizes=NULL 2 arenaUsed=kept | arenaUsed=NULL 0 | "
        "nMasks=2,nBands=3 2 arenaUsed=kept | nMasks=1,dValidBytes=NULL 2 arenaUsed=kept | nMasks=0,dValidBytes 2 arenaUsed=kept | "
        "nMasks=1,dValidBytes 0 | dims>INT_MAX 6 arenaUsed=kept",
    "lerc_amd_decode_tiles_device_bands":
        "valid 0 | ctx=NULL 2 | dArena=NULL 2 | offsets=NULL 2 | sizes=NULL 2 | nTiles=0 2 | nTiles=-1 2 | nCols=0 2 | nCols=-1 2 | nRows=0 2 "
        "| nRows=-1 2 | nBands=0 2 | nBands=-1 2 | dataType=8 2 | dTiles=NULL 2 | nMasks=2,nBands=3 2 | nMasks=1,dValidBytes=NULL 2 | "
        "nMasks=0,dValidBytes 2 | nMasks=1,dValidBytes 0 | dims>INT_MAX 6",
    "lerc_amd_encode_raster_tiles_device":
        "valid 0 | ctx=NULL 2 arenaUsed=0 | dRaster=NULL 2 arenaUsed=0 | dataType=8 2 arenaUsed=0 | nCols=0 2 arenaUsed=0 | nCols=-1 2 "
        "arenaUsed=0 | nRows=0 2 arenaUsed=0 | nRows=-1 2 arenaUsed=0 | nBands=0 2 arenaUsed=0 | nBands=-1 2 arenaUsed=0 | tileCols=0 2 "
        "arenaUsed=0 | tileCols=-1 2 arenaUsed=0 | tileRows=0 2 arenaUsed=0 | tileRows=-1 2 arenaUsed=0 | maxZErr=-1 2 arenaUsed=0 | "
        "dArena=NULL 2 arenaUsed=0 | slotBytes=8 2 arenaUsed=0 | slotBytes=0 0 | offsets=NULL 2 arenaUsed=0 | sizes=NULL 2 arenaUsed=0 | "
        "arenaUsed=NULL 0 | nMasks=2,nBands=3 2 arenaUsed=0 | nMasks=1,dValidBytes=NULL 2 arenaUsed=0 | nMasks=0,dValidBytes 2 arenaUsed=0 | "
        "nMasks=1,dValidBytes 0 | dims>INT_MAX 6 arenaUsed=0",
    "lerc_amd_decode_raster_tiles_device":
        "valid 0 | ctx=NULL 2 | dArena=NULL 2 | offsets=NULL 2 | sizes=NULL 2 | dataType=8 2 | nCols=0 2 | nCols=-1 2 | nRows=0 2 | nRows=-1 "
        "2 | nBands=0 2 | nBands=-1 2 | tileCols=0 2 | tileCols=-1 2 | tileRows=0 2 | tileRows=-1 2 | dRaster=NULL 2 | nMasks=2,nBands=3 2 | "
        "nMasks=1,dValidBytes=NULL 2 | nMasks=0,dValidBytes 2 | nMasks=1,dValidBytes 0 | dims>INT_MAX 6",
    "lerc_amd_encode_raster_tiles_device_strided":
        "valid 0 | ctx=NULL 2 arenaUsed=0 | dRaster=NULL 2 arenaUsed=0 | dataType=8 2 arenaUsed=0 | nCols=0 2 arenaUsed=0 | nCols=-1 2 "
        "arenaUsed=0 | nRows=0 2 arenaUsed=0 | nRows=-1 2 arenaUsed=0 | nBands=0 2 arenaUsed=0 | nBands=-1 2 arenaUsed=0 | tileCols=0 2 "
        "arenaUsed=0 | tileCols=-1 2 arenaUsed=0 | tileRows=0 2 arenaUsed=0 | tileRows=-1 2 arenaUsed=0 | maxZErr=-1 2 arenaUsed=0 | "
        "dArena=NULL 2 arenaUsed=0 | slotBytes=8 2 arenaUsed=0 | slotBytes=0 0 | offsets=NULL 2 arenaUsed=0 | sizes=NULL 2 arenaUsed=0 | "
        "arenaUsed=NULL 0 | nMasks=2,nBands=3 2 arenaUsed=0 | nMasks=1,dValidBytes=NULL 2 arenaUsed=0 | nMasks=0,dValidBytes 2 arenaUsed=0 | "
        "nMasks=1,dValidBytes 0 | dims>INT_MAX 6 arenaUsed=0",
    "lerc_amd_decode_raster_tiles_device_strided":
        "valid 0 | ctx=NULL 2 | dArena=NULL 2 | offsets=NULL 2 | sizes=NULL 2 | dataType=8 2 | nCols=0 2 | nCols=-1 2 | nRows=0 2 | nRows=-1 "
        "2 | nBands=0 2 | nBands=-1 2 | tileCols=0 2 | tileCols=-1 2 | tileRows=0 2 | tileRows=-1 2 | dRaster=NULL 2 | nMasks=2,nBands=3 2 | "
        "nMasks=1,dValidBytes=NULL 2 | nMasks=0,dValidBytes 2 | nMasks=1,dValidBytes 0 | dims>INT_MAX 6",
    "lerc_amd_encode_raster_tiles_device_range":
        "valid 0 | ctx=NULL 2 arenaUsed=0 | dRaster=NULL 2 arenaUsed=0 | dataType=8 2 arenaUsed=0 | nCols=0 2 arenaUsed=0 | nCols=-1 2 "
        "arenaUsed=0 | nRows=0 2 arenaUsed=0 | nRows=-1 2 arenaUsed=0 | nBands=0 2 arenaUsed=0 | nBands=-1 2 arenaUsed=0 | tileCols=0 2 "
        "arenaUsed=0 | tileCols=-1 2 arenaUsed=0 | tileRows=0 2 arenaUsed=0 | tileRows=-1 2 arenaUsed=0 | nTileCols=0 2 arenaUsed=0 | "
        "nTileCols=-1 2 arenaUsed=0 | nTileRows=0 2 arenaUsed=0 | nTileRows=-1 2 arenaUsed=0 | maxZErr=-1 2 arenaUsed=0 | dArena=NULL 2 "
        "arenaUsed=0 | slotBytes=8 2 arenaUsed=0 | slotBytes=0 0 | offsets=NULL 2 arenaUsed=0 | sizes=NULL 2 arenaUsed=0 | arenaUsed=NULL 0 | "
        "nMasks=2,nBands=3 2 arenaUsed=0 | nMasks=1,dValidBytes=NULL 2 arenaUsed=0 | nMasks=0,dValidBytes 2 arenaUsed=0 | "
        "nMasks=1,dValidBytes 0 | dims>INT_MAX 6 arenaUsed=0 | tileCol0=-1 2 arenaUsed=0 | tileRow0=-1 2 arenaUsed=0",
    "lerc_amd_decode_raster_window_device":
        "valid 0 | ctx=NULL 2 | dArena=NULL 2 | offsets=NULL 2 | sizes=NULL 2 | dataType=8 2 | nCols=0 2 | nCols=-1 2 | nRows=0 2 | nRows=-1 "
        "2 | nBands=0 2 | nBands=-1 2 | tileCols=0 2 | tileCols=-1 2 | tileRows=0 2 | tileRows=-1 2 | winCols=0 2 | winCols=-1 2 | winRows=0 "
        "2 | winRows=-1 2 | dWindow=NULL 2 | nMasks=2,nBands=3 2 | nMasks=1,dValidBytes=NULL 2 | nMasks=0,dValidBytes 2 | "
        "nMasks=1,dValidBytes 0 | dims>INT_MAX 6",
    "lerc_amd_gather_blobs":
        "ctx=NULL 2 | ncclComm=NULL 2",
    "lerc_amd_mask_rle_device":
        "valid 0 | ctx=NULL 2 size=kept | dBits=NULL 2 size=kept | nBytes=0 2 size=kept | dOut=NULL 2 size=kept | size=NULL 2 | "
        "dBits=misaligned 2 size=kept",
    "lerc_amd_mask_rle_decode_device":
        "valid 0 | ctx=NULL 2 | dRle=NULL 2 | rleBytes=0 2 | dBits=NULL 2 | nBytes=0 2 | rleBytes=1 2",
}


if __name__ == "__main__":
    sim = capi.sim()
    env = Env(sim.lib, M.HostMem())
    import textwrap
    print("TABLE = {")
    for name in SPECS:
        lines = textwrap.wrap(" | ".join(run_rows(env, name)), 132, break_long_words=False, break_on_hyphens=False)
        print('    "%s":\n        "%s",' % (name, ' "\n        "'.join(lines)))
    print("}")
    env.close()
