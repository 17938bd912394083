"""Shared by test_sim_raster_depth.py (CPU emulator library) and test_gpu_raster_depth.py (MI355X): a driver for
lerc_amd_encode_raster_tiles_device_depth / lerc_amd_decode_raster_tiles_device_depth (include/lerc_amd_depth.h) -- a pixel-interleaved
raster [H, W, C] with packed pixels, or a view of one with padded rows, cut into a grid of tiles and coded as blobs of nDepth = C.
The checker's word: every blob equals lerc_encode of that rectangle with nDepth = C; the way back restores pixels and mask and leaves
padding and everything beside the view alone."""
import ctypes as ct

import numpy as np

import capi
import tiles_depth_common as D

SENT = 0xA7


def bind(L):
    D.bind(L)
    vp, u64, u32, i = ct.c_void_p, ct.c_ulonglong, ct.c_uint, ct.c_int
    L.lerc_amd_encode_raster_tiles_device_depth.restype = u32
    L.lerc_amd_encode_raster_tiles_device_depth.argtypes = [vp, vp, u32, i, i, i, u64, u64, i, i, i, vp, u64, ct.c_double, vp, u64, u64, vp, vp, vp]
    L.lerc_amd_decode_raster_tiles_device_depth.restype = u32
    L.lerc_amd_decode_raster_tiles_device_depth.argtypes = [vp, vp, vp, vp, u32, i, i, i, u64, u64, i, i, vp, i, vp, u64]
    return L


class RasterDepth(D.DepthBatch):
    def __init__(self, L, mem):
        bind(L)
        D.DepthBatch.__init__(self, L, mem)

    def encode_raster(self, big, col0, w, mask_big, tile, e, slot_bytes=0, pixel_pitch=None):
        """big: [H, Wbig, C], the raster is its columns col0 .. col0 + w; mask_big [H, Wm] or None (its columns 0 .. w)
        -> (status, blobs in grid order, offsets, sizes)"""
        h, wbig, c = big.shape
        item = big.itemsize
        nty, ntx = (h + tile - 1) // tile, (w + tile - 1) // tile
        n = nty * ntx
        kr, pr = self.mem.up(big)
        km, pm = self.mem.up(mask_big) if mask_big is not None else (None, None)
        cap = n * slot_bytes if slot_bytes else n * (tile * tile * c * item + tile * tile + 2048)
        ka, pa = self.mem.empty(cap + 16)
        offs = np.zeros(n, np.uint64)
        sizes = np.zeros(n, np.uint32)
        used = ct.c_ulonglong(0)
        rc = self.L.lerc_amd_encode_raster_tiles_device_depth(self.h, pr + col0 * c * item, capi.dt_code(big.dtype), w, h, c, c if pixel_pitch is None else pixel_pitch,
                                                              wbig * c, tile, tile, 0 if mask_big is None else 1, pm, 0 if mask_big is None else mask_big.shape[1],
                                                              float(e), pa, cap, int(slot_bytes), offs.ctypes.data, sizes.ctypes.data, ct.byref(used))
        arena = self.mem.down(ka)
        assert arena[cap:].tolist() == [0xCD] * 16, "bytes behind the arena were written"
        assert self.mem.down(kr).tobytes() == np.ascontiguousarray(big).tobytes(), "the raster was written"
        blobs = [arena[int(offs[t]):int(offs[t]) + int(sizes[t])].tobytes() for t in range(n)] if rc == 0 else []
        return rc, blobs, offs, sizes

    def decode_raster(self, blobs, shape_big, col0, w, dtype, mask_cols, tile, pixel_pitch=None):
        """-> (status, [H, Wbig, C] as left behind (sentinel bytes where nothing was to be written), mask [H, mask_cols] or None)"""
        h, wbig, c = shape_big
        item = np.dtype(dtype).itemsize
        n = len(blobs)
        offs = np.zeros(n, np.uint64)
        at = 0
        for t, b in enumerate(blobs):
            offs[t] = at
            at += (len(b) + 15) & ~15
        arena = np.zeros(at + 64, np.uint8)
        for t, b in enumerate(blobs):
            arena[int(offs[t]):int(offs[t]) + len(b)] = np.frombuffer(b, np.uint8)
        sizes = np.array([len(b) for b in blobs], np.uint32)
        ka, pa = self.mem.up(arena)
        ko, po = self.mem.empty(h * wbig * c * item, fill=SENT)
        kv, pv = self.mem.empty(h * mask_cols, fill=SENT) if mask_cols else (None, None)
        rc = self.L.lerc_amd_decode_raster_tiles_device_depth(self.h, pa, offs.ctypes.data, sizes.ctypes.data, capi.dt_code(dtype), w, h, c,
                                                              c if pixel_pitch is None else pixel_pitch, wbig * c, tile, tile, po + col0 * c * item,
                                                              1 if mask_cols else 0, pv, mask_cols)
        out = self.mem.down(ko, h * wbig * c * item).view(dtype).reshape(h, wbig, c)
        mask = self.mem.down(kv, h * mask_cols).reshape(h, mask_cols) if mask_cols else None
        return rc, out, mask


def rects(h, w, tile):
    return [(y, min(h, y + tile), x, min(w, x + tile)) for y in range(0, h, tile) for x in range(0, w, tile)]


def check_raster(B, R, dtype, e, h, w, c, tile, with_mask, view, slotted=False, seed=3):
    rng = np.random.default_rng(seed)
    dtype = np.dtype(dtype)
    pad0, pad1 = (5, 3) if view else (0, 0)    # (columns of the larger tensor in front of and behind the view)
    wbig = pad0 + w + pad1
    big = D.tiles_of(rng, 1, h, wbig, c, dtype)[0]
    mask_cols = (w + 7) if with_mask else 0    # (a mask with a pitch of its own)
    mask_big = None
    if with_mask:
        mask_big = np.zeros((h, mask_cols), np.uint8)
        mask_big[:, :w] = D.random_blob_mask(rng, 1, h, w)[0]
        mask_big[:20, :20] = 0    # (a tile's worth of the first tile partly invalid, whatever the blobs did)
    ras = big[:, pad0:pad0 + w]
    want = []
    for y0, y1, x0, x1 in rects(h, w, tile):
        rc, blob = R.encode(np.ascontiguousarray(ras[y0:y1, x0:x1]), e, n_depth=c, mask=None if mask_big is None else np.ascontiguousarray(mask_big[y0:y1, x0:x1]))
        assert rc == 0
        want.append(blob)
    slot = (tile * tile * c * dtype.itemsize + tile * tile + 2048 + 15) & ~15 if slotted else 0
    c0 = B.counters()
    rc, blobs, offs, sizes = B.encode_raster(big, pad0, w, mask_big, tile, e, slot_bytes=slot)
    c1 = B.counters()
    assert rc == 0, (rc, B.note())
    for t in range(len(want)):
        assert blobs[t] == want[t], "tile %d: %d bytes, the reference makes %d (%s)" % (t, len(blobs[t]), len(want[t]), B.note())
    assert (c1[0] - c0[0], c1[1] - c0[1]) == (len(want), 0), (c0, c1, B.note())
    if slotted:
        assert sorted(int(o) for o in offs) == [t * slot for t in range(len(want))]
    # ---- the way back
    rc, out, mask = B.decode_raster(want, (h, wbig, c), pad0, w, dtype, mask_cols, tile)
    assert rc == 0, (rc, B.note())
    for t, (y0, y1, x0, x1) in enumerate(rects(h, w, tile)):
        rc_r, p_r, m_r = R.decode(want[t], want_masks=1 if with_mask else 0)
        assert rc_r == 0
        assert out[y0:y1, pad0 + x0:pad0 + x1].tobytes() == p_r.reshape(y1 - y0, x1 - x0, c).tobytes(), "tile %d: pixels" % t
        if with_mask:
            assert np.array_equal(mask[y0:y1, x0:x1], m_r.reshape(y1 - y0, x1 - x0)), "tile %d: mask" % t
    raw = out.view(np.uint8).reshape(h, wbig * c * dtype.itemsize)
    lo, hi = pad0 * c * dtype.itemsize, (pad0 + w) * c * dtype.itemsize
    assert (raw[:, :lo] == SENT).all() and (raw[:, hi:] == SENT).all(), "bytes beside the view were written"
    if with_mask:
        assert (mask[:, w:] == SENT).all(), "the mask's padding was written"


# ---- the boundary: status rows of the two raster entry points.  A good call: a 16 x 16 x 3 uint16 raster, packed, tiles of 8 x 8,
# no mask.  (row name, what differs from the good call, status); every row is asked of both calls unless it names an argument only the
# encode has (maxZErr, slotBytes)
OK = dict(ctx=1, raster=1, arena=1, offs=1, sizes=1, dt=3, w=16, h=16, d=3, pp=3, rp=48, tc=8, tr=8, nm=0, mask=0, mp=0, e=0.0, slot=0)
TABLE = [
    ("no context", dict(ctx=0), 2), ("no raster", dict(raster=0), 2), ("no arena", dict(arena=0), 2), ("no offsets", dict(offs=0), 2),
    ("no sizes", dict(sizes=0), 2), ("a mask counted but not given", dict(nm=1, mp=16), 2), ("a mask given but not counted", dict(mask=1, mp=16), 2),
    ("nCols 0", dict(w=0), 2), ("nCols -1", dict(w=-1), 2), ("nRows 0", dict(h=0), 2), ("nRows -5", dict(h=-5), 2),
    ("tileCols 0", dict(tc=0), 2), ("tileRows -1", dict(tr=-1), 2), ("nDepth 0", dict(d=0, pp=0), 2), ("nDepth -1", dict(d=-1), 2),
    ("a type that is none", dict(dt=8), 2),
    ("RGB out of RGBA: pixelPitch above nDepth", dict(pp=4, rp=64), 2), ("pixelPitch below nDepth", dict(pp=2), 2), ("pixelPitch 1", dict(pp=1), 2),
    ("rows that overlap", dict(rp=47), 2), ("a mask pitch below nCols", dict(nm=1, mask=1, mp=15), 2),
    ("maxZErr < 0", dict(e=-1.0), 2), ("slotBytes 24", dict(slot=24), 2),
    ("a tile beyond INT_MAX", dict(w=65536, h=65536, rp=65536 * 3, tc=65536, tr=65536), 6),
    ("a tile beyond INT_MAX by its depth", dict(w=32768, h=32768, d=4, pp=4, rp=32768 * 4, tc=32768, tr=32768), 6),
    ("nDepth 0 beside a tile beyond INT_MAX", dict(w=65536, h=65536, d=0, pp=0, rp=65536 * 3, tc=65536, tr=65536), 2),
]


def check_refused(B):
    big = np.zeros((16, 16, 4), np.uint16)
    kr, pr = B.mem.up(big)
    ka, pa = B.mem.empty(1 << 16)
    km, pm = B.mem.up(np.ones((16, 16), np.uint8))
    offs = np.zeros(16, np.uint64)
    sizes = np.zeros(16, np.uint32)
    for name, change, status in TABLE:
        a = dict(OK, **change)
        h = B.h if a["ctx"] else None
        ras, arena, mask = (pr if a["raster"] else None), (pa if a["arena"] else None), (pm if a["mask"] else None)
        po, ps = (offs.ctypes.data if a["offs"] else None), (sizes.ctypes.data if a["sizes"] else None)
        rc = B.L.lerc_amd_encode_raster_tiles_device_depth(h, ras, a["dt"], a["w"], a["h"], a["d"], a["pp"], a["rp"], a["tc"], a["tr"], a["nm"], mask, a["mp"], a["e"],
                                                           arena, 1 << 16, a["slot"], po, ps, None)
        assert rc == status, (name, "encode", rc, status)
        if "e" in change or "slot" in change:
            continue
        rc = B.L.lerc_amd_decode_raster_tiles_device_depth(h, arena, po, ps, a["dt"], a["w"], a["h"], a["d"], a["pp"], a["rp"], a["tc"], a["tr"], ras, a["nm"], mask, a["mp"])
        assert rc == status, (name, "decode", rc, status)
