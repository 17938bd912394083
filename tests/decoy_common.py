"""Block streams seeded with DECOY block headers: legitimate Lerc2 blobs whose pixel payloads spell out complete, mutually consistent
block headers, aimed at the speculative decoders (tile_fast_decode_scan.hip guesses block starts from byte patterns; the two walking
tiers behind it start walks from headers found in windows).  Shared by test_sim_decoys.py (emulator) and test_gpu_decoys.py.

Three parts:
  * the STREAM MODEL (`model`): a plain restatement of Lerc2::ReadTiles' walk and of the scan's candidate rules -- true block starts,
    candidates, survivors (START & END), false survivors, with their blob offsets.  It never calls the library under test: it is the
    precondition checker ("the stream really holds the false survivors the case is about"), not an oracle for pixels;
  * the GENERATOR (`Layout`, `generate`): a raster whose 8 x 8 blocks are all bit-stuffed at exactly nb bits with block minimum 0, so
    every block has the same known length and block k begins at dataBegin + (sum of the lengths in front): byte strings can be laid
    into payloads at exact blob offsets (from codec 3 on a payload is one little-endian bit stream: BitStuffer2.cpp:476-540).  Single
    blocks may be made raw, constant or all zero;
  * the PLANS and CHECKS (`build_case`, `check_decoy_case`, `check_tiers`).
The piece size is a parameter: the emulator build stages 8 KiB pieces, the device 32 KiB."""
import struct

import numpy as np

import capi

DT_SIZE = [1, 1, 2, 2, 4, 4, 4, 8]


def type_used(dt, tc):
    """Lerc2.h:528-542: the type a block's offset is stored in, -1: no such type"""
    if dt in (2, 4):
        r = dt - tc
    elif dt in (3, 5):
        r = dt - 2 * tc
    elif dt == 6:
        return 6 if tc == 0 else (2 if tc == 1 else 1)
    elif dt == 7:
        r = dt if tc == 0 else dt - 2 * tc + 1
    else:
        return dt
    return r if 0 <= r <= 7 else -1


def off_bytes(dt):
    """offset type code -> bytes of the offset (0: the data type has no such offset type)"""
    return [DT_SIZE[type_used(dt, tc)] if type_used(dt, tc) >= 0 else 0 for tc in range(4)]


def sig_ok(prev, cur, pattern):
    step = 2 if pattern == 14 else 1
    return cur == prev or cur == ((prev + step) & pattern) or cur == 0


def _define(name):
    """the values tile_fast.h gives the macro `name`, in the file's order (emulator builds first), whatever the spacing"""
    import os
    import re
    text = open(os.path.join(capi.ROOT, "lerc_amd", "csrc", "tile_fast.h")).read()
    return [int(v) for v in re.findall(r"^\s*#\s*define\s+%s\s+(\d+)" % name, text, re.M)]


def scan_piece(emulator):
    """bytes of a scanning decoder's piece: the emulator build's (LERC_SMALL_GROUPS, which the Makefile's sim target sets) or the device's"""
    import os
    import re
    small, full = _define("LERC_SCAN_PIECE")
    sim_flags = re.search(r"^SIM_FLAGS\s*:?=.*$", open(os.path.join(capi.ROOT, "lerc_amd", "csrc", "Makefile")).read(), re.M).group(0)
    assert small < full and "LERC_SMALL_GROUPS" in sim_flags
    return small if emulator else full


def scan_pre(tb):
    """bytes staged in front of a piece's own (tile_fast.h: scanPre)"""
    return (2 * (2 + 64 * tb) + 31) & ~31


# ------------------------------------------------------------------------------------------------------------------ the stream model
class Model:
    pass


def model(blob, dtype, rows, cols, mask=None):
    """-> Model: version, data_begin, starts (true block starts, walked as Lerc2::ReadTiles does), cands [(begin, end)], survivors,
    false_survivors (sorted blob offsets), missing (true starts that are no survivors).  One value a pixel; mask: the band's valid pixels
    (the masked scan, MODE 1, takes count bytes 1 ... 64)."""
    b = np.frombuffer(blob, np.uint8)
    n = len(b)
    dt = capi.dt_code(dtype)
    tb = DT_SIZE[dt]
    assert bytes(blob[:6]) == b"Lerc2 "
    version = struct.unpack_from("<i", blob, 6)[0]
    assert version >= 4, version
    n_rows, n_cols, n_depth, n_valid, micro, blob_size, dt_blob = struct.unpack_from("<7i", blob, 14)
    valid = np.ones((rows, cols), bool) if mask is None else np.asarray(mask) != 0
    assert (n_rows, n_cols, n_depth, n_valid, micro, blob_size, dt_blob) == (rows, cols, 1, int(valid.sum()), 8, n, dt)
    hdr = 90 if version >= 6 else 66
    mask_bytes = struct.unpack_from("<i", blob, hdr)[0]
    assert (mask_bytes == 0) == (mask is None), "mask bytes"
    data_begin = hdr + 4 + mask_bytes + 2 * tb + 1
    assert b[data_begin - 1] == 0, "the band is stored in one sweep"
    v5 = version >= 5
    pattern = 14 if v5 else 15
    ob = off_bytes(dt)
    # the true path
    starts = []
    pos = data_begin
    for bi in range((rows + 7) // 8):
        for bj in range((cols + 7) // 8):
            n_el = int(valid[8 * bi:8 * bi + 8, 8 * bj:8 * bj + 8].sum())
            f = int(b[pos])
            assert n_el or f & 3 == 2, ("a block without a valid pixel", pos, f)
            assert (f >> 2) & pattern == bj & pattern and not (v5 and f & 4), ("signature", pos, f)
            starts.append(pos)
            mode, tc = f & 3, f >> 6
            if mode == 0:
                pos += 1 + n_el * tb
            elif mode == 2:
                pos += 1
            elif mode == 3:
                assert ob[tc]
                pos += 1 + ob[tc]
            else:
                assert ob[tc]
                t = int(b[pos + 1 + ob[tc]])
                nb = t & 31
                assert t >> 6 == 2 and int(b[pos + 2 + ob[tc]]) == n_el and nb, (pos, t)
                if t & 32:
                    nl = int(b[pos + 3 + ob[tc]]) - 1
                    pos += 4 + ob[tc] + (nl * nb + 7) // 8 + (n_el * nl.bit_length() + 7) // 8
                else:
                    pos += 3 + ob[tc] + (n_el * nb + 7) // 8
    assert pos == n, (pos, n)
    # the scan's candidates (tile_fast_decode_scan.hip: candidate)
    wl, hl = cols & 7, rows & 7
    counts = {64}
    if hl:
        counts.add(8 * hl)
    if wl and wl != hl:
        counts.add(8 * wl)
    if mask is not None:
        counts = set(range(1, 65))
    hit = np.isin(b[1:], sorted(counts)) & ((b[:-1] & 0xC0) == 0x80) & ((b[:-1] & 31) != 0)
    cands = []
    for q in (np.nonzero(hit)[0] + 1).tolist():
        t = int(b[q - 1])
        nb, lut, cnt = t & 31, (t >> 5) & 1, int(b[q])
        if lut:
            nl = ((int(b[q + 1]) if q + 1 < n else 0) - 1) & 0xFF
            if not 1 <= nl <= 254:
                continue
            payload = 1 + (nl * nb + 7) // 8 + (cnt * nl.bit_length() + 7) // 8
        else:
            payload = (cnt * nb + 7) // 8
        for tc in range(4):
            if not ob[tc]:
                continue
            p = q - 2 - ob[tc]
            if p < data_begin:
                continue
            f = int(b[p])
            if f & 3 != 1 or f >> 6 != tc or (v5 and f & 4):
                continue
            ln = 3 + ob[tc] + payload
            e = p + ln
            if ln > 1 + cnt * tb or e > n:
                continue
            if e < n:
                nf = int(b[e])
                if not sig_ok((f >> 2) & pattern, (nf >> 2) & pattern, pattern) or (v5 and nf & 4):
                    continue
            cands.append((p, e))
    begins = {p for p, _ in cands} | {data_begin}
    ends = {e for _, e in cands} | {data_begin}
    m = Model()
    m.version, m.data_begin, m.starts, m.cands = version, data_begin, starts, cands
    m.survivors = sorted(begins & ends)
    true = set(starts)
    m.false_survivors = [p for p in m.survivors if p not in true]
    m.missing = [p for p in starts if p not in begins or p not in ends]
    return m


def per_piece(positions, piece):
    out = {}
    for p in positions:
        out[p // piece] = out.get(p // piece, 0) + 1
    return out


# ---------------------------------------------------------------------------------------------------------------------- the generator
class Layout:
    """Where the blocks of a (rows x cols) raster of `dtype` lie in the blob if every block is bit-stuffed at nb bits with minimum 0
    (offset: one byte) -- but for `kinds`: {block index: "raw" | "zero" | ("const", v)} (v a whole number 1 ... 255).  Rows / columns
    that are no multiples of 8 (edge blocks hold fewer values; one that would be no shorter bit-stuffed is raw) and a `mask` (a block
    holds its valid pixels; none: one byte; mask_bytes: what the mask takes in the blob) are the generator's two further parameters."""

    def __init__(self, dtype, rows, cols, nb, kinds=None, mask=None, mask_bytes=0):
        self.dtype, self.rows, self.cols, self.nb = np.dtype(dtype), rows, cols, nb
        self.dt = capi.dt_code(dtype)
        self.tb = DT_SIZE[self.dt]
        self.kinds = dict(kinds or {})
        self.mask = None if mask is None else np.asarray(mask) != 0
        self.nbr, self.nbc = (rows + 7) // 8, (cols + 7) // 8
        self.n_blocks = self.nbr * self.nbc
        self.data_begin = 90 + 4 + mask_bytes + 2 * self.tb + 1            # codec 6
        self.stuffed_len = 4 + 8 * nb
        assert self.stuffed_len < 1 + 64 * self.tb, "longer than the raw form"
        self.byte_tc = [tc for tc in range(4) if type_used(self.dt, tc) == 1][0]    # the offset type "one unsigned byte"
        lens, self.coords = [], []
        for k in range(self.n_blocks):
            i0, j0 = 8 * (k // self.nbc), 8 * (k % self.nbc)
            ii, jj = np.meshgrid(np.arange(i0, min(i0 + 8, rows)), np.arange(j0, min(j0 + 8, cols)), indexing="ij")
            ii, jj = ii.ravel(), jj.ravel()
            if self.mask is not None:
                keep = self.mask[ii, jj]
                ii, jj = ii[keep], jj[keep]
            self.coords.append((ii, jj))
            n = len(ii)
            kind = self.kinds.get(k)
            if n == 0:
                kind = self.kinds[k] = "zero"
            elif kind is None and 4 + (n * nb + 7) // 8 >= 1 + n * self.tb:
                kind = self.kinds[k] = "raw"
            assert kind in (None, "raw") or n in (0, 64)
            lens.append(4 + (n * nb + 7) // 8 if kind is None else 1 + n * self.tb if kind == "raw" else 1 if kind == "zero" else 2)
        self.n_el = np.array([len(c[0]) for c in self.coords])
        self.lens = np.array(lens)
        self.starts = self.data_begin + np.concatenate([[0], np.cumsum(self.lens)[:-1]])
        self.blob_len = int(self.data_begin + self.lens.sum())

    def sig(self, k):
        return (k % self.nbc) & 14

    def payload(self, k):
        """blob offsets [begin, end) of the bytes of block k that the pixels decide freely"""
        kind = self.kinds.get(k)
        s = int(self.starts[k])
        if kind is None:
            return s + 4, s + int(self.lens[k])
        assert kind == "raw"
        return s + 1, s + int(self.lens[k])

    def block_at(self, off):
        return int(np.searchsorted(self.starts, off, side="right")) - 1

    def stuffed_blocks_in_piece(self, piece, i, n_min=64):
        """the plain bit-stuffed blocks (of n_min values at least) that lie inside piece i whole"""
        return [k for k in range(self.n_blocks) if self.kinds.get(k) is None and self.n_el[k] >= n_min and self.starts[k] >= i * piece
                and self.starts[k] + self.lens[k] <= (i + 1) * piece]


def generate(lay, plan, seed, control=False):
    """-> (raster of quantised values, the block stream it has to encode to).  plan: [(blob offset, bytes)], each inside one block's
    payload.  control: the decoy bytes are left as filler (the same filler, the same pixels everywhere else)."""
    rng = np.random.default_rng(seed)
    total = lay.blob_len - lay.data_begin
    stream = rng.integers(0, 256, total, dtype=np.uint8)
    if lay.mask is not None:
        # (a masked band's scan takes any count 1 ... 64 behind a bits byte: filler without bytes 10...... holds no accidental candidate)
        stream[(stream & 0xC0) == 0x80] &= 0x3F
    planned = np.zeros(total, bool)
    for off, bs in plan:
        k = lay.block_at(off)
        lo, hi = lay.payload(k)
        assert lo <= off and off + len(bs) <= hi, ("a decoy leaves its host's payload", off, len(bs), lo, hi)
        r = off - lay.data_begin
        assert not planned[r:r + len(bs)].any(), ("decoys overlap", off)
        planned[r:r + len(bs)] = True
        if not control:
            stream[r:r + len(bs)] = np.frombuffer(bytes(bs), np.uint8)
    nb, tb = lay.nb, lay.tb
    q = np.zeros((lay.rows, lay.cols), np.int64)
    top_draw = rng.integers(0, 1 << (nb - 1), lay.n_blocks)
    for k in range(lay.n_blocks):
        kind = lay.kinds.get(k)
        s = int(lay.starts[k]) - lay.data_begin
        flag_sig = lay.sig(k) << 2
        n = int(lay.n_el[k])
        if kind == "zero":
            stream[s] = 2 | flag_sig
            continue
        if kind is not None and kind != "raw":
            v = int(kind[1])
            assert 1 <= v <= 255
            stream[s] = 3 | flag_sig | (lay.byte_tc << 6)
            stream[s + 1] = v
            q[lay.coords[k]] = v * 50 if lay.dtype.kind == "f" else v      # (floats: q at MaxZError 0.01)
            continue
        lo, hi = lay.payload(k)
        lo -= lay.data_begin; hi -= lay.data_begin
        width = 8 * tb if kind == "raw" else nb
        bits = np.unpackbits(stream[lo:hi], bitorder="little")[:n * width].reshape(n, width).astype(np.int64)
        v = (bits << np.arange(width)).sum(axis=1)
        # one value 0 and one with the top bit set keep nb what it is (a raw block: the full range); in values no decoy byte touches
        free = [i for i in range(n) if not planned[lo + (i * width) // 8: lo + ((i + 1) * width - 1) // 8 + 1].any()]
        assert len(free) >= 2, ("no room for the block's smallest and largest value", k)
        v[free[0]] = 0
        v[free[-1]] = (1 << width) - 1 if kind == "raw" else (1 << (nb - 1)) | int(top_draw[k])
        q[lay.coords[k]] = v
        packed = np.packbits(((v[:, None] >> np.arange(width)) & 1).astype(np.uint8).ravel(), bitorder="little")    # (the last byte's spare bits: 0)
        assert len(packed) == hi - lo
        for off, bs in ([] if control else plan):      # (the two values set above lie outside every decoy)
            r = off - lay.data_begin
            if lo <= r < hi:
                assert bytes(packed[r - lo:r - lo + len(bs)]) == bytes(bs), "a decoy reaches into the spare bits of a payload's last byte"
        stream[lo:hi] = packed
        if kind == "raw":
            stream[s] = flag_sig
        else:
            stream[s:s + 4] = [1 | flag_sig | (lay.byte_tc << 6), 0, 0x80 | nb, n]
    return q, stream


def to_raster(lay, q, max_z_err):
    if lay.dtype.kind == "f":
        return (q.astype(np.float64) * (2.0 * max_z_err)).astype(lay.dtype)    # q < 2^20: the quantiser returns q exactly
    if lay.dtype.kind == "i" and "raw" in lay.kinds.values():
        return q.astype(np.dtype("u%d" % lay.tb)).view(lay.dtype)
    return q.astype(lay.dtype)


# ------------------------------------------------------------------------------------------------------------------------ decoys
def decoy(dt, tc, sig, rng, nbd=1, lut=None, count=64):
    """A complete bit-stuffed block header and as many payload bytes as it claims: flag (mode 1, offset type tc, signature sig), offset,
    bits byte 10?nnnnn, count [, table size + 1 = lut, table, indices].  The filler holds no byte that reads like a count or bits byte."""
    ob = off_bytes(dt)[tc] or 1      # (an offset type the data type does not have: laid out as if it had one byte)
    head = [1 | (sig << 2) | (tc << 6)] + rng.integers(0, 0x40, ob).tolist() + [0x80 | (0x20 if lut is not None else 0) | nbd, count]
    if lut is not None:
        nl = (lut - 1) & 0xFF
        n_pay = 1 + (nl * nbd + 7) // 8 + (count * nl.bit_length() + 7) // 8 if 1 <= nl <= 254 else 1 + 8 * nbd
        body = [lut] + rng.integers(0, 0x40, n_pay - 1).tolist()
    else:
        body = rng.integers(0, 0x40, (count * nbd + 7) // 8).tolist()
    return bytes(head + body)


def chain_bytes(dt, n, sig, rng, tc=None, nbd=1, lut=None, end=True, count=64):
    """n decoys back to back -- each begins where the one in front ends: all but the first are SURVIVORS -- and, unless the chain is to
    end with its host (end=False), four bytes the last decoy's signature goes on into (a block row begins) that are no block: a
    bit-stuffed block's flag byte with a bits byte of 0.  -> (bytes, where each decoy begins)"""
    byte_tc = [t for t in range(4) if type_used(dt, t) == 1][0]
    if tc is None:
        tc = byte_tc
    ds = [decoy(dt, tc, sig, rng, nbd, lut, count) for _ in range(n)]
    rel = [sum(len(d) for d in ds[:i]) for i in range(n)]
    return b"".join(ds) + (bytes([1 | (byte_tc << 6), 0, 0, 0]) if end else b""), rel


class Case:
    pass


def shape_for(dtype, piece):
    """-> (shape, bits a value, MaxZError): 3 to 5 pieces of stream"""
    small = piece < 32768
    if np.dtype(dtype) == np.uint16:
        return ((64, 256) if small else (256, 256)), 15, 0.0
    if np.dtype(dtype) == np.int32:
        return ((32, 256) if small else (160, 256)), 30, 0.0
    return ((48, 256), 20, 0.01) if small else ((192, 256), 19, 0.01)


PLANS = ["mid", "ends-with-host", "boundary", "boundary-host", "tail", "lut", "offset-types", "crowd", "under-cap", "raw-host", "flat-run", "long-chain", "ragged", "masked"]
DTYPES = {"u16": np.uint16, "i32": np.int32, "f32": np.float32}
FLOAT_BITS = {"f32b18": 18, "f32b19": 19, "f32b20": 20}       # float32 at MaxZError 0.01 with 18, 19 and 20 bits a value (the mid plan)
CHUNK = _define("LERC_CHUNK_BYTES")[0]      # the walking tiers' chunk (tile_fast.h; the one-launch decoder walks sub-chunks of half of it)


def case_names():
    out = []
    for plan in PLANS:
        for d in DTYPES:
            if plan == "raw-host" and d != "u16":       # (a raw block's bytes ARE the pixels: any byte string is a uint16 raster; floats would have to dodge NaN)
                continue
            if plan == "long-chain" and d == "u16":     # (a uint16 payload, 120 bytes, holds no chain of more than nine decoys)
                continue
            out.append(f"{plan}-{d}")
    return out + [f"mid-{d}" for d in FLOAT_BITS]


def _plan(name, lay, piece, rng):
    """-> (plan [(offset, bytes)], offsets where the plan promises a false survivor, extra: dict of things the checks look at)"""
    dt = lay.dt
    plan, promised, extra = [], [], {}
    n_pieces = (lay.blob_len + piece - 1) // piece
    dlen = 12      # a decoy with a one-byte offset at 1 bit a value

    def lay_chain(off, n, sig, **kw):
        bs, rel = chain_bytes(dt, n, sig, rng, **kw)
        plan.append((off, bs))
        promised.extend(off + r for r in rel[1:])

    def blocks(i):
        ks = lay.stuffed_blocks_in_piece(piece, i)
        assert len(ks) >= 12, (i, len(ks))
        return ks

    if name == "mid":
        # chains of 2, 3 and 8 decoys in the middle of real payloads, two or three hosts a piece
        for i in range(n_pieces - 1):
            ks = blocks(i)
            if i % 2 == 0:
                lay_chain(lay.payload(ks[3])[0] + 5, 2, 6)
                lay_chain(lay.payload(ks[6])[0] + 9, 3, 10)
                lay_chain(lay.payload(ks[-2])[0] + 7, 2, 0)
            else:
                lay_chain(lay.payload(ks[len(ks) // 2])[0] + 6, 8, 4)
    elif name == "ends-with-host":
        # the chain's last decoy ends where its host ends: the real next block has END set twice, and the false chain tiles into the path
        for i in range(n_pieces - 1):
            ks = blocks(i)
            for k, n in ((ks[4], 3), (ks[-3], 2)):
                hi = lay.payload(k)[1]
                lay_chain(hi - n * dlen, n, lay.sig(k + 1), end=False)
    elif name == "boundary":
        # a chain that straddles a piece's first own byte: its survivors are the last ones in front of the piece and the first ones in it
        hit = []
        for m in range(1, n_pieces):
            x = m * piece
            k = lay.block_at(x)
            lo, hi = lay.payload(k)
            if lay.kinds.get(k) is None and lo + 30 <= x and x + 42 + 4 <= hi - 6:
                lay_chain(x - 30, 6, 8)         # decoys at x - 30, - 18, - 6 | + 6, + 18, + 30
                hit.append(x)
        assert hit, "no piece boundary lies in the middle of a payload: another shape"
        extra["boundaries"] = hit
    elif name == "boundary-host":
        # the host's header lies in front of a piece's first own byte, and a chain just behind that byte ends with the host: the piece's
        # first survivors are false ones that TILE into the path -- only the survivors in front of the own bytes (true ones) say so
        hit = []
        for m in range(1, n_pieces):
            x = m * piece
            k = lay.block_at(x)
            lo, hi = lay.payload(k)
            if lay.kinds.get(k) is None and lo <= x <= hi - 3 * dlen and hi - 4 * dlen >= lo + 8:
                lay_chain(hi - 4 * dlen, 4, lay.sig(k + 1), end=False)      # (its three survivors lie in the piece's own bytes)
                hit.append(x)
        assert hit, "no piece boundary with a payload's last 48 bytes behind it: another shape"
        extra["boundaries"] = hit
    elif name == "tail":
        # in the stream's last block: a chain that ends with the blob, and a decoy whose length runs past the blob's end
        k = lay.n_blocks - 1
        lo, hi = lay.payload(k)
        assert hi == lay.blob_len
        lay_chain(hi - 3 * dlen, 3, 2, end=False)
        bs, _ = chain_bytes(dt, 1, 2, rng, end=False)
        past = decoy(dt, lay.byte_tc, 2, rng, nbd=12)[:16]            # claims 100 bytes: 52 are left
        plan.append((hi - 3 * dlen - 16 - dlen, bs + past))
        extra["not_candidates"] = [hi - 3 * dlen - 16]
        lay_chain(lay.payload(blocks(n_pieces - 2)[5])[0] + 6, 3, 12)
        # and bytes BEHIND the blob, in a buffer longer than the blob (the last piece stages them): the chain of the last block goes on
        # there -- three more decoys and filler.  Nothing behind the blob's end is a block: e <= blobRel, and units behind it are not scanned
        extra["behind"] = chain_bytes(dt, 3, 2, rng)[0] + bytes(rng.integers(0, 256, 600, dtype=np.uint8))
    elif name == "lut":
        ks = blocks(1)
        lay_chain(lay.payload(ks[2])[0] + 6, 3, 6, lut=2)              # table of one entry: 14 bytes a decoy
        lay_chain(lay.payload(ks[5])[0] + 6, 2, 6, lut=5, nbd=2)       # four entries
        for k, bad in ((ks[8], 1), (ks[10], 0)):                        # table sizes 0 and 255 after the - 1: no candidates
            off = lay.payload(k)[0] + 6
            bs, _ = chain_bytes(dt, 1, 4, rng, end=False)
            plan.append((off, bs + decoy(dt, lay.byte_tc, 4, rng, lut=bad) + decoy(dt, lay.byte_tc, 4, rng) + b"\x00"))
            extra.setdefault("not_candidates", []).append(off + dlen)
    elif name == "offset-types":
        ks = blocks(1)
        j = 2
        for tc in range(4):
            if off_bytes(dt)[tc]:
                lay_chain(lay.payload(ks[j])[0] + 6, 3, 2 * tc + 2, tc=tc)
            else:
                off = lay.payload(ks[j])[0] + 6
                bs, rel = chain_bytes(dt, 3, 2 * tc + 2, rng, tc=tc)
                plan.append((off, bs))
                extra.setdefault("not_candidates", []).extend(off + r for r in rel)
            j += 2
    elif name == "crowd":
        # more false survivors in one piece than the mending's table of struck entries holds
        ks = blocks(1)
        for k in ks[2:11]:
            lay_chain(lay.payload(k)[0] + 6, 8, 6)       # 9 hosts x 7 survivors
        lay_chain(lay.payload(ks[11])[0] + 6, 3, 6)      # + 2 = 65: one more than the table holds
        extra["crowded_piece"] = 1
    elif name == "under-cap":
        # the same crowd one decoy short: 64 false survivors, exactly what the table holds -- the piece has to strike them all
        ks = blocks(1)
        for k in ks[2:11]:
            lay_chain(lay.payload(k)[0] + 6, 8, 6)
        lay_chain(lay.payload(ks[11])[0] + 6, 2, 6)
        extra["crowded_piece"] = 1
    elif name == "raw-host":
        k = [k for k, kind in lay.kinds.items() if kind == "raw"][0]
        lay_chain(lay.payload(k)[0] + 8, 3, 6)
        lay_chain(lay.payload(k)[1] - 2 * dlen - 4, 2, lay.sig(k + 1))
    elif name == "flat-run":
        k = min(lay.kinds) - 1       # the last noisy block in front of the run
        lay_chain(lay.payload(k)[0] + 6, 3, 6)
        lay_chain(lay.payload(k)[1] - 2 * dlen, 2, lay.sig(k + 1), end=False)
    elif name == "long-chain":
        # for the walking tiers: false chains of more than nine steps -- one that dies in the middle of a payload, one that merges into
        # the path at its host's end
        n = (lay.payload(0)[1] - lay.payload(0)[0] - 16) // dlen
        assert n >= 10
        ks = blocks(1)
        lay_chain(lay.payload(ks[3])[0] + 6, n, 6)
        k = blocks(2)[1]
        lay_chain(lay.payload(k)[1] - n * dlen, n, lay.sig(k + 1), end=False)
        # ... and two aimed at the walking tiers' chunks (CHUNK bytes from the blob's first byte on): a chain that runs through a chunk's
        # last KiB and dies on the chunk's last bytes, and one that begins in a chunk's last bytes and goes on into the next chunk's window
        hosts = {lay.block_at(off) for off, _ in plan}
        ends, crosses = [], []
        ne = 10 if lay.payload(0)[1] - lay.payload(0)[0] >= 200 else 8      # (decoys of the chunk-aimed chains: what a payload has room for)
        for x in range(CHUNK, lay.blob_len, CHUNK):
            k = lay.block_at(x)
            lo, hi = lay.payload(k) if lay.kinds.get(k) is None else (0, 0)
            if k in hosts or k - 1 in hosts or k + 1 in hosts or x // piece == 0 or x % piece == 0 or k >= lay.n_blocks - 2:      # (a piece's first byte: the boundary plan)
                continue
            if not ends and lo + 8 <= x - 4 - ne * dlen and x <= hi - 8:
                lay_chain(x - 4 - ne * dlen, ne, 6)          # (its four closing bytes are the chunk's last)
                ends.append(x); hosts.add(k)
            elif ends and not crosses and lo + 8 <= x - 3 * dlen and x + (ne - 3) * dlen + 4 <= hi - 8:
                lay_chain(x - 3 * dlen, ne, 6)
                crosses.append(x); hosts.add(k)
        assert ends and crosses, "no chunk boundary in the middle of a payload: another shape"
        extra["chunk_ends"], extra["chunk_crosses"] = ends, crosses
    elif name == "ragged":
        # decoys that carry the edge blocks' count bytes (8 x rows mod 8, 8 x columns mod 8) as well as 64
        hl8, wl8 = 8 * (lay.rows & 7), 8 * (lay.cols & 7)
        for i in (1, 2):
            ks = blocks(i)
            lay_chain(lay.payload(ks[2])[0] + 6, 3, 6)
            lay_chain(lay.payload(ks[5])[0] + 6, 4, 4, count=hl8)
            if i == 1:
                lay_chain(lay.payload(ks[8])[0] + 6, 2, 10, count=wl8)
            k = ks[-2]
            lay_chain(lay.payload(k)[1] - 3 * (4 + hl8 // 8), 3, lay.sig(k + 1), count=hl8, end=False)
    elif name == "masked":
        # count bytes 1 ... 64; chains of 5-byte decoys (8 values or fewer) in the block in front of a run of one-byte blocks
        run0 = min(k for k, kind in lay.kinds.items() if kind == "zero")
        k = run0 - 1
        assert lay.kinds.get(k) is None and lay.payload(k)[1] - lay.payload(k)[0] >= 36
        lay_chain(lay.payload(k)[1] - 4 * 5, 4, lay.sig(k + 1), count=7, end=False)
        i = run0 + 30
        # (a candidate is no longer than the raw form of so many values: 1 + count x sizeof(T) -- a 5-byte decoy of ONE value is none for
        # uint16, whose raw form is 3 bytes: two values at the least there)
        for cnt, n in ((1 if lay.tb > 2 else 2, 3), (8, 2), (33, 2), (64, 2)):
            while lay.kinds.get(i) is not None or lay.payload(i)[1] - lay.payload(i)[0] < 50:
                i += 1
            lay_chain(lay.payload(i)[0] + 5, n, 6, count=cnt)
            i += 3
    else:
        raise ValueError(name)
    return plan, promised, extra


def _ragged_or_masked(plan_name, d, piece, O):
    """-> (rows, cols, mask, bytes the mask takes in the blob)"""
    if plan_name == "ragged":
        return 250, 253, None, 0
    rows, cols = (64, 256) if piece < 32768 else (256, 256)
    rng = np.random.default_rng(77)
    mask = (rng.random((rows, cols)) > 0.3).astype(np.uint8)         # 30 % invalid, sparse
    mask[16:24, 40:200] = 0                                          # a run of 20 blocks without a valid pixel: one byte each
    mask[16:24, 32:40] = 1; mask[18:20, 32:40] = 0                   # the block in front of the run: 48 values, a payload of whole bytes
    rc, blob = O.encode(np.ones((rows, cols), DTYPES[d]) + mask.astype(DTYPES[d]), 0, mask=mask)
    assert rc == 0
    return rows, cols, mask, struct.unpack_from("<i", blob, 90)[0]


def _kinds(plan_name, dtype, rows, cols, nb, piece):
    if plan_name == "raw-host":
        probe = Layout(dtype, rows, cols, nb)
        return {probe.stuffed_blocks_in_piece(piece, 1)[4]: "raw"}
    if plan_name == "flat-run":
        probe = Layout(dtype, rows, cols, nb)
        k0 = probe.stuffed_blocks_in_piece(piece, 1)[6]
        return {k: (("const", 77) if k < k0 + 50 else "zero") for k in range(k0, k0 + 90)}
    return None


_built = {}


def build_case(O, name, piece):
    """The case `name` ("<plan>-<type>") for pieces of `piece` bytes, its preconditions asserted from the model.  O: the oracle (it
    encodes; the library under test is not touched).  Cached: every test of a file shares one build."""
    key = (name, piece)
    if key in _built:
        return _built[key]
    plan_name, d = name.rsplit("-", 1)
    dtype = np.float32 if d in FLOAT_BITS else DTYPES[d]
    (rows, cols), nb, mz = shape_for(dtype, piece)
    nb = FLOAT_BITS.get(d, nb)
    if plan_name == "ragged" and d == "u16":
        nb = 14      # (at 15 bits the 2 x 8 blocks of the last block row are raw, 32 on end: no stream of the scanning decoder, decoys or none)
    mask, mask_bytes = None, 0
    if plan_name in ("ragged", "masked"):
        rows, cols, mask, mask_bytes = _ragged_or_masked(plan_name, d, piece, O)
    kw = {} if mask is None else {"mask": mask}
    lay = Layout(dtype, rows, cols, nb, _kinds(plan_name, dtype, rows, cols, nb, piece), mask, mask_bytes)
    plan, promised, extra = _plan(plan_name, lay, piece, np.random.default_rng(sum(map(ord, name))))
    c = Case()
    c.name, c.plan_name, c.dtype, c.max_z_err, c.layout, c.piece, c.plan, c.extra = name, plan_name, dtype, mz, lay, piece, plan, extra
    c.mask, c.kw = mask, kw
    for seed in range(1000, 1040):
        # filler is drawn again until the CONTROL raster (same plan, decoy bytes left as filler) holds no false survivor
        q, stream = generate(lay, plan, seed, control=True)
        arr = to_raster(lay, q, mz)
        rc, blob = O.encode(arr, mz, **kw)
        assert rc == 0
        assert blob[lay.data_begin:] == stream.tobytes() and len(blob) == lay.blob_len, "the control raster's blocks did not come out as aimed"
        mc = model(blob, dtype, rows, cols, mask)
        if not mc.false_survivors:
            break
    else:
        raise AssertionError("no filler without accidental false survivors")
    c.control, c.control_blob, c.control_model = arr, blob, mc
    q, stream = generate(lay, plan, seed)
    c.arr = to_raster(lay, q, mz)
    rc, c.blob = O.encode(c.arr, mz, **kw)
    assert rc == 0
    # every block came out bit-stuffed with the intended nb and length (else the aim is off and the case is void)
    assert len(c.blob) == lay.blob_len and c.blob[lay.data_begin:] == stream.tobytes(), "the blocks did not come out as aimed"
    rc, dec, _ = O.decode(c.blob)
    v = np.ones((rows, cols), bool) if mask is None else mask != 0
    assert rc == 0 and np.array_equal(dec.reshape(rows, cols)[v].view(np.uint8), c.arr[v].view(np.uint8)), "the quantiser did not return q"
    m = c.model = model(c.blob, dtype, rows, cols, mask)
    assert list(lay.starts) == m.starts
    # ---- preconditions (conditions, not measurements)
    fs = set(m.false_survivors)
    assert set(promised) <= fs and len(fs) >= len(promised), ("the plan's false survivors", sorted(set(promised) - fs))
    cand_begins = {p for p, _ in m.cands}
    for p in extra.get("not_candidates", []):
        assert p not in cand_begins, ("a decoy the rules have to reject is a candidate", p)
    c.per_piece = per_piece(m.false_survivors, piece)
    if plan_name == "crowd":
        assert c.per_piece == {1: 65}, c.per_piece
    elif plan_name == "under-cap":
        assert c.per_piece == {1: 64}, c.per_piece
    elif plan_name == "long-chain":
        assert max(c.per_piece.values()) <= 64 and len(promised) >= 32, c.per_piece       # (for the walking tiers: chains of more than nine steps)
    else:
        assert max(c.per_piece.values()) <= 8, c.per_piece
    if plan_name == "boundary-host":
        for x in extra["boundaries"]:
            k = lay.block_at(x)
            inside = [p for p in m.false_survivors if x <= p < lay.starts[k + 1]]
            assert lay.starts[k] < x and len(inside) >= 2 and inside[-1] + 12 == lay.starts[k + 1], (x, inside)
    if plan_name == "boundary":
        pre = scan_pre(lay.tb)
        for x in extra["boundaries"]:
            front = [p for p in m.false_survivors if x - pre <= p < x]
            inside = [p for p in m.false_survivors if p >= x]
            assert front and inside and inside[0] - front[-1] == 12, (x, front, inside[:2])
    c.promised = promised
    _built[key] = c
    return c


# -------------------------------------------------------------------------------------------------------------------------- checks
def same(a, b):
    if a is None or b is None:
        return a is None and b is None
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8).ravel(), np.ascontiguousarray(b).view(np.uint8).ravel())


def same_valid(want, got, mask):
    """decodes (status, pixels, mask) agree: the pixels where the band is valid, and the mask"""
    if mask is None:
        return same(want[1], got[1]) and same(want[2], got[2])
    v = np.asarray(mask).ravel() != 0
    return same(want[2], got[2]) and same(np.asarray(want[1]).ravel()[v], np.asarray(got[1]).ravel()[v])


def fletcher32(b):
    s1 = s2 = 0xFFFF
    words = len(b) // 2
    i = 0
    while words:
        t = min(words, 359)
        words -= t
        for _ in range(t):
            s1 += b[i] << 8; i += 1
            s1 += b[i]; i += 1
            s2 += s1
        s1 = (s1 & 0xFFFF) + (s1 >> 16)
        s2 = (s2 & 0xFFFF) + (s2 >> 16)
    if len(b) & 1:
        s1 += b[i] << 8
        s2 += s1
    s1 = (s1 & 0xFFFF) + (s1 >> 16)
    s2 = (s2 & 0xFFFF) + (s2 >> 16)
    return ((s2 << 16) | s1) & 0xFFFFFFFF


def reseal(bb):
    """the checksum of a damaged copy put right, so that the damage reaches the block decoders"""
    bb = bytearray(bb)
    struct.pack_into("<I", bb, 10, fletcher32(bytes(bb[14:])))
    return bytes(bb)


def damaged_copies(c, n=8):
    """one byte flipped inside a decoy, one inside a real header next to a decoy; every other copy with its checksum put right"""
    rng = np.random.default_rng(len(c.name) + c.piece)
    lay = c.layout
    out = []
    for t in range(n):
        off, bs = c.plan[int(rng.integers(0, len(c.plan)))]
        if t % 2 == 0:
            at = off + int(rng.integers(0, len(bs)))
        else:
            k = min(lay.block_at(off) + int(rng.integers(0, 2)), lay.n_blocks - 1)
            at = int(lay.starts[k]) + int(rng.integers(0, min(4, lay.lens[k])))
        y = bytearray(c.blob)
        y[at] ^= 1 << int(rng.integers(0, 8))
        out.append((f"{c.name}-flip{t}-at{at}", reseal(y) if t % 4 >= 2 else bytes(y)))
    return out


def check_decoy_case(T, P, c):
    """Bit-exact (integers, and float32 blobs decoded by a deterministic decoder: no tolerance).  T: the trusted decoder, P: the library
    under test through the stock C ABI."""
    rc, blob = P.encode(c.arr, c.max_z_err, **c.kw)
    assert rc == 0 and blob == c.blob, "the encoder's blob differs from the oracle's"
    want = T.decode(c.blob)
    got = P.decode(c.blob)
    assert want[0] == 0 and got[0] == 0, (c.name, got[0])
    assert same_valid(want, got, c.mask), c.name
    if "behind" in c.extra:      # a buffer longer than the blob, decoys behind the blob's end
        y = c.blob + c.extra["behind"]
        d1, d2 = T.decode(y), P.decode(y)
        assert d1[0] == 0 and d2[0] == 0 and same_valid(d1, d2, c.mask), (c.name, "bytes behind the blob", d2[0])
    for name, y in damaged_copies(c):
        d1, d2 = T.decode(y), P.decode(y)
        assert (d1[0] == 0) == (d2[0] == 0), (name, d1[0], d2[0])
        if d1[0] == 0:
            assert same_valid(d1, d2, c.mask), name


def check_masked_tiers(T, P, c):
    """A band with a mask: the scan (MODE 1) cuts the stream into blocks -- lerc_amd_decode_forms()[0] counts the band -- and neither the
    decode kernels refuse its offsets nor the scan hands the band on (refusals 0 and 1), control raster and decoys alike."""
    for kind, blob in (("control", c.control_blob), ("decoys", c.blob), ("decoys", c.blob)):
        f0, q0 = P.decode_forms(), P.decode_refusals()
        want, got = T.decode(blob), P.decode(blob)
        f1, q1 = P.decode_forms(), P.decode_refusals()
        assert want[0] == 0 and got[0] == 0 and same_valid(want, got, c.mask), (c.name, kind)
        assert f1[0] == f0[0] + 1 and q1[:2] == q0[:2], (c.name, kind, f0, f1, q0, q1, P.last_note())


def decode_watched(ctx, T, blob, shape, dtype):
    """one decode on the context `ctx` (see the test files' Context), pixels checked against T's -> (forms' rise, refusals' rise, paths' rise)"""
    f0, q0, c0 = ctx.forms(), ctx.refusals(), ctx.paths()
    rc, out = ctx.decode(blob, shape, dtype)
    assert rc == 0, (rc, ctx.note())
    want = T.decode(blob)
    assert want[0] == 0 and same(want[1], out), "pixels"
    f1, q1, c1 = ctx.forms(), ctx.refusals(), ctx.paths()
    return [b - a for a, b in zip(f0, f1)], [b - a for a, b in zip(q0, q1)], [b - a for a, b in zip(c0, c1)]


SCAN = [0, 0, 0, 1]


def check_tiers(new_context, T, c, other):
    """Which tier served, on a context of the case's own (the tiers remember: DecodeTiers, codec_decode.cpp).
    other: a control case of ANOTHER shape (for the crowd plan)."""
    shape = c.arr.shape
    ctx = new_context()
    try:
        # the control raster: the scanning decoder, early counts, nothing thrown away (blocks the scan does not see -- the raw host, the
        # flat run -- are entered by the mending: a count that changes costs the context's first such band one launch)
        f, q, p = decode_watched(ctx, T, c.control_blob, shape, c.dtype)
        assert f == SCAN and q[2] <= (1 if c.layout.kinds else 0) and p[2:] == [1, 0], ("control", f, q, p, ctx.note())
    finally:
        ctx.close()
    ctx = new_context()
    try:
        seen = [decode_watched(ctx, T, c.blob, shape, c.dtype) for _ in range(3)]
        note = ctx.note()
        if c.plan_name == "crowd":
            # more than the tables hold: the piece gives up, the band is handed on (counted) and served behind the scanning decoder;
            # the next band of the shape starts below the scanning tier; a band of another shape is not affected
            f, q, p = seen[0]
            assert q[2] >= 1 and f[3] == 0, (c.name, seen, note)
            for f, q, p in seen[1:]:
                assert f[3] == 0 and q[2] == 0, (c.name, seen, note)
            f, q, p = decode_watched(ctx, T, other.control_blob, other.arr.shape, other.dtype)
            assert f == SCAN and p[2:] == [1, 0], ("another shape", f, q, p, ctx.note())
        elif c.plan_name == "boundary":
            # The anchor rule trusts the last two survivors in front of a piece's own bytes if the one ends where the other begins; two
            # decoys of a chain that straddles the piece's first byte are such a pair.  The piece then walks from a false anchor, finds
            # no way through and gives up: the band is handed on ONCE, a walking tier serves it on the streaming path, and the
            # shape's next bands start there with nothing thrown away (the scanning decoder's mending).
            f, q, p = seen[0]
            assert q[2] >= 1 and f[3] == 0 and f[1] + f[2] == 1 and p[2:] == [1, 0], (c.name, seen, note)
            for f, q, p in seen[1:]:
                assert f[3] == 0 and f[1] + f[2] == 1 and q[2] == 0 and p[2:] == [1, 0], (c.name, seen, note)
        else:
            # at most 8 false survivors a piece: the scanning decoder serves the band.  Striking changes a piece's early count, so the
            # context's first such band may throw one launch away (the late form mends) and the bands behind it none.
            assert [f for f, _, _ in seen] == [SCAN] * 3, (c.name, seen, note)
            assert seen[0][1][2] <= 1 and [q[2] for _, q, _ in seen[1:]] == [0, 0], (c.name, seen, note)
            assert all(p[2:] == [1, 0] for _, _, p in seen), (c.name, seen, note)
            if "behind" in c.extra:
                f, q, p = decode_watched(ctx, T, c.blob + c.extra["behind"], shape, c.dtype)
                assert f == SCAN and q[2] == 0 and p[2:] == [1, 0], (c.name, "bytes behind the blob", f, q, p, ctx.note())
    finally:
        ctx.close()
    return seen, note


# ---- the tiers behind the scanning decoder: the knobs are read once a process, so the case list runs in a child process a setting
KNOBS = [("LERC_AMD_DECODE_SCAN", "0"), ("LERC_AMD_DECODE_LAUNCHES", "2"), ("LERC_AMD_SCAN_EARLY", "0")]

CHILD_CODE = r"""
import sys, os
sys.path.insert(0, os.path.join(%r, "tests"))
import numpy as np, capi, decoy_common as D
O = capi.oracle()
P = getattr(capi, %r)()
piece = %d
late = os.environ.get("LERC_AMD_SCAN_EARLY") == "0"
for name in D.case_names():
    c = D.build_case(O, name, piece)
    for kind, blob in (("control", c.control_blob), ("decoys", c.blob)):
        c0, q0, f0 = P.path_counters(), P.decode_refusals(), P.decode_forms()
        want, got = O.decode(blob), P.decode(blob)
        c1, q1, f1 = P.path_counters(), P.decode_refusals(), P.decode_forms()
        assert want[0] == 0 and got[0] == 0 and D.same_valid(want, got, c.mask), ("pixels", name, kind)
        if kind == "control" and c.mask is None:
            assert c1[2] == c0[2] + 1 and c1[3] == c0[3], ("the control raster left the streaming path", name, c0, c1, P.last_note())
        if late and f1[3] > f0[3]:      # (the scanning decoder served the band -- the tiers remember a shape that was handed on)
            assert q1[2] == q0[2], ("a launch thrown away with late counts", name, kind, q0, q1, P.last_note())
    for tag, y in D.damaged_copies(c, 4):
        d1, d2 = O.decode(y), P.decode(y)
        assert (d1[0] == 0) == (d2[0] == 0), (tag, d1[0], d2[0])
        if d1[0] == 0:
            assert D.same_valid(d1, d2, c.mask), tag
print("decoys ok")
"""


def run_knob_child(lib_name, piece, knob, value, timeout=900):
    import os
    import subprocess
    import sys
    env = dict(os.environ, **{knob: value})
    out = subprocess.run([sys.executable, "-c", CHILD_CODE % (capi.ROOT, lib_name, piece)], env=env, stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT, timeout=timeout)
    assert out.returncode == 0 and b"decoys ok" in out.stdout, out.stdout.decode()[-3000:]
