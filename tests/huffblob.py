"""A small reader of single-band Lerc2 blobs coded in the 8-bit Huffman modes (Lerc2.cpp WriteHeader / WriteMask /
WriteMinMaxRanges, Huffman.cpp WriteCodeTable), and the decoder's sub-sequence rule (huffman_kernels.hip: huffSubWords):
enough to tell where the Huffman stream begins in the blob (how many bytes into an aligned word the decoder finds it) and
how many speculative sub-sequences the decoder cuts it into."""
import math
import struct

DT_SIZE = [1, 1, 2, 2, 4, 4, 4, 8]
IEM_TILING, IEM_DELTA_HUFFMAN, IEM_HUFFMAN = 0, 1, 2

# huffman_dev.h / huffman_kernels.hip defaults
SUB_WORDS_MIN, SUB_WORDS_MAX = 33, 41
WG_PER_CU = 3
DEC_THREADS_GPU, DEC_THREADS_SIM = 256, 16    # (emulator builds: LERC_SMALL_GROUPS)


def _header_bytes(v):
    return 6 + 4 + (4 if v >= 3 else 0) + 4 * (7 if v >= 4 else 6) + (8 if v >= 6 else 0) + 8 * (5 if v >= 6 else 3)


def parse(blob):
    """-> dict(version, n_rows, n_cols, n_depth, num_valid, dt, mode, [stream_begin, stream_bytes, max_len, n_codes])"""
    b = bytes(blob)
    assert b[:6] == b"Lerc2 ", "not a Lerc2 blob"
    v = struct.unpack_from("<i", b, 6)[0]
    assert v >= 3, v
    at = 14
    n_rows, n_cols = struct.unpack_from("<2i", b, at); at += 8
    n_depth = 1
    if v >= 4:
        n_depth = struct.unpack_from("<i", b, at)[0]; at += 4
    num_valid, _mb, blob_size, dt = struct.unpack_from("<4i", b, at)
    assert blob_size == len(b), "one band only"
    at = _header_bytes(v)
    n_mask = struct.unpack_from("<i", b, at)[0]
    at += 4 + n_mask
    out = dict(version=v, n_rows=n_rows, n_cols=n_cols, n_depth=n_depth, num_valid=num_valid, dt=dt, mode=None)
    if num_valid == 0:
        return out
    if v >= 4:
        nb = n_depth * DT_SIZE[dt]
        lo, hi = b[at:at + nb], b[at + nb:at + 2 * nb]
        at += 2 * nb
        if lo == hi:
            return out    # constant planes: nothing follows
    one_sweep = b[at]; at += 1
    if one_sweep:
        out["mode"] = "one-sweep"
        return out
    out["mode"] = b[at]; at += 1
    if out["mode"] not in (IEM_DELTA_HUFFMAN, IEM_HUFFMAN):
        return out
    # code table: 4 ints (version, size, i0, i1), the code lengths bit-stuffed, the codes MSB first in 32-bit words
    _tv, size, i0, i1 = struct.unpack_from("<4i", b, at); at += 16
    b0 = b[at]; at += 1
    cb = 4 if (b0 >> 6) == 0 else 3 - (b0 >> 6)
    n = int.from_bytes(b[at:at + cb], "little"); at += cb
    bits = b0 & 31
    assert n == i1 - i0 and not (b0 & 32), (n, i0, i1, b0)
    n_len_bytes = (n * bits + 7) >> 3
    packed = int.from_bytes(b[at:at + n_len_bytes], "little")
    at += n_len_bytes
    lens = [(packed >> (i * bits)) & ((1 << bits) - 1) for i in range(n)]    # (codec >= 3: LSB first)
    at += 4 * ((sum(lens) + 31) // 32)
    out.update(stream_begin=at, stream_bytes=len(b) - at, max_len=max(lens), n_codes=sum(1 for x in lens if x))
    assert 0 < out["stream_bytes"] and out["stream_bytes"] % 4 == 0, out
    return out


def sub_words(stream_bits, slots, threads):
    """huffSubWords: odd width in [33, 41] words that fills the `slots` resident workgroups in the fewest rounds (ties: smallest)"""
    words = (stream_bits + 31) // 32
    best, best_cost = SUB_WORDS_MIN, None
    for w in range(SUB_WORDS_MIN, SUB_WORDS_MAX + 1, 2):
        n_sub = -(-words // w)
        n_wg = -(-n_sub // threads)
        cost = -(-n_wg // max(slots, 1)) * w
        if best_cost is None or cost < best_cost:
            best, best_cost = w, cost
    return best


def n_sub(info, compute_units, threads):
    """the decoder's sub-sequence count for a parsed blob (decodeHuffman: the stream's whole words)"""
    stream_bits = (info["stream_bytes"] // 4) * 32
    sw = sub_words(stream_bits, WG_PER_CU * compute_units, threads)
    return -(-stream_bits // (sw * 32))


def round_cap(n):
    """sync rounds (host round trips) allowed for a stream of n sub-sequences: a log-depth resolution"""
    return 2 + (math.ceil(math.log2(n)) if n > 1 else 0)
