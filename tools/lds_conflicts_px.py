#!/usr/bin/env python3
"""Counts the LDS bank conflicts of k_rt_cut_px / k_rt_paste_px (lerc_amd/csrc/raster_tiles_px.hip) from their address arithmetic, for
the layout they use -- one padding dword after every 16 * pixelPitch bytes of a row's run -- and for the run laid out as in memory.
No GPU: the banks are those of the 32-lane groups of ds_read_b32 / ds_write_b32 and their 8- and 16-bit forms, dword address mod 32;
lanes on one dword do not conflict.  The degree printed is the largest number of different dwords on one bank within a group.

  transposing side   lane l of a row moves the elements of pixels l * V .. l * V + V - 1 of one band (V = 16 / element size), one
                     element an instruction
  copying side       lane l moves the l-th 16-byte vector of the run as four dwords, one dword an instruction

k_rtd_cut / k_rtd_paste (raster_tiles_depth.hip) use the same layout.  For planes and lines their run is the staged one, pitch nDepth:
the rows P = nDepth of the first table are theirs.  For gapped pixels (nDepth < pixelPitch) the run is the raster's, pitch pixelPitch,
copied as above, and there is a third side, the second table's:

  compacting side    lane l moves the elements l * V .. l * V + V - 1 of the COMPACTED run (nDepth elements a pixel), one element an
                     instruction: element j lies at element (j // nDepth) * pixelPitch + j % nDepth of the run.  A vector begins at any
                     element of a pixel, so the degree is the largest over the nDepth phases
"""


def degree(dwords):
    banks = {}
    for d in set(dwords):
        banks.setdefault(d % 32, set()).add(d)
    return max(len(v) for v in banks.values())


def at(byte, pitch, padded):
    """dword of a byte of the run; pitch in elements: a lane's V pixels are 16 * pitch bytes whatever the element size"""
    return (byte + (4 * (byte // (16 * pitch)) if padded else 0)) // 4


def main():
    print("%-8s %-5s %-28s %-28s" % ("element", "P", "transposing side: padded (as in memory)", "copying side: padded (as in memory)"))
    for item in (1, 2, 4, 8):
        v = 16 // item
        for p in range(2, 9):
            out = []
            for padded in (True, False):
                tr = max(degree([at(((l * v + q) * p + b) * item + w * 4, p, padded) for l in range(32)])
                         for q in range(v) for b in range(p) for w in range(max(1, item // 4)))
                cp = max(degree([at(16 * l + 4 * j, p, padded) for l in range(32)]) for j in range(4))
                out.append((tr, cp))
            print("%-8d %-5d %-28s %-28s" % (item, p, "%d (%d)" % (out[0][0], out[1][0]), "%d (%d)" % (out[0][1], out[1][1])))
    print()
    print("%-8s %-5s %-5s %-28s" % ("element", "P", "D", "compacting side: padded (as in memory)"))
    for item in (1, 2, 4, 8):
        v = 16 // item
        for p in range(2, 9):
            for d in range(1, p):
                out = []
                for padded in (True, False):
                    out.append(max(degree([at((((j0 + l * v + q) // d) * p + (j0 + l * v + q) % d) * item + w * 4, p, padded) for l in range(32)])
                                   for q in range(v) for j0 in range(d) for w in range(max(1, item // 4))))
                print("%-8d %-5d %-5d %-28s" % (item, p, d, "%d (%d)" % (out[0], out[1])))


if __name__ == "__main__":
    main()
