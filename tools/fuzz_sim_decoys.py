"""Soak test on the emulator (no GPU): rasters whose payloads carry random PLANS of decoy block headers (tests/decoy_common.py) --
chains of random length, offset type, bits a value and signature at random places of the stream, piece boundaries and the stream's
tail included, sometimes with a look-up table -- through the emulator build and the oracle: blob, status and pixels have to agree, and
so do the verdicts on copies with one byte flipped.  Prints the seed of every plan that does not, and what the stream model counted.
    python tools/fuzz_sim_decoys.py [seed] [seconds]"""
import sys, os, time, subprocess
sys.path.insert(0, 'tests'); sys.path.insert(0, '.')
import numpy as np, capi, decoy_common as D
subprocess.check_call(["make", "-s", "-C", os.path.join(capi.ROOT, "lerc_amd", "csrc"), "sim", "-j8"])
S = capi.sim(); O = capi.oracle()
seed0 = int(sys.argv[1]) if len(sys.argv) > 1 else 1
budget = float(sys.argv[2]) if len(sys.argv) > 2 else 120
PIECE = 8192
t0 = time.time(); n = 0; bad = 0; most = 0; total_false = 0
while time.time() - t0 < budget:
    seed = seed0 * 1000003 + n
    rng = np.random.default_rng(seed)
    d = str(rng.choice(list(D.DTYPES)))
    dtype = D.DTYPES[d]
    (rows, cols), nb, mz = D.shape_for(dtype, PIECE)
    if dtype == np.float32: nb = int(rng.integers(18, 21))
    lay = D.Layout(dtype, rows, cols, nb)
    plan, used = [], set()
    for _ in range(int(rng.integers(1, 40))):
        how = int(rng.integers(0, 4))
        if how == 0: k = lay.block_at(int(rng.integers(1, lay.blob_len // PIECE + 1)) * PIECE - int(rng.integers(0, 2)) * lay.stuffed_len)
        elif how == 1: k = lay.n_blocks - 1 - int(rng.integers(0, 3))
        else: k = int(rng.integers(0, lay.n_blocks))
        k = min(max(k, 0), lay.n_blocks - 1)
        if k in used: continue
        tcs = [tc for tc in range(4) if D.off_bytes(lay.dt)[tc]]
        tc = int(rng.choice(tcs)); nbd = int(rng.integers(1, 4)); lut = int(rng.integers(2, 6)) if rng.random() < 0.2 else None
        sig = 2 * int(rng.integers(0, 8)) if rng.random() < 0.5 or k + 1 >= lay.n_blocks else lay.sig(k + 1)
        lo, hi = lay.payload(k)
        one = len(D.decoy(lay.dt, tc, sig, rng, nbd, lut))
        room = hi - lo - 10
        if one > room: continue
        cnt = int(rng.integers(1, room // one + 1))
        with_host = rng.random() < 0.4
        bs, _ = D.chain_bytes(lay.dt, cnt, sig, rng, tc=tc, nbd=nbd, lut=lut, end=not with_host and cnt * one + 4 <= room)
        off = hi - len(bs) if with_host else lo + 5 + int(rng.integers(0, room - len(bs) + 1))
        if off < lo + 5 or off + len(bs) > hi: continue
        plan.append((off, bs)); used.add(k)
    q, stream = D.generate(lay, plan, seed & 0xFFFF)
    arr = D.to_raster(lay, q, mz)
    r1, b1 = O.encode(arr, mz)
    tag = f"seed {seed} {d} nb {nb} chains {len(plan)}"
    if r1 != 0 or b1[lay.data_begin:] != stream.tobytes():
        n += 1; continue      # (a block came out otherwise than aimed -- a look-up table won: the plan is void)
    m = D.model(b1, dtype, rows, cols)
    pp = D.per_piece(m.false_survivors, PIECE)
    most = max(most, max(pp.values(), default=0)); total_false += len(m.false_survivors)
    r2, b2 = S.encode(arr, mz)
    if r2 != 0 or b2 != b1: print("ENC MISMATCH", tag); bad += 1
    d1, d2 = O.decode(b1), S.decode(b1)
    if d1[0] != d2[0] or not D.same(d1[1], d2[1]): print("DEC MISMATCH", tag, d1[0], d2[0], pp, S.last_note()); bad += 1
    for t in range(2):
        if not plan: break
        off, bs = plan[int(rng.integers(0, len(plan)))]
        y = bytearray(b1); y[off + int(rng.integers(0, len(bs)))] ^= 1 << int(rng.integers(0, 8))
        y = D.reseal(y) if t else bytes(y)
        d1, d2 = O.decode(y), S.decode(y)
        if (d1[0] == 0) != (d2[0] == 0) or (d1[0] == 0 and not D.same(d1[1], d2[1])): print("DAMAGED MISMATCH", tag, d1[0], d2[0]); bad += 1
    n += 1
print("seed", seed0, "plans", n, "mismatches", bad, "false survivors in all", total_false, "most in one piece", most)
