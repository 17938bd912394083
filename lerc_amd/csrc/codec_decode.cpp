// codec_decode.cpp -- lerc_decode() producing device-resident pixels: the entry points, the streaming launches and
// which of them takes a band (DecodeTiers).  Every band they do not take blind, or hand on, is decoded by
// decodeBands() (codec_decode_band.cpp).
#include "codec.h"
#include "huffman.h"
#include "fpl.h"
#include "tile_fast.h"
#include <algorithm>
#include <cstdint>
#include <cstdio>

namespace lerc {

// ------------------------------------------------------------------------------------------------
// streaming kernels for one band
// ------------------------------------------------------------------------------------------------
// (a band's result cell: codec.h)
static_assert(sizeof(FastDecodeParams) <= 128, "cell layout");

size_t fastBandWorkspace(int nRows, int nCols, u32 sizeGiven, u32 nTiles)
{
  const FastWalkPlan wp = makeFastWalkPlan(nRows, nCols, sizeGiven, nTiles);
  const size_t perTile = (size_t)wp.nChunks * (sizeof(FastChunkRec) + (size_t)kDiscWalks * kFastListCap * 2 + 12) + (size_t)wp.nBlocks * 4
    + (size_t)(wp.nChunks / kResolveWG + 2) * 4 + 4096 + kResolveWG * sizeof(FastChunkRec);
  return perTile * nTiles + (size_t)kDecodeChunks * kDiscWalks * kFastListCap * 2 + (1u << 16);
}

// Enqueues header check, discovery and decode of nTiles blobs (one band: nTiles == 1, dTileOffset == nullptr) by the form, for the
// shape and with the epoch of ticket `t`; nothing is read back here.  dParams [nTiles] and dFallback [4 * nTiles] receive the
// verdicts; the flags in dFallback are raised by writing the epoch (tile_fast.h), so the cells need no clearing.  t.gridBytes: what
// the scanning decoder's launch was sized for.
static bool launchFastBands(Context& ctx, StreamTicket& t, const u8* dBlobs, u32 sizeBound, u32 nTiles, const u64* dTileOffset,
                            const u32* dTileSize, void* dOut, FastDecodeParams* dParams, u32* dFallback, u8* hCell = nullptr)
{
  const int form = t.form, dt = t.shape.dt, nRows = t.shape.nRows, nCols = t.shape.nCols;
  const u32 epoch = t.epoch;
  hipStream_t st = ctx.activeStream();
  const FastWalkPlan fwp = makeFastWalkPlan(nRows, nCols, sizeBound, nTiles);
  const size_t nT = nTiles, sChunk = fastChunkStride(fwp.nChunks);
  FastDecodeBatch tb;
  tb.nTiles = nTiles; tb.nChunks = fwp.nChunks; tb.nBlocks = fwp.nBlocks; tb.nWaves = fwp.nWaves; tb.discChunks = fwp.discChunks;
  tb.tileElems = (u64)nRows * (u64)nCols; tb.tileOffset = dTileOffset; tb.tileSize = dTileSize;
  FastDecodeBuffers fbuf;
  fbuf.params = dParams;
  fbuf.fallback = dFallback;
  fbuf.hostParams = hCell ? reinterpret_cast<FastDecodeParams*>(hCell + kCellParams) : nullptr;
  fbuf.hostFallback = hCell ? reinterpret_cast<u32*>(hCell + kCellFallback) : nullptr;
  fbuf.epoch = epoch;
  fbuf.publishEpoch = (fastTestGiveUp() & 2u) ? epoch ^ 0x5A5A5A5Au : epoch;
  fbuf.spinLimit = (fastTestGiveUp() & 2u) ? 8u : (1u << 22);
  fbuf.testRewalk = (fastTestGiveUp() & 4u) ? 1u : 0u;
  fbuf.wgCell = fbuf.wgGroupCell = fbuf.wgAcc = nullptr;
  // The scanning decoder asks for a piece's bytes without waiting for the band header where the blob is expected to reach that far:
  // a batch's sizes are exact; a single band comes with its size (the synchronous calls) or with its buffer's capacity (a decode
  // queued behind the encode that writes the blob) -- then what the context's last band of this shape had, plus an eighth (the
  // bands of one job are alike), else half the raster's raw size.  A guess that is too large costs loads nobody looks at, one
  // that is too small the header's latency in the pieces behind it.
  {
    const u64 raw = (u64)nRows * (u64)nCols * (u64)dtSize(dt);
    u32 spec = sizeBound;
    bool fromHint = false;
    if (!dTileOffset && (u64)sizeBound * 10u >= raw * 9u)    // (as large as the raster itself: a capacity, not a size)
    {
      const u64 last = ctx.tiers.sizeGuess.n;
      fromHint = ctx.tiers.sizeGuess.holds(t.shape);
      const u64 guess = fromHint ? last + last / 8u + 65536u : raw / 2u;
      spec = (u32)std::min<u64>(guess, sizeBound);
    }
    fbuf.scanSpecEnd = dTileOffset ? 0xFFFFFFFFu : spec;
    // (... and the launch itself is sized by a guess that comes from a band of this shape: LERC_AMD_SCAN_GRID=0 sizes it by what was given)
    static const bool gridByGuess = []() { const char* e = getenv("LERC_AMD_SCAN_GRID"); return !e || atoi(e) != 0; }();
    fbuf.scanEarly = form == kFormScanEarly ? 1u : 0u;
    fbuf.scanGridBytes = (gridByGuess && fromHint && spec < sizeBound) ? spec : 0u;
    t.gridBytes = form >= kFormScan ? (fbuf.scanGridBytes ? fbuf.scanGridBytes : sizeBound) : 0u;
  }
  fbuf.wgStride = fbuf.wgGroupStride = 0;
  // (epoch-tagged cells, never cleared: they live as long as the context and share its area with the encoder's)
  if (form >= kFormWalk)
  {
    // everything in one launch: a cell per workgroup and per group of workgroups, and the groups' checksum accumulators
    // (counters: left zero by the launch's last workgroup)
    const size_t sWg = fastAnyWgStride(sizeBound, dtSize(dt)), sGrp = fastAnyGroupStride(sizeBound, dtSize(dt));
    fbuf.wgStride = (u32)sWg; fbuf.wgGroupStride = (u32)sGrp;
    fbuf.wgCell = (u64*)ctx.persistentState(1, (nT * (sWg + sGrp) + 8) * 8);
    fbuf.wgGroupCell = fbuf.wgCell ? fbuf.wgCell + nT * sWg : nullptr;
    fbuf.wgAcc = (u64*)ctx.persistentState(0, (nT * sGrp + 8) * 8);
    if (!fbuf.wgCell || !fbuf.wgAcc) return false;
    fbuf.recs = nullptr; fbuf.lists = nullptr; fbuf.chunkCell = fbuf.groupCell = fbuf.waveFletcher = nullptr;
    if (form >= kFormScan)
    {
      ProfScope ps(ctx, "fast_decode_scan");
      launchFastDecodeScan(dt, nRows, nCols, tb, dBlobs, sizeBound, fbuf, dOut, st);
      return true;
    }
    ProfScope ps(ctx, "fast_decode_one");
    launchFastDecodeOne(dt, nRows, nCols, tb, dBlobs, sizeBound, fbuf, dOut, st);
    return true;
  }
  fbuf.recs = ctx.allocT<FastChunkRec>(nT * fwp.nChunks + kResolveWG);    // (+ what the resolve step's unconditional loads may touch)
  fbuf.lists = ctx.allocT<u16>((nT * fwp.nChunks + kDecodeChunks) * (size_t)(kDiscWalks * kFastListCap) + 8);    // (+ what the gather step's clamped loads may touch)
  const size_t cellWords = nT * (2 * sChunk + fastGroupStride(fwp.nChunks)) + 8;
  fbuf.chunkCell = (u64*)ctx.persistentState(1, cellWords * 8);
  fbuf.groupCell = fbuf.chunkCell ? fbuf.chunkCell + nT * 2 * sChunk : nullptr;
  fbuf.waveFletcher = ctx.allocT<u64>(2 * nT * (size_t)fwp.nWaves + 4);
  if (!fbuf.recs || !fbuf.lists || !fbuf.chunkCell || !fbuf.waveFletcher)
    return false;
  static const char* kStage[kFastDecodeStages] = { "fast_discover", "fast_decode" };
  for (int stage = 0; stage < kFastDecodeStages; stage++)
  {
    ProfScope ps(ctx, kStage[stage]);
    launchFastDecode(stage, dt, nRows, nCols, tb, dBlobs, sizeBound, fbuf, dOut, st);
  }
  return true;
}

bool launchFastBand(Context& ctx, StreamTicket& t, const u8* dBand, u32 sizeGiven, void* dOutBand, u8* dCell, u8* hCell)
{
  return launchFastBands(ctx, t, dBand, sizeGiven, 1, nullptr, nullptr, dOutBand, reinterpret_cast<FastDecodeParams*>(dCell + kCellParams),
                         reinterpret_cast<u32*>(dCell + kCellFallback), hCell);
}

// ------------------------------------------------------------------------------------------------
// which form takes a band: DecodeTiers (codec.h)
// ------------------------------------------------------------------------------------------------
static bool fastDecodeOneLaunch()    // the one-launch decoders; LERC_AMD_DECODE_LAUNCHES=2: discovery + decode as two launches only
{
  static const bool one = []() { const char* e = getenv("LERC_AMD_DECODE_LAUNCHES"); return !e || atoi(e) != 2; }();
  return one;
}

// The highest form at most maxForm that is switched on (LERC_AMD_DECODE_LAUNCHES=2: the two-launch form only; LERC_AMD_DECODE_SCAN=0:
// not the scanning decoder; LERC_AMD_SCAN_EARLY=0: no early counts), takes the raster (the scanning decoder: whole 8 x 8 blocks) and
// is not kept off by a window: a stream the scanning decoder cannot follow -- many blocks that are not bit-stuffed -- costs a launch
// before the next tier gets it, and the bands of one job are alike.
int DecodeTiers::pick(int maxForm, const RasterShape& s)
{
  static const bool scanOn = []() { const char* e = getenv("LERC_AMD_DECODE_SCAN"); return !e || atoi(e) != 0; }();
  static const bool earlyOn = []() { const char* e = getenv("LERC_AMD_SCAN_EARLY"); return !e || atoi(e) != 0; }();
  int f = std::min(maxForm, (int)kFormScanEarly);
  if (f <= kFormGeneral) return kFormGeneral;
  if (!fastDecodeOneLaunch()) return kFormTwoLaunch;
  if (f >= kFormScan)
  {
    if (!scanOn || !fastDecodeScanEligible(s.nRows, s.nCols)) f = kFormWalk;
    else if (offScan.take(s)) f = kFormWalk;
    else if (f == kFormScanEarly && (!earlyOn || s.nRows % 8 != 0 || s.nCols % 8 != 0)) f = kFormScan;    // (ragged rasters count late: three count values in their filter make false survivors -- which the mending strikes, changing a count -- likelier: one piece in 3 244 of the 8190^2 raster, enough to throw every early launch away)
    else if (f == kFormScanEarly && countLate.take(s)) f = kFormScan;
  }
  return f;
}

// A form's launch was thrown away for the stream's sake.  The scanning decoder: the next kScanSkip decodes of that shape start one
// tier down.  Its early counts (a piece says how many blocks it holds as soon as the survivors are counted; one whose check or mending
// comes to another count -- a stream with blocks the scan does not see: constant, all zero, raw -- raises a flag): the next lateSpan
// decodes count late, which mends; four times as many after every further one.
void DecodeTiers::handedOn(const StreamTicket& t)
{
  const RasterShape anyType = { -1, t.shape.nRows, t.shape.nCols };
  if (t.form == kFormScan) offScan.open(anyType, kScanSkip);
  if (t.form == kFormScanEarly) { countLate.open(anyType, lateSpan); lateSpan = std::min<u32>(lateSpan * 4u, kScanLateMax); }
}

bool DecodeTiers::judge(const StreamTicket& t, u32 verdict, u32 blobEnd)
{
  if (verdict == 0u)
  {
    if (t.form >= kFormTwoLaunch && t.form <= kFormScanEarly) formCount[std::min<int>(t.form, kFormScan)]++;
    sizeGuess.open(t.shape, blobEnd);    // (the guess for the next band of that shape: launchFastBands)
    return true;
  }
  if (verdictLaunchWasted(verdict)) refusalCount[2]++;
  if (!verdictTierRefused(verdict) || t.form < kFormScan) return false;
  // The launch was sized by the last band of this shape and this one is larger: not the stream's fault -- the guess is forgotten,
  // the shape keeps its tier.  (t.gridBytes is what THIS band's launch held pieces for, whatever has been enqueued since.)
  if ((verdict & kVerdictBlockCount) && t.gridBytes != 0u && fastScanNumWG(blobEnd) > fastScanNumWG(t.gridBytes)) { sizeGuess.n = 0u; return false; }
  handedOn(t);
  return false;
}

void DecodeTiers::judgeBatch(const StreamTicket& t, u32 nServed, bool manyWentOn)
{
  formCount[std::min<int>(t.form, kFormScan)] += nServed;
  if (manyWentOn) handedOn(t);    // (sizes are exact in a batch: no guess to keep or to forget; the tiles that went on are judged one by one)
}

// reason bits of a tile's / band's four epoch tagged flag cells
u32 fastFlagBits(const u32* cells, u32 epoch)
{
  u32 bits = 0;
  for (int k = 0; k < 4; k++) if (cells[k] == epoch) bits |= 1u << k;
  return bits;
}

// what the host makes of a band's cell after the sync: 0 = decoded and checksum good, else the reason bits (tile_fast.h: kVerdict...)
u32 fastBandVerdict(const u8* hCell, u32 epoch, u32* blobEnd)
{
  FastDecodeParams hp;
  memcpy(&hp, hCell + kCellParams, sizeof(hp));
  u32 cells[4];
  memcpy(cells, hCell + kCellFallback, 16);
  u32 fb = fastFlagBits(cells, epoch);
  if (!hp.ok) fb |= kVerdictNotOurs;
  else if (!fb && !hp.checksumOk) fb |= kVerdictBadChecksum;
  if (blobEnd) *blobEnd = hp.blobEnd;
  return fb;
}

// Device-resident single-band blobs: everything is enqueued before a single byte of the blob has been seen by the
// host (the header is checked by the kernels); one synchronisation.  false: nothing was enqueued (ticket.form == kFormGeneral),
// the caller goes the long way (header read, general kernels, exact status codes).
bool decodeEnqueueStreaming(Context& ctx, const DecodeRequest& rq, u8* slot, StreamTicket& ticket)
{
  ticket = StreamTicket();
  const int dt = rq.dt, nRows = rq.nRows, nCols = rq.nCols;
  if (!slot || !rq.dBlob || rq.hBlob || rq.nBands != 1 || rq.nDepth != 1 || rq.blobSize < 70 || !rq.dOut) return false;
  if (!fastDecodeEligible(dt, 6, 8, nRows, nCols, 1, true)) return false;
  if (((uintptr_t)rq.dBlob & 15) || ((uintptr_t)rq.dOut & 15)) return false;
  hipStream_t st = ctx.activeStream();
  ctx.reset();
  if (!ctx.reserve(fastBandWorkspace(nRows, nCols, rq.blobSize) + 4096)) return false;
  const size_t cellsBytes = 64 + kCellBytes;
  static_assert(64 + kCellBytes <= Context::kAsyncSlotBytes, "a verdict fits a pinned slot");
  u8* dCells = ctx.allocT<u8>(cellsBytes);
  if (!dCells) return false;
  StreamTicket t;
  t.epoch = ctx.nextEpoch();
  t.shape = { dt, nRows, nCols };
  // (the kernels write the verdict -- header check, checksum, flags -- through to `slot`, pinned host memory, as well as to
  // the device cell they read it back from: a copy kernel behind the decode would cost every call 4 us.  The slot is wiped
  // first: if a launch fails, what the operation that had the slot before left there must not read as this one's "ok")
  memset(slot + 64, 0, kCellBytes);
  (void)hipGetLastError();
  t.form = ctx.tiers.pick(rq.maxForm, t.shape);
  if (t.form <= kFormGeneral) return false;
  if (!launchFastBand(ctx, t, rq.dBlob, rq.blobSize, rq.dOut, dCells + 64, slot + 64)) return false;
  if (hipGetLastError() != hipSuccess) { ctx.lastError = "lerc_amd: a streaming decode kernel could not be launched"; return false; }
  if (rq.nMasks > 0 && rq.dValidBytes) hipMemsetAsync(rq.dValidBytes, 1, (size_t)nRows * nCols, st);    // numValid == nPix or no verdict
  ticket = t;
  return true;
}

bool decodeStreamingVerdict(Context& ctx, const u8* slot, const StreamTicket& ticket, u32* bits)
{
  if (ctx.profOn()) ctx.profCollect();
  u32 blobEnd = 0;
  const u32 verdict = fastBandVerdict(slot + 64, ticket.epoch, &blobEnd);
  if (bits) *bits = verdict;
  if (verdict & kVerdictGaveUp) ctx.wipePersistentState();    // (a workgroup gave up waiting: the checksum accumulators may hold residue)
  if (ctx.tiers.judge(ticket, verdict, blobEnd)) return true;
  char msg[128];
  snprintf(msg, sizeof(msg), "streaming decode (form %d) handed the blob on (reason bits 0x%x)", ticket.form, verdict);
  ctx.lastNote = msg;
  return false;
}

// The same with the wait in the middle.  handled == false: nothing was decided, the caller goes the long way; ticket.form says
// whether (and which of) the streaming kernels were tried.
static u32 decodeSpeculative(Context& ctx, const DecodeRequest& rq, bool& handled, StreamTicket& ticket, u32* bits = nullptr)
{
  handled = false;
  u8* pin = (u8*)ctx.pinned(64 + kCellBytes);
  ticket = StreamTicket();
  if (!pin || !decodeEnqueueStreaming(ctx, rq, pin, ticket)) return kOk;
  if (!ctx.sync()) return kFailed;
  handled = decodeStreamingVerdict(ctx, pin, ticket, bits);
  return kOk;
}

// What a host-pointer call may send through decodeSpeculativeToHost -- the header says so: one band, every pixel valid, 8 x 8
// blocks, nDepth 1, the call's own shape and type, neither constant nor lossless-raw.
bool speculativeDecodeEligible(const Header& hd, const DecodeRequest& rq)
{
  const size_t nPix = (size_t)rq.nRows * rq.nCols;
  return rq.nBands == 1 && rq.nDepth == 1 && !rq.hUsesNoData && hd.version >= 3 && hd.nRows == rq.nRows
    && hd.nCols == rq.nCols && hd.nDepth == 1 && hd.dt == rq.dt && hd.mbSize == 8 && hd.nBlobsMore == 0
    && (size_t)hd.numValid == nPix && (unsigned)hd.blobSize <= rq.blobSize && hd.maxZErr > 0 && hd.zMin != hd.zMax;
}

// Host-pointer calls on a device copy of the blob: the same, with the pixels' (and the mask bytes') way back to the host
// enqueued behind the kernels, so that the calling thread waits once.  handled == false: the device did not vouch for
// what it wrote (the caller goes the long way and overwrites it).
u32 decodeSpeculativeToHost(Context& ctx, const DecodeRequest& rq, void* hOut, size_t outBytes, u8* hMask, size_t maskBytes, bool& handled, StreamTicket& ticket)
{
  handled = false;
  ticket = StreamTicket();
  u8* pin = (u8*)ctx.pinned(64 + kCellBytes);
  if (!pin || !decodeEnqueueStreaming(ctx, rq, pin, ticket)) return kOk;
  hipStream_t st = ctx.activeStream();
  hipMemcpyAsync(hOut, rq.dOut, outBytes, hipMemcpyDeviceToHost, st);
  if (hMask && rq.dValidBytes) hipMemcpyAsync(hMask, rq.dValidBytes, maskBytes, hipMemcpyDeviceToHost, st);
  if (!ctx.sync()) return kFailed;
  handled = decodeStreamingVerdict(ctx, pin, ticket);
  if (handled) { ctx.pathCount[2]++; ctx.lastDecodeStreamed = true; }
  return kOk;
}

u32 decodeDevice(Context& ctx, const DecodeRequest& rq)
{
  // tiers: the scanning decoder, the walking one-launch decoder, the two-launch form (each follows streams the one in front cannot), the general kernels
  ctx.scanOffsetsBan = false;
  DecodeTiers& tiers = ctx.tiers;
  const RasterShape shape = { rq.dt, rq.nRows, rq.nCols };
  int level = rq.noStreaming ? (int)kFormGeneral : tiers.pick(rq.maxForm, shape);
  // A band whose header says "not for the streaming kernels" (a mask, another mode) costs the blind attempt a launch and a wait before
  // the host reads the header itself.  The bands of one job are alike: after such a refusal the next few requests of that shape go
  // to the header-reading path at once (which still hands an unmasked band to the streaming kernels, a header read later).
  const bool blind = !tiers.notBlind.take(shape);
  while (blind && level > kFormGeneral)
  {
    bool handled = false;
    DecodeRequest r = rq;
    r.maxForm = level;
    u32 bits = 0;
    StreamTicket ticket;
    const u32 src = decodeSpeculative(ctx, r, handled, ticket, &bits);
    if (src != kOk) return src;
    if (handled) { ctx.pathCount[2]++; return kOk; }
    if (ticket.form == kFormGeneral) break;    // (not a request the streaming kernels take blind: decodeBands looks at every band)
    if (bits == kVerdictBadChecksum) return kFailed;    // (decoded by the streaming kernels, and the checksum is wrong: no other tier would say anything else)
    if (bits & kVerdictNotOurs) { tiers.notBlind.open(shape, DecodeTiers::kBlindSkip); break; }    // (a mask, another mode: the other forms would say the same)
    level = tiers.below(level, shape);
  }
  bool fellBack = false;
  u32 rc = decodeBands(ctx, rq, level, fellBack);
  bool repeated = false;
  while (rc == kOk && fellBack && level > kFormGeneral)
  {
    level = tiers.below(level, shape);
    repeated = level == kFormGeneral;
    rc = decodeBands(ctx, rq, level, fellBack);
  }
  if (rc == kOk) ctx.pathCount[(repeated || !ctx.lastDecodeStreamed) ? 3 : 2]++;
  return rc;
}

// ------------------------------------------------------------------------------------------------
// A mosaic's worth of independent blobs (one per tile, all of one shape and type) in one call.  Blobs the
// streaming kernels refuse (masked, constant, other shapes, damaged ...) are decoded one by one afterwards, which
// also produces the exact status for a bad one.
// ------------------------------------------------------------------------------------------------
u32 decodeTilesDevice(Context& ctx, const TilesDecodeRequest& rq)
{
  if (!rq.dArena || !rq.hOffsets || !rq.hSizes || !rq.dOut || rq.nTiles <= 0 || rq.nRows <= 0 || rq.nCols <= 0 || rq.dt < 0 || rq.dt > DT_Double)
    return kWrongParam;
  if (tilesBytesDecodeEligible(rq)) return decodeTilesBytes(ctx, rq);
  const int tbytes = dtSize(rq.dt);
  const u64 tileElems = (u64)rq.nRows * (u64)rq.nCols;
  const RasterShape shape = { rq.dt, rq.nRows, rq.nCols };
  int batchForm = kFormGeneral;    // (no batch launch yet)
  auto decodeOne = [&](int t) -> u32
  {
    DecodeRequest one;
    one.dBlob = rq.dArena + rq.hOffsets[t]; one.blobSize = rq.hSizes[t]; one.dt = rq.dt; one.nDepth = 1; one.nCols = rq.nCols;
    one.nRows = rq.nRows; one.nBands = 1; one.nMasks = 0; one.dValidBytes = nullptr;
    one.dOut = (u8*)rq.dOut + (size_t)t * tileElems * tbytes;
    if (batchForm > kFormGeneral) one.startAt(ctx.tiers.below(batchForm, shape));    // the batch's kernels have just been tried: the next form (or, if the batch was the two-launch form, the general kernels); no batch launch: every form
    const u32 rc = decodeDevice(ctx, one);
    ctx.tileBatchCount[3]++;
    if (rc == kFailed)    // (a failed decode leaves zeros, include/lerc_amd.h: the streaming kernels may have written pixels of a damaged blob)
    {
      hipMemsetAsync(one.dOut, 0, (size_t)tileElems * tbytes, ctx.activeStream());
      hipStreamSynchronize(ctx.activeStream());
    }
    return rc;
  };
  bool fastOk = fastDecodeEligible(rq.dt, 6, 8, rq.nRows, rq.nCols, 1, true) && ((uintptr_t)rq.dArena & 15) == 0
    && ((uintptr_t)rq.dOut & 15) == 0 && ((tileElems * tbytes) % 16 == 0 || rq.nRows % 8 != 0 || rq.nCols % 8 != 0);    // (ragged tiles: pixel-wise stores)
  u32 maxSize = 0;
  for (int t = 0; t < rq.nTiles; t++)
  {
    if (rq.hOffsets[t] % 16 != 0 || rq.hSizes[t] < 70) fastOk = false;
    maxSize = std::max(maxSize, rq.hSizes[t]);
  }
  if (!fastOk)
  {
    for (int t = 0; t < rq.nTiles; t++) { const u32 rc = decodeOne(t); if (rc != kOk) return rc; }
    return kOk;
  }

  hipStream_t st = ctx.activeStream();
  const size_t perTile = fastBandWorkspace(rq.nRows, rq.nCols, maxSize, 1) - (1u << 16) + sizeof(FastDecodeParams) + 64;
  const int maxBatch = (int)std::max<size_t>(1, std::min<size_t>((size_t)rq.nTiles, ((size_t)1024 << 20) / perTile));
  std::vector<int> redo;
  for (int t0 = 0; t0 < rq.nTiles; t0 += maxBatch)
  {
    const int n = std::min(maxBatch, rq.nTiles - t0);
    if (!ctx.reserve(fastBandWorkspace(rq.nRows, rq.nCols, maxSize, (u32)n) + (size_t)n * (sizeof(FastDecodeParams) + 64) + 8192)) return kFailed;
    // verdict cells [status 64][params n][fallback 16 n], then the offsets / sizes the kernels index by tile
    const size_t cellsBytes = 64 + (size_t)n * (sizeof(FastDecodeParams) + 16);
    u8* dCells = ctx.allocT<u8>(cellsBytes);
    u64* dOff = ctx.allocT<u64>((size_t)n + 1);
    u32* dSize = ctx.allocT<u32>((size_t)n + 1);
    // (pinned: the tables on their way up, then -- a region of its own, so that nobody has to wait in between -- the verdicts' way back)
    const size_t upBytes = ((size_t)n * 12 + 64 + 63) & ~(size_t)63;
    u8* pinUp = (u8*)ctx.pinned(upBytes + cellsBytes);
    if (!dCells || !dOff || !dSize || !pinUp) return kFailed;
    u8* pin = pinUp + upBytes;
    u64* hOff = reinterpret_cast<u64*>(pinUp);
    u32* hSize = reinterpret_cast<u32*>(pinUp + (size_t)n * 8);
    for (int i = 0; i < n; i++) { hOff[i] = rq.hOffsets[t0 + i]; hSize[i] = rq.hSizes[t0 + i]; }
    hipMemcpyAsync(dOff, hOff, (size_t)n * 8, hipMemcpyHostToDevice, st);
    hipMemcpyAsync(dSize, hSize, (size_t)n * 4, hipMemcpyHostToDevice, st);
    FastDecodeParams* dParams = reinterpret_cast<FastDecodeParams*>(dCells + 64);
    u32* dFallback = reinterpret_cast<u32*>(dCells + 64 + (size_t)n * sizeof(FastDecodeParams));
    // (batches count late, form 3: a tile is a handful of pieces -- nothing to gain from early counts --, and one piece in some thousands
    // has a false survivor that its mending strikes: with early counts that tile would be decoded once more by itself, a wait and
    // a launch of its own; 65 536 tiles: 0.386 of peak against 0.456)
    StreamTicket ticket;
    ticket.epoch = ctx.nextEpoch();
    ticket.shape = shape;
    ticket.form = batchForm = ctx.tiers.pick(kFormScan, shape);
    const u32 epoch = ticket.epoch;
    if (!launchFastBands(ctx, ticket, rq.dArena, maxSize, (u32)n, dOff, dSize, (u8*)rq.dOut + (size_t)t0 * tileElems * tbytes, dParams, dFallback))
      return kFailed;
    hipMemcpyAsync(pin, dCells, cellsBytes, hipMemcpyDeviceToHost, st);
    if (!ctx.sync()) return kFailed;
    if (ctx.profOn()) ctx.profCollect();
    const FastDecodeParams* hp = reinterpret_cast<const FastDecodeParams*>(pin + 64);
    const u32* hfb = reinterpret_cast<const u32*>(pin + 64 + (size_t)n * sizeof(FastDecodeParams));
    redo.clear();
    bool gaveUp = false;
    for (int i = 0; i < n; i++) gaveUp = gaveUp || (fastFlagBits(hfb + 4 * i, epoch) & kVerdictGaveUp) != 0u;
    if (gaveUp) ctx.wipePersistentState();    // (a workgroup gave up waiting: the checksum accumulators may hold residue)
    for (int i = 0; i < n; i++)
    {
      const u32 bits = fastFlagBits(hfb + 4 * i, epoch);
      const bool good = hp[i].ok && !bits && hp[i].checksumOk;
      if (good) { ctx.pathCount[2]++; ctx.tileBatchCount[2]++; }
      else
      {
        if (redo.empty())
        {
          char msg[160];
          snprintf(msg, sizeof(msg), "tile %d of the batch went to the general path (header ok %u, reason bits 0x%x, checksum ok %u)",
                   t0 + i, hp[i].ok, bits, hp[i].checksumOk);
          ctx.lastNote = msg;
        }
        redo.push_back(t0 + i);
      }
    }
    // (more than an eighth of the tiles went on: tiles this form does not follow, the next batches start one tier down)
    ctx.tiers.judgeBatch(ticket, (u32)(n - (int)redo.size()), redo.size() > (size_t)n / 8);
    for (int t : redo) { const u32 rc = decodeOne(t); if (rc != kOk) return rc; }    // (reuses the workspace: the batch is done with it)
  }
  return kOk;
}

}    // namespace lerc
