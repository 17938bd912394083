// codec_encode.cpp -- lerc_encode() on device-resident pixels: the entry points and the streaming launches.
//
// A request the streaming kernels take is decided on the device; every other one, and every band they hand
// back, goes band by band through encodeBands() (codec_encode_band.cpp).
#include "codec.h"
#include "huffman.h"
#include "fpl.h"
#include "tile_fast.h"
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>

namespace lerc {

// ------------------------------------------------------------------------------------------------
// streaming kernels: buffers + launches for nTiles rasters of one shape (a single raster is nTiles == 1)
// ------------------------------------------------------------------------------------------------
struct FastEncodeLaunch
{
  FastEncodeBuffers fb;
  FastBatch batch;
  BandParams bp;
  u32 cand;
  double maxZErr;
};

// LERC_AMD_ENCODE_LAUNCHES=2 keeps the two-launch form (statistics, then scan + pack) for a single raster: a tuning / test knob
bool fastEncodeOneLaunch()
{
  static const bool one = []() { const char* e = getenv("LERC_AMD_ENCODE_LAUNCHES"); return !(e && e[0] == '2'); }();
  return one;
}

static size_t fastEncodeWorkspace(int nRows, int nCols, u32 nTiles)
{
  const size_t nWG = fastEncodeNumWG(nRows, nCols);
  return (size_t)nTiles * (nWG * (kFastBlocksPerWG * sizeof(FastBlockDesc) + 64) + kFastPrefixStage + sizeof(FastEncodeResult)
                           + (fastScanGroups((u32)nWG) + 1) * (4 + 8 * kScanPartWords) + fastPackGroups((u32)nWG) * 16 + fastTicketStride((u32)nWG) * 4 + 256)
    + 65536;
}

static bool prepareFastEncode(Context& ctx, int dt, int nRows, int nCols, double maxZErr, u32 nTiles, u64 tileElems, bool arena,
                              FastEncodeLaunch& fl)
{
  const u32 nWG = fastEncodeNumWG(nRows, nCols);
  const bool isFlt = dt >= DT_Float;
  const size_t nT = nTiles;
  FastEncodeBuffers& fb = fl.fb;
  fl.batch.nTiles = nTiles; fl.batch.nWG = nWG; fl.batch.tileElems = tileElems; fl.batch.nBlobsMore = 0;
  memset(&fb.solo, 0, sizeof(fb.solo));
  memset(&fb.fused, 0, sizeof(fb.fused));
  if (nTiles == 1 && !arena && fastSoloOk(dt, nRows, nCols))
  {
    // one raster: two launches, the pack step's first blocks scan and decide (tile_fast.h)
    memset(&fb, 0, sizeof(fb));
    const bool form = fastEncodeOneLaunch();
    const u32 nWGf = form ? fastFusedNumWG(dt, nRows, nCols) : nWG;    // (the one-launch form counts its own workgroups)
    const size_t nGroups = std::max(fastPackGroups(nWG), fastPackGroups(nWGf)), nFused = fastFusedGroups(std::max(nWG, nWGf));
    // (counters: the pack accumulators, then the one-launch form's key cells; cells: a cell per workgroup, then the
    // one-launch form's group cells and first-row errors)
    u8* counters = ctx.persistentState(0, (nGroups + 1) * 8 + 2 * nGroups * 8 + 256);
    u8* cells = ctx.persistentState(1, ((size_t)std::max(nWG, nWGf) + 2 * nFused + 16) * 8 + 256);
    fb.desc = ctx.allocT<FastBlockDesc>((size_t)nWG * kFastBlocksPerWG);
    fb.wgSize = ctx.allocT<u32>(fastWgStride(nWG) + 4);
    fb.wgMinKey = ctx.allocT<u64>(nWG + 4);
    fb.wgMaxKey = ctx.allocT<u64>(nWG + 4);
    fb.wgFlags = ctx.allocT<u32>(nWG + 4);
    fb.tickets = ctx.allocT<u32>(fastTicketStride(nWG) + 4);
    fb.result = ctx.allocT<FastEncodeResult>(1);
    fb.prefixStage = ctx.allocT<u8>(kFastPrefixStage);
    if (!counters || !cells || !fb.desc || !fb.wgSize || !fb.wgMinKey || !fb.wgMaxKey || !fb.wgFlags || !fb.tickets || !fb.result || !fb.prefixStage)
      return false;
    fb.packPart = (u64*)counters;
    fb.solo.cells = (u64*)cells;
    if (form)
    {
      const size_t nCell = std::max(nWG, nWGf);
      fb.fused.sizeCell = (u64*)cells;
      fb.fused.baseCell = (u64*)cells + nCell;
      fb.fused.totalCell = (u64*)cells + nCell + nFused;
      fb.fused.raise = (u64*)cells + nCell + 2 * nFused;
      fb.fused.packPart = (u64*)counters;
      fb.fused.keyPart = (u64*)counters + nGroups + 1;
      fb.fused.nWG = nWGf;
    }
  }
  else
  {
    fb.desc = ctx.allocT<FastBlockDesc>(nT * nWG * kFastBlocksPerWG);
    fb.wgSize = ctx.allocT<u32>(nT * fastWgStride(nWG) + 4);
    fb.wgBase = ctx.allocT<u32>(nT * fastWgStride(nWG) + 4);
    fb.wgMinKey = ctx.allocT<u64>(nT * nWG + 4);
    fb.wgMaxKey = ctx.allocT<u64>(nT * nWG + 4);
    fb.wgFlags = ctx.allocT<u32>(nT * nWG + 4);
    fb.groupBase = ctx.allocT<u32>(nT * (fastScanGroups(nWG) + 1) + 4);
    fb.scanPart = ctx.allocT<u64>(kScanPartWords * nT * fastScanGroups(nWG) + 4);
    fb.packPart = ctx.allocT<u64>(nT * fastPackGroups(nWG) + 4);
    fb.tickets = ctx.allocT<u32>(nT * fastTicketStride(nWG) + 4);
    fb.result = ctx.allocT<FastEncodeResult>(nT);
    fb.prefixStage = ctx.allocT<u8>(nT * kFastPrefixStage);
    fb.tileOffset = arena ? ctx.allocT<u64>(nT + 1) : nullptr;
    if (!fb.desc || !fb.wgSize || !fb.wgBase || !fb.wgMinKey || !fb.wgMaxKey || !fb.wgFlags || !fb.result
      || !fb.groupBase || !fb.scanPart || !fb.packPart || !fb.tickets
      || !fb.prefixStage || (arena && !fb.tileOffset))
      return false;
  }
  fl.cand = 0;
  if (isFlt)
  {
    static const double errCand[9] = { 1, 0.5, 0.1, 0.05, 0.01, 0.005, 0.001, 0.0005, 0.0001 };
    for (int c = 0; c < 9; c++) if (errCand[c] / 2 > maxZErr) fl.cand |= 1u << c;
  }
  BandParams& bp = fl.bp;
  memset(&bp, 0, sizeof(bp));
  bp.nRows = nRows; bp.nCols = nCols; bp.nDepth = 1; bp.dt = dt; bp.version = kCodecVersion;
  bp.mb = 8; bp.nTV = (nRows + 7) / 8; bp.nTH = (nCols + 7) / 8;
  bp.allValid = 1;
  bp.maxQ = maxValToQuantize(dt);
  bp.maxZErr = isFlt ? maxZErr : std::max(0.5, floor(maxZErr));
  bp.scale = 1 / (2 * bp.maxZErr);
  bp.invScale = 2 * bp.maxZErr;
  bp.intLossless = (!isFlt && bp.maxZErr == 0.5) ? 1 : 0;
  fl.maxZErr = maxZErr;
  return true;
}

static void runFastEncode(Context& ctx, const FastEncodeLaunch& fl, const void* dData, u8* dOut, u64 capacity, u64 arenaBase)
{
  // one kernel per stage (and per profiling group): statistics (+ first-row rounding errors), scan + decide (+ tile
  // placement for batches), pack + checksum
  static const char* kStage[3] = { "fast_stats_sizes", "fast_scan_decide", "fast_pack" };
  const bool ragged = fl.bp.nRows % 8 != 0 || fl.bp.nCols % 8 != 0;
  if (fl.fb.fused.sizeCell && (dOut || ragged))    // one raster, one launch (size queries: only where the two-launch form cannot go)
  {
    ProfScope ps(ctx, "fast_encode1");
    FastEncodeBuffers fb = fl.fb;
    fb.fused.epoch = ctx.nextEpoch();    // (never 0, the tag of a cell nobody has written yet)
    fb.fused.publishEpoch = (fastTestGiveUp() & 1u) ? fb.fused.epoch ^ 0x5A5A5A5Au : fb.fused.epoch;
    fb.fused.spinLimit = (fastTestGiveUp() & 1u) ? 8u : (1u << 22);
    launchFastEncode(0, fl.bp, fl.maxZErr, fl.cand, dData, dOut, capacity, arenaBase, fb, fl.batch, ctx.activeStream());
    return;
  }
  // (no output buffer: the size is known after the decisions -- one raster: the pack step's last workgroup takes them)
  const int nStages = (dOut || fl.fb.solo.cells) ? 3 : 2;
  for (int stage = 0; stage < nStages; stage++)
  {
    if (stage == 1 && fl.fb.solo.cells) continue;    // (one raster: the pack step scans and decides itself)
    ProfScope ps(ctx, kStage[stage]);
    FastEncodeBuffers fb = fl.fb;
    if (stage == 2 && fb.solo.cells) fb.solo.epoch = ctx.nextEpoch();    // (never 0, the tag of a cell nobody has written yet)
    launchFastEncode(stage, fl.bp, fl.maxZErr, fl.cand, dData, dOut, capacity, arenaBase, fb, fl.batch, ctx.activeStream());
  }
}

// single band requests the streaming kernels can take (the same test encodeDevice makes)
static bool encodeStreamingOk(const EncodeRequest& rq)
{
  bool anyNoData = false;
  if (rq.hUsesNoData) for (int i = 0; i < rq.nBands; i++) anyNoData = anyNoData || rq.hUsesNoData[i] != 0;
  return !anyNoData && rq.version == kCodecVersion && rq.maxZErr != 777 && ((uintptr_t)rq.dOut & 15) == 0 && ((uintptr_t)rq.dData & 15) == 0
    && fastEncodeEligible(rq.dt, rq.nRows, rq.nCols, rq.nDepth, rq.nMasks > 0, rq.maxZErr, fastEncodeOneLaunch());
}

bool encodeEnqueueStreaming(Context& ctx, const EncodeRequest& rq, u8* slot)
{
  if (!slot || rq.nBands != 1 || !encodeStreamingOk(rq)) return false;
  ctx.reset();
  if (!ctx.reserve(fastEncodeWorkspace(rq.nRows, rq.nCols, 1) + (1u << 16))) return false;
  FastEncodeLaunch fl;
  if (!prepareFastEncode(ctx, rq.dt, rq.nRows, rq.nCols, rq.maxZErr, 1, 0, false, fl)) return false;
  // (one raster: the deciding block and the last workgroup write the result straight into `slot`, pinned host memory -- no
  // kernel reads it, and a copy kernel behind the encode would cost every call 4 us)
  const bool direct = fl.fb.solo.cells != nullptr;
  if (direct)
  {
    // (wiped first: if a launch fails, what the operation that had the slot before left there must not read as this one's
    // verdict -- "redo" sends the request to the general path, which reports what is wrong)
    FastEncodeResult init;
    memset(&init, 0, sizeof(init));
    init.redo = 1u; init.redoReason = 0x80000000u;
    memcpy(slot, &init, sizeof(init));
    fl.fb.result = reinterpret_cast<FastEncodeResult*>(slot);
  }
  (void)hipGetLastError();
  runFastEncode(ctx, fl, rq.dData, rq.dOut, rq.dOut ? (u64)rq.outCapacity : ~0ull, 0);
  if (hipGetLastError() != hipSuccess) { ctx.lastError = "lerc_amd: a streaming encode kernel could not be launched"; return false; }
  return direct || hipMemcpyAsync(slot, fl.fb.result, sizeof(FastEncodeResult), hipMemcpyDeviceToHost, ctx.activeStream()) == hipSuccess;
}

void encodeStreamingVerdict(Context& ctx, const EncodeRequest& rq, const u8* slot, bool& redo, u32& status, u32& numBytesNeeded, u32& numBytesWritten)
{
  FastEncodeResult hres;
  memcpy(&hres, slot, sizeof(hres));
  if (ctx.profOn()) ctx.profCollect();
  redo = false; status = kOk;
  if (!hres.redo && !hres.stuck)
  {
    ctx.pathCount[0]++;
    numBytesNeeded = hres.blobSize;
    numBytesWritten = rq.dOut ? hres.blobSize : 0;
    return;
  }
  {
    char msg[160];
    snprintf(msg, sizeof(msg), "streaming encode handed the band to the general kernels (redo %u, reason bits 0x%x, stuck %u, blob %u bytes)",
             hres.redo, hres.redoReason, hres.stuck, hres.blobSize);
    ctx.lastNote = msg;
  }
  if (hres.stuck) ctx.wipePersistentState();
  if (rq.dOut && hres.redoReason == 64u && hres.blobSize > rq.outCapacity) { status = kBufferTooSmall; return; }
  redo = true;
}

u32 encodeDevice(Context& ctx, const EncodeRequest& rq, u32& numBytesNeeded, u32& numBytesWritten)
{
  numBytesNeeded = numBytesWritten = 0;
  const int tb = dtSize(rq.dt);
  const i64 nPix = (i64)rq.nRows * rq.nCols;
  const size_t maskBytes = (size_t)((nPix + 7) >> 3) + 64;
  const size_t nPos8 = (size_t)((rq.nRows + 7) / 8) * ((rq.nCols + 7) / 8);
  // workspace: two bit masks, block sizes + offsets + scan scratch, one-sweep ranks, Huffman scratch, small stuff
  size_t need = 2 * maskBytes + 3 * (nPos8 + 1024) * 4 + 3 * ((size_t)(nPix >> 5) + 1024) * 4
    + (rq.dt <= DT_Byte ? huffmanScratchBytes(nPix, rq.nDepth) : 0) + (size_t)rq.nDepth * 16 + (1u << 16);
  bool anyNoData = false;
  if (rq.hUsesNoData) for (int i = 0; i < rq.nBands; i++) anyNoData = anyNoData || rq.hUsesNoData[i] != 0;
  if (anyNoData && !rq.hNoDataValues) return kWrongParam;
  if (anyNoData) need += (size_t)nPix * rq.nDepth * tb + (size_t)nPix + 8192;
  if (rq.nMasks > 0 || rq.dt >= DT_Float) need += maskRleScratchBytes(maskBytes) + (4u << 20) + 8192;    // a large mask is run-length coded on the device
  if (rq.dt >= DT_Float && (rq.maxZErr == 0 || anyNoData) && rq.version >= 6) need += fplEncodeScratchBytes(nPix * rq.nDepth, tb);
  // (a size query, dOut == nullptr, takes the first two steps of the streaming path: statistics and decisions)
  if (rq.version < 2 || rq.version > kCodecVersion) return kWrongParam;
  if (rq.version < 6 && anyNoData) return kWrongParam;    // Lerc.cpp:341-344
  if (rq.version < 4 && rq.nDepth > 1) return kFailed;    // Lerc2::Set refuses (Lerc2.cpp:85-86)
  const bool fastOk = !anyNoData && rq.version == kCodecVersion && rq.maxZErr != 777 && ((uintptr_t)rq.dOut & 15) == 0 && ((uintptr_t)rq.dData & 15) == 0
    && fastEncodeEligible(rq.dt, rq.nRows, rq.nCols, rq.nDepth, rq.nMasks > 0, rq.maxZErr, fastEncodeOneLaunch());
  const u32 nWG = fastOk ? fastEncodeNumWG(rq.nRows, rq.nCols) : 0;
  need += fastOk ? fastEncodeWorkspace(rq.nRows, rq.nCols, 1) : 0;
  const size_t bandCap = (size_t)nPix * tb + 4096;    // a band's blob never exceeds its raw form by more than the small sections
  if (fastOk && rq.nBands > 1 && rq.dOut) need += bandCap + 256;
  (void)nWG;
  if (!ctx.reserve(need)) return kFailed;
  (void)tb;

  // ---- streaming path: everything is decided on the device, one synchronisation at the end.  If an
  // assumption fails (NaN, all-integer floats, raisable error bound, constant image, 16 x 16 retry,
  // raw fallback) the device says so and the general path below redoes the band.
  if (fastOk && rq.nBands > 1)
  {
    // several bands: each is a blob of its own with "bands to follow" in its header (Lerc.cpp:628-789); a band is packed
    // into 16-byte aligned scratch (its place in the output is wherever the band before it ended) and copied over
    hipStream_t st = ctx.activeStream();
    FastEncodeLaunch fl;
    if (!prepareFastEncode(ctx, rq.dt, rq.nRows, rq.nCols, rq.maxZErr, 1, 0, false, fl)) return kFailed;
    u8* dBandBlob = rq.dOut ? ctx.allocT<u8>(bandCap) : nullptr;
    FastEncodeResult* pinRes = (FastEncodeResult*)ctx.pinned(sizeof(FastEncodeResult));
    if (!pinRes || (rq.dOut && !dBandBlob)) return kFailed;
    u64 total = 0;
    bool redo = false;
    for (int iBand = 0; iBand < rq.nBands && !redo; iBand++)
    {
      fl.batch.nBlobsMore = (u32)(rq.nBands - 1 - iBand);
      const u8* dBand = (const u8*)rq.dData + (size_t)iBand * nPix * tb;
      const bool direct = fl.fb.solo.cells != nullptr;    // (the kernels write the result into pinned memory themselves)
      if (direct) { memset(pinRes, 0, sizeof(*pinRes)); pinRes->redo = 1u; pinRes->redoReason = 0x80000000u; fl.fb.result = pinRes; }
      runFastEncode(ctx, fl, dBand, dBandBlob, dBandBlob ? (u64)bandCap : ~0ull, 0);
      if (!direct) hipMemcpyAsync(pinRes, fl.fb.result, sizeof(FastEncodeResult), hipMemcpyDeviceToHost, st);
      if (!ctx.sync()) return kFailed;
      if (pinRes->stuck) ctx.wipePersistentState();
      if (pinRes->redo || pinRes->stuck) { redo = true; break; }
      const u32 bandBytes = pinRes->blobSize;
      if (total + bandBytes > (u64)UINT_MAX) return kDimsTooLarge;
      if (rq.dOut)
      {
        if (total + bandBytes > rq.outCapacity) return kBufferTooSmall;
        hipMemcpyAsync(rq.dOut + total, dBandBlob, bandBytes, hipMemcpyDeviceToDevice, st);
      }
      total += bandBytes;
    }
    if (ctx.profOn()) ctx.profCollect();
    if (!redo)
    {
      if (rq.dOut && !ctx.sync()) return kFailed;
      ctx.pathCount[0]++;
      numBytesNeeded = (u32)total;
      numBytesWritten = rq.dOut ? (u32)total : 0;
      return kOk;
    }
    ctx.reset();
  }
  else if (fastOk)
  {
    FastEncodeResult* pinRes = (FastEncodeResult*)ctx.pinned(sizeof(FastEncodeResult));
    if (!pinRes) return kFailed;
    if (!encodeEnqueueStreaming(ctx, rq, reinterpret_cast<u8*>(pinRes))) return kFailed;
    if (!ctx.sync()) return kFailed;
    bool redo = false;
    u32 status = kOk;
    encodeStreamingVerdict(ctx, rq, reinterpret_cast<const u8*>(pinRes), redo, status, numBytesNeeded, numBytesWritten);
    if (!redo) return status;
    ctx.reset();
  }

  return encodeBands(ctx, rq, numBytesNeeded, numBytesWritten);
}

// ------------------------------------------------------------------------------------------------
// A mosaic's worth of independent tiles in one call: every tile becomes its own blob (own header, ranges,
// checksum), byte for byte what encodeDevice() makes of it; the blobs go into one arena at 16-byte aligned offsets.
// Tiles the streaming kernels hand back (constant tiles, NaNs, ...) are encoded one by one behind their sub-batch.
// ------------------------------------------------------------------------------------------------
u32 encodeTilesDevice(Context& ctx, const TilesEncodeRequest& rq, u64& arenaUsed)
{
  arenaUsed = 0;
  if (!rq.dData || !rq.dArena || !rq.hOffsets || !rq.hSizes || rq.nTiles <= 0 || rq.nRows <= 0 || rq.nCols <= 0 || rq.dt < 0 || rq.dt > DT_Double
    || rq.maxZErr < 0 || (rq.slotBytes & 15u) != 0)
    return kWrongParam;
  if (tilesBytesEncodeEligible(rq)) return encodeTilesBytes(ctx, rq, arenaUsed);    // (8-bit: the Huffman decision, a tile per workgroup)
  const bool slotted = rq.slotBytes != 0;    // every tile has its place: no arena to fill front to back
  const int tb = dtSize(rq.dt);
  const u64 tileElems = (u64)rq.nRows * (u64)rq.nCols;
  // (tiles whose sides are no multiples of 8 -- 257 x 257 elevation tiles -- go through the one-launch encoder's ragged form, pixel by
  // pixel where rows do not start on 16-byte boundaries; whole-block tiles must lie 16 bytes apart)
  const bool raggedTile = rq.nRows % 8 != 0 || rq.nCols % 8 != 0;
  const bool fastOk = rq.maxZErr != 777 && ((uintptr_t)rq.dArena & 15) == 0 && ((uintptr_t)rq.dData & 15) == 0
    && (raggedTile ? fastEncodeOneLaunch() : (tileElems * tb) % 16 == 0)
    && fastEncodeEligible(rq.dt, rq.nRows, rq.nCols, 1, false, rq.maxZErr, raggedTile);
  u64 end = 0;    // arena bytes in use

  auto encodeOne = [&](int t) -> u32
  {
    end = slotted ? (u64)t * rq.slotBytes : (end + 15) & ~15ull;
    EncodeRequest one;
    one.dData = (const u8*)rq.dData + (size_t)t * tileElems * tb;
    one.dt = rq.dt; one.nDepth = 1; one.nCols = rq.nCols; one.nRows = rq.nRows; one.nBands = 1; one.nMasks = 0; one.dValidBytes = nullptr;
    one.maxZErr = rq.maxZErr;
    one.dOut = rq.dArena + end;
    one.outCapacity = (u32)std::min<u64>(slotted ? rq.slotBytes : (rq.arenaCapacity > end ? rq.arenaCapacity - end : 0), 0xFFFFFFFFull);
    u32 needed = 0, written = 0;
    const u32 rc = encodeDevice(ctx, one, needed, written);
    if (rc != kOk) return rc;
    rq.hOffsets[t] = end; rq.hSizes[t] = written;
    end += written;
    ctx.tileBatchCount[1]++;
    return kOk;
  };

  if (slotted && rq.arenaCapacity < (u64)rq.nTiles * rq.slotBytes) return kBufferTooSmall;
  if (!fastOk || (slotted && !fastEncodeOneLaunch()))
  {
    for (int t = 0; t < rq.nTiles; t++) { const u32 rc = encodeOne(t); if (rc != kOk) return rc; }
    arenaUsed = slotted ? (u64)rq.nTiles * rq.slotBytes : end;
    return kOk;
  }

  hipStream_t st = ctx.activeStream();
  std::vector<int> redo;
  if (fastEncodeOneLaunch())
  {
    // ---- the one-launch encoder, a tile per blockIdx.y: every tile's blob goes into a slot of its own (half the tile's raw
    // size: a tile that needs more is encoded by itself afterwards), then the tiles are placed and moved into the arena
    const u32 nWGt = fastFusedNumWG(rq.dt, rq.nRows, rq.nCols);
    const size_t cellWords = fastFusedCellWords(nWGt), counterWords = fastFusedCounterWords(nWGt);
    const u64 slotBytes = slotted ? rq.slotBytes : ((tileElems * tb / 2 + 4096) + 15) & ~15ull;
    const bool isFlt = rq.dt >= DT_Float;
    // one launch for tiles [t0, t0 + n), every blob in a slot of slotBytes; redoOut: the tiles it hands back, with the reason bits
    // An arena is filled WITHOUT slots and without a pass that moves the blobs: a tile's last workgroup claims the tile's room with an
    // atomic add on the batch's cursor (tile_fast.h: FastFused::arenaCursor), the tiles lie in the order of their claims.
    // LERC_AMD_TILE_ARENA=copy keeps the slots + k_fast_tile_copy form (a knob for A/B runs and tests).
    // (The emulator runs workgroups one after the other: a workgroup that waits for one BEHIND it waits for ever there.  Emulator builds keep
    // the copy form unless asked, and then give up after a few polls -- which is the hand-back path's test.)
#ifdef HIPSIM
    static const bool cursorMode = []() { const char* e = getenv("LERC_AMD_TILE_ARENA"); return e && strcmp(e, "cursor") == 0; }();
#else
    static const bool cursorMode = []() { const char* e = getenv("LERC_AMD_TILE_ARENA"); return !(e && strcmp(e, "copy") == 0); }();
#endif
    const bool direct = !slotted && cursorMode;
    auto runBatch = [&](int t0, int n, u64 slotBytes, std::vector<std::pair<int, u32> >& redoOut) -> u32
    {
      if (!ctx.reserve((size_t)n * (((slotted || direct) ? 0 : slotBytes) + sizeof(FastEncodeResult) + 8) + (1u << 16))) return kFailed;
      u8* cells = ctx.persistentState(1, (size_t)n * (cellWords + (direct ? 1 : 0)) * 8 + 256);
      u8* counters = ctx.persistentState(0, (size_t)n * counterWords * 8 + 256);
      u8* slots = slotted ? rq.dArena + (size_t)t0 * slotBytes : direct ? rq.dArena : ctx.allocT<u8>((size_t)n * slotBytes);
      // (the results and, behind them, the batch's cursor: cleared by one memset)
      FastEncodeResult* dRes = (FastEncodeResult*)ctx.alloc((size_t)n * sizeof(FastEncodeResult) + 16);
      u64* dCursor = dRes ? reinterpret_cast<u64*>(reinterpret_cast<u8*>(dRes) + (size_t)n * sizeof(FastEncodeResult)) : nullptr;
      static_assert(sizeof(FastEncodeResult) % 8 == 0, "the cursor behind the results is 8-byte aligned");
      u64* dOff = ctx.allocT<u64>((size_t)n + 1);
      if (!cells || !counters || !slots || !dRes || !dOff) return kFailed;
      FastEncodeLaunch fl;
      memset(&fl.fb, 0, sizeof(fl.fb));
      const u32 nG = fastFusedGroups(nWGt), nPG = fastPackGroups(nWGt);
      FastFused& f = fl.fb.fused;
      f.sizeCell = (u64*)cells; f.baseCell = f.sizeCell + nWGt; f.totalCell = f.baseCell + nG; f.raise = f.totalCell + nG;
      f.packPart = (u64*)counters; f.keyPart = f.packPart + nPG + 1;
      f.nWG = nWGt; f.nTiles = (u32)n; f.cellStride = (u32)cellWords; f.counterStride = (u32)counterWords;
      f.tileElems = tileElems; f.outStride = slotBytes;
      end = (end + 15) & ~15ull;
      if (direct)
      {
        f.outStride = 0;
        f.arenaCursor = dCursor;
        f.tileCell = (u64*)cells + (size_t)n * cellWords;    // (epoch-tagged, behind the tiles' own cells)
        f.tileOffset = dOff;
        f.arenaBase = end; f.arenaCapacity = rq.arenaCapacity;
      }
      f.epoch = ctx.nextEpoch();
      f.publishEpoch = (fastTestGiveUp() & 1u) ? f.epoch ^ 0x5A5A5A5Au : f.epoch;
      f.spinLimit = (fastTestGiveUp() & 1u) ? 8u : (1u << 22);
#ifdef HIPSIM
      if (direct) f.spinLimit = 64u;
#endif
      fl.fb.result = dRes;
      fl.batch.nTiles = (u32)n; fl.batch.nWG = nWGt; fl.batch.tileElems = tileElems; fl.batch.nBlobsMore = 0;
      fl.cand = 0;
      if (isFlt)
      {
        static const double errCand[9] = { 1, 0.5, 0.1, 0.05, 0.01, 0.005, 0.001, 0.0005, 0.0001 };
        for (int c = 0; c < 9; c++) if (errCand[c] / 2 > rq.maxZErr) fl.cand |= 1u << c;
      }
      BandParams& bp = fl.bp;
      memset(&bp, 0, sizeof(bp));
      bp.nRows = rq.nRows; bp.nCols = rq.nCols; bp.nDepth = 1; bp.dt = rq.dt; bp.version = kCodecVersion;
      bp.mb = 8; bp.nTV = (rq.nRows + 7) / 8; bp.nTH = (rq.nCols + 7) / 8;
      bp.allValid = 1;
      bp.maxQ = maxValToQuantize(rq.dt);
      bp.maxZErr = isFlt ? rq.maxZErr : std::max(0.5, floor(rq.maxZErr));
      bp.scale = 1 / (2 * bp.maxZErr);
      bp.invScale = 2 * bp.maxZErr;
      bp.intLossless = (!isFlt && bp.maxZErr == 0.5) ? 1 : 0;
      fl.maxZErr = rq.maxZErr;
      (void)hipGetLastError();
      hipMemsetAsync(dRes, 0, (size_t)n * sizeof(FastEncodeResult) + 16, st);    // (the kernels raise `stuck`, nobody else clears it; the cursor)
      {
        ProfScope ps(ctx, "fast_encode1");
        launchFastEncode(0, fl.bp, fl.maxZErr, fl.cand, (const u8*)rq.dData + (size_t)t0 * tileElems * tb, slots, direct ? rq.arenaCapacity : slotBytes, 0, fl.fb, fl.batch, st);
      }
      if (!slotted && !direct)
      {
        ProfScope ps(ctx, "fast_tile_move");
        launchFastTileCopy(dRes, dOff, slots, slotBytes, slotBytes, rq.dArena, (u32)n, end, rq.arenaCapacity, st);
      }
      if (hipGetLastError() != hipSuccess) { ctx.lastError = "lerc_amd: a streaming encode kernel could not be launched"; return kFailed; }
      const size_t resBytes = (size_t)n * sizeof(FastEncodeResult) + 16, offBytes = ((size_t)n + 1) * 8;    // (+ the cursor)
      u8* pin = (u8*)ctx.pinned(resBytes + offBytes);
      if (!pin) return kFailed;
      hipMemcpyAsync(pin, dRes, resBytes, hipMemcpyDeviceToHost, st);
      if (!slotted) hipMemcpyAsync(pin + resBytes, dOff, offBytes, hipMemcpyDeviceToHost, st);
      if (!ctx.sync()) return kFailed;
      if (ctx.profOn()) ctx.profCollect();
      const FastEncodeResult* res = reinterpret_cast<const FastEncodeResult*>(pin);
      const u64* off = reinterpret_cast<const u64*>(pin + resBytes);
      redoOut.clear();
      bool anyStuck = false;
      for (int i = 0; i < n; i++)
      {
        if (res[i].redo || res[i].stuck)
        {
          anyStuck = anyStuck || res[i].stuck != 0;
          if (!slotted && (res[i].redoReason & 128u)) return kBufferTooSmall;    // the arena is full
          redoOut.push_back(std::make_pair(t0 + i, res[i].stuck ? 0u : res[i].redoReason));    // (slotted: a tile that does not fit its slot says so when it is encoded by itself)
          continue;
        }
        rq.hOffsets[t0 + i] = slotted ? (u64)(t0 + i) * slotBytes : off[i];
        rq.hSizes[t0 + i] = res[i].blobSize;
        ctx.pathCount[0]++; ctx.tileBatchCount[0]++;
      }
      if (anyStuck) ctx.wipePersistentState();
      if (direct) { u64 claimed; memcpy(&claimed, pin + (size_t)n * sizeof(FastEncodeResult), 8); end += claimed; }    // (incl. the room of tiles that were handed back: holes)
      else if (!slotted) end = off[n];
      return kOk;
    };
    // (a tile that compresses to more than half its raw size -- lossless noise, a small error bound -- does not fit the batch's
    // slots.  A few such tiles are encoded one by one behind the batch; a batch full of them is encoded once more with slots
    // that hold raw blocks, instead of tile after tile with a wait each)
    const u64 slotBig = slotted ? slotBytes : ((tileElems * tb + tileElems / 64 + 4096) + 15) & ~15ull;
    // (a tile is a blockIdx.y: at most 65535 of them per launch)
    const int maxBatch = (int)std::max<size_t>(1, std::min<size_t>(std::min<size_t>((size_t)rq.nTiles, 65535), ((size_t)2 << 30) / slotBytes));
    const int maxBig = (int)std::max<size_t>(1, std::min<size_t>(std::min<size_t>((size_t)rq.nTiles, 65535), ((size_t)2 << 30) / slotBig));
    std::vector<std::pair<int, u32> > back;
    for (int t0 = 0; t0 < rq.nTiles; t0 += maxBatch)
    {
      const int n = std::min(maxBatch, rq.nTiles - t0);
      const u64 end0 = end;
      const unsigned long long count0 = ctx.pathCount[0], batch0 = ctx.tileBatchCount[0];
      u32 rc = runBatch(t0, n, slotBytes, back);
      if (rc != kOk) return rc;
      size_t tooBig = 0;
      for (const auto& r : back) if (r.second == 64u) tooBig++;    // (kRedoCapacity and nothing else)
      if (!slotted && !direct && tooBig > (size_t)std::max(8, n / 32))
      {
        end = end0; ctx.pathCount[0] = count0; ctx.tileBatchCount[0] = batch0;
        for (int s0 = t0; s0 < t0 + n; s0 += maxBig)
        {
          rc = runBatch(s0, std::min(maxBig, t0 + n - s0), slotBig, back);
          if (rc != kOk) return rc;
          for (const auto& r : back) { rc = encodeOne(r.first); if (rc != kOk) return rc; }
        }
        continue;
      }
      for (const auto& r : back) { rc = encodeOne(r.first); if (rc != kOk) return rc; }    // (reuses the workspace: the batch is done with it)
    }
    arenaUsed = slotted ? (u64)rq.nTiles * slotBytes : end;
    return kOk;
  }

  // sub-batches keep the workspace bounded (block descriptors are 1/16 of the pixels)
  const size_t perTile = fastEncodeWorkspace(rq.nRows, rq.nCols, 1) - 65536;
  const int maxBatch = (int)std::max<size_t>(1, std::min<size_t>((size_t)rq.nTiles, ((size_t)256 << 20) / perTile));
  for (int t0 = 0; t0 < rq.nTiles; t0 += maxBatch)
  {
    const int n = std::min(maxBatch, rq.nTiles - t0);
    if (!ctx.reserve(fastEncodeWorkspace(rq.nRows, rq.nCols, (u32)n))) return kFailed;
    FastEncodeLaunch fl;
    if (!prepareFastEncode(ctx, rq.dt, rq.nRows, rq.nCols, rq.maxZErr, (u32)n, tileElems, true, fl)) return kFailed;
    end = (end + 15) & ~15ull;
    runFastEncode(ctx, fl, (const u8*)rq.dData + (size_t)t0 * tileElems * tb, rq.dArena, rq.arenaCapacity, end);
    const size_t resBytes = (size_t)n * sizeof(FastEncodeResult), offBytes = ((size_t)n + 1) * 8;
    u8* pin = (u8*)ctx.pinned(resBytes + offBytes);
    if (!pin) return kFailed;
    hipMemcpyAsync(pin, fl.fb.result, resBytes, hipMemcpyDeviceToHost, st);
    hipMemcpyAsync(pin + resBytes, fl.fb.tileOffset, offBytes, hipMemcpyDeviceToHost, st);
    if (!ctx.sync()) return kFailed;
    if (ctx.profOn()) ctx.profCollect();
    const FastEncodeResult* res = reinterpret_cast<const FastEncodeResult*>(pin);
    const u64* off = reinterpret_cast<const u64*>(pin + resBytes);
    redo.clear();
    for (int i = 0; i < n; i++)
    {
      if (res[i].redo || res[i].stuck)
      {
        if (res[i].redoReason & 128u) return kBufferTooSmall;    // the arena is full
        redo.push_back(t0 + i);
        continue;
      }
      rq.hOffsets[t0 + i] = off[i];
      rq.hSizes[t0 + i] = res[i].blobSize;
      ctx.pathCount[0]++; ctx.tileBatchCount[0]++;
    }
    end = off[n];
    for (int t : redo) { const u32 rc = encodeOne(t); if (rc != kOk) return rc; }    // (reuses the workspace: the batch is done with it)
  }
  arenaUsed = end;
  return kOk;
}

}    // namespace lerc
