// codec_encode.cpp -- lerc_encode() on device-resident pixels: the entry points and the streaming launches.
//
// A request the streaming kernels take is decided on the device; every other one, and every band they hand
// back, goes band by band through encodeBands() (codec_encode_band.cpp).
//   streamingEligible   may the streaming kernels take rasters of this shape blind?
//   FastEncodePlan      one launch sequence: workspaceBytes(), layout(), arm(), launch(), fetch()
//   FastHarvest         what became of a launch's rasters; the counters of the streaming encodes
//   TileBatchEncoder    a mosaic's worth of tiles in sub-batches, the tiles handed back one by one behind them
#include "codec.h"
#include "huffman.h"
#include "fpl.h"
#include "tile_fast.h"
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

namespace lerc {

// LERC_AMD_ENCODE_LAUNCHES=2 keeps the two-launch form (statistics, then scan + pack) for a single raster: a tuning / test knob
bool fastEncodeOneLaunch()
{
  static const bool one = []() { const char* e = getenv("LERC_AMD_ENCODE_LAUNCHES"); return !(e && e[0] == '2'); }();
  return one;
}

// May the streaming kernels take rasters of this shape blind?  The callers differ in three ways:
//   dOut        what has to lie on a 16-byte boundary besides the pixels: a request's output buffer (nullptr, a size query, does) or a batch's arena
//   nDepth, hasMask, plain   a request (each band of a stack alike) may ask for depth, a mask, noData values, an older codec (!plain); a tile is one plain band
//   tileStride  bytes from one raster to the next, 0: there is only one.  Rasters of whole blocks are read 16 bytes a lane and must lie 16 bytes apart; ragged
//               ones (257 x 257 elevation tiles) are read pixel by pixel where rows do not start on 16-byte boundaries, and are the one-launch encoder's alone
static bool streamingEligible(int dt, int nRows, int nCols, int nDepth, bool hasMask, bool plain, double maxZErr, const void* dData,
                              const void* dOut, u64 tileStride)
{
  const bool ragged = nRows % 8 != 0 || nCols % 8 != 0;
  return plain && maxZErr != 777 && ((uintptr_t)dOut & 15) == 0 && ((uintptr_t)dData & 15) == 0 && (ragged || tileStride % 16 == 0)
    && fastEncodeEligible(dt, nRows, nCols, nDepth, hasMask, maxZErr, fastEncodeOneLaunch());
}
static bool anyNoData(const EncodeRequest& rq)
{
  bool any = false;
  if (rq.hUsesNoData) for (int i = 0; i < rq.nBands; i++) any = any || rq.hUsesNoData[i] != 0;
  return any;
}
static bool encodeStreamingOk(const EncodeRequest& rq)
{
  return streamingEligible(rq.dt, rq.nRows, rq.nCols, rq.nDepth, rq.nMasks > 0, !anyNoData(rq) && rq.version == kCodecVersion, rq.maxZErr,
                           rq.dData, rq.dOut, 0);
}

// ---- the kernels' parameters
BandParams fastBandParams(int dt, int nRows, int nCols, double maxZErr)
{
  // integer types: Lerc2 rounds the bound down to a whole number, and a bound below 1 is lossless (0.5).  So the bound is > 0 here: a
  // float request with maxZErr == 0 never gets this far (fastEncodeEligible refuses it, the entry points refuse negative bounds), and
  // makeBandParams' scale -- 0 for a bound of 0 -- is 1 / (2 * maxZErr)
  const bool isFlt = dt >= DT_Float;
  BandParams bp = makeBandParams(dt, nRows, nCols, 1, kCodecVersion, 8, isFlt ? maxZErr : std::max(0.5, floor(maxZErr)), true);
  bp.intLossless = (!isFlt && bp.maxZErr == 0.5) ? 1 : 0;
  return bp;
}
u32 raiseCandidates(int dt, double maxZErr)
{
  static const double errCand[9] = { 1, 0.5, 0.1, 0.05, 0.01, 0.005, 0.001, 0.0005, 0.0001 };
  u32 cand = 0;
  if (dt >= DT_Float) for (int c = 0; c < 9; c++) if (errCand[c] / 2 > maxZErr) cand |= 1u << c;
  return cand;
}

// ---- one launch sequence of the streaming kernels over nTiles rasters of one shape (a single raster, a band of a stack: nTiles == 1)
struct FastEncodePlan
{
  // kOneLaunch     k_fast_encode1: statistics, block decisions, pack and checksum from one read (a tile per blockIdx.y)
  // kTwoLaunches   one raster: statistics, then a pack step whose first blocks scan and decide (LERC_AMD_ENCODE_LAUNCHES=2; every size query of whole blocks)
  // kThreeLaunches statistics, scan + decide (+ the tiles' places in the arena), pack: a tile batch under that knob; a raster beyond the others' 32-bit byte counts
  enum Form { kOneLaunch, kTwoLaunches, kThreeLaunches };
  // where the blobs go.  kOwnBuffer: one raster, into the buffer given to launch().  A batch: kSlots -- every tile has its place, t * slotBytes;
  // kCursor -- straight into the arena, a tile's last workgroup claims the tile's room with an atomic add on the batch's cursor (tile_fast.h:
  // FastFused::arenaCursor), the tiles lie in the order of their claims; kCopy -- into slots of the workspace, then placed and moved
  // (k_fast_tile_copy); kPlaced -- the three-launch form: its second step places the tiles, its third packs them there
  enum Arena { kOwnBuffer, kSlots, kCursor, kCopy, kPlaced };
  Form form;
  Arena arena;
  int dt, nRows, nCols;
  u32 nTiles, nWG, nCell;    // nWG: workgroups of 64 blocks a raster; nCell: workgroups a raster whose cells the persistent areas hold
  u64 tileElems, slotBytes, arenaCapacity = 0;
  u8* dArena = nullptr;
  FastEncodeBuffers fb;
  FastBatch batch;
  BandParams bp;
  u32 cand; double maxZErr;
  u8* slots = nullptr;       // kCopy: the slots
  u64* dOff = nullptr;       // a batch: [nTiles + 1] where the tiles lie in the arena
  const FastEncodeResult* res = nullptr; const u64* off = nullptr;    // (after fetch(), in pinned memory)
  u64 claimed = 0;           // kCursor: bytes the batch has claimed (incl. the room of tiles that were handed back: holes)
  FastEncodePlan(int dt_, int nRows_, int nCols_, double maxZErr_, u32 nTiles_ = 1, Arena arena_ = kOwnBuffer, u64 slotBytes_ = 0)
    : arena(arena_), dt(dt_), nRows(nRows_), nCols(nCols_), nTiles(nTiles_), nWG(fastEncodeNumWG(nRows_, nCols_)),
      tileElems(arena_ == kOwnBuffer ? 0 : (u64)nRows_ * (u64)nCols_), slotBytes(slotBytes_), bp(fastBandParams(dt_, nRows_, nCols_, maxZErr_)),
      cand(raiseCandidates(dt_, maxZErr_)), maxZErr(maxZErr_)
  {
    const bool one = fastEncodeOneLaunch();
    if (arena == kOwnBuffer) form = !fastSoloOk(dt, nRows, nCols) ? kThreeLaunches : one ? kOneLaunch : kTwoLaunches;
    else form = arena == kPlaced ? kThreeLaunches : kOneLaunch;
    const u32 nWGf = fastFusedNumWG(dt, nRows, nCols);    // (the one-launch form counts its own workgroups)
    nCell = oneRaster() ? (one ? std::max(nWG, nWGf) : nWG) : nWGf;    // (one raster keeps cells for both of its forms)
    memset(&fb, 0, sizeof(fb));
    if (form == kOneLaunch) fb.fused.nWG = nWGf;
    batch.nTiles = nTiles; batch.nWG = (form == kOneLaunch && !oneRaster()) ? nWGf : nWG; batch.tileElems = tileElems; batch.nBlobsMore = 0;
  }
  bool oneRaster() const { return arena == kOwnBuffer && form != kThreeLaunches; }
  // the staged forms' buffers for n rasters (one raster's one launch keeps them too, for its size queries)
  static size_t stagedBytes(int nRows, int nCols, u32 n)
  {
    const size_t nWG = fastEncodeNumWG(nRows, nCols);
    return (size_t)n * (nWG * (kFastBlocksPerWG * sizeof(FastBlockDesc) + 64) + kFastPrefixStage + sizeof(FastEncodeResult)
                        + (fastScanGroups((u32)nWG) + 1) * (4 + 8 * kScanPartWords) + fastPackGroups((u32)nWG) * 16 + fastTicketStride((u32)nWG) * 4 + 256)
      + 65536;
  }
  size_t workspaceBytes() const
  {
    // (a batch in one launch: the results, the cursor and the offsets -- and the slots where the blobs are moved afterwards)
    if (form == kOneLaunch && !oneRaster()) return (size_t)nTiles * ((arena == kCopy ? slotBytes : 0) + sizeof(FastEncodeResult) + 8) + (1u << 16);
    return stagedBytes(nRows, nCols, nTiles);
  }
  // carves the plan's buffers out of the context's two persistent areas ([0] counters the kernels leave zero, [1] epoch-tagged cells)
  // and the bump workspace (reserve() first): every per-raster array holds nTiles consecutive sets
  bool layout(Context& ctx)
  {
    const size_t nT = nTiles;
    const bool raster = oneRaster(), three = form == kThreeLaunches;
    const u32 nGrp = fastFusedGroups(nCell), nPack = fastPackGroups(nCell);
    const size_t cellWords = fastFusedCellWords(nCell), counterWords = fastFusedCounterWords(nCell);
    u64 *cells = nullptr, *counters = nullptr;
    if (!three)
    {
      // (cells: per workgroup, then the one-launch form's group cells and first-row errors -- kCursor: and a cell a tile behind all sets; counters: pack accumulators, key cells)
      cells = (u64*)ctx.persistentState(1, nT * (cellWords + (arena == kCursor ? 1 : 0)) * 8 + 256);
      counters = (u64*)ctx.persistentState(0, nT * counterWords * 8 + 256);
      if (!cells || !counters) return false;
    }
    if (raster || three)
    {
      // (one raster: the pack step's first blocks scan and decide, tile_fast.h -- no scan buffers, the accumulators and cells persistent)
      fb.desc = ctx.allocT<FastBlockDesc>(nT * nWG * kFastBlocksPerWG);
      fb.wgSize = ctx.allocT<u32>(nT * fastWgStride(nWG) + 4);
      if (three) fb.wgBase = ctx.allocT<u32>(nT * fastWgStride(nWG) + 4);
      fb.wgMinKey = ctx.allocT<u64>(nT * nWG + 4);
      fb.wgMaxKey = ctx.allocT<u64>(nT * nWG + 4);
      fb.wgFlags = ctx.allocT<u32>(nT * nWG + 4);
      if (three) fb.groupBase = ctx.allocT<u32>(nT * (fastScanGroups(nWG) + 1) + 4);
      if (three) fb.scanPart = ctx.allocT<u64>(kScanPartWords * nT * fastScanGroups(nWG) + 4);
      if (three) fb.packPart = ctx.allocT<u64>(nT * fastPackGroups(nWG) + 4);
      fb.tickets = ctx.allocT<u32>(nT * fastTicketStride(nWG) + 4);
      fb.result = ctx.allocT<FastEncodeResult>(nT);
      fb.prefixStage = ctx.allocT<u8>(nT * kFastPrefixStage);
      if (arena == kPlaced) dOff = fb.tileOffset = ctx.allocT<u64>(nT + 1);
      if (!fb.desc || !fb.wgSize || !fb.wgMinKey || !fb.wgMaxKey || !fb.wgFlags || !fb.tickets || !fb.result || !fb.prefixStage
        || (three && (!fb.wgBase || !fb.groupBase || !fb.scanPart || !fb.packPart)) || (arena == kPlaced && !dOff))
        return false;
      if (raster) { fb.packPart = counters; fb.solo.cells = cells; }
    }
    else
    {
      if (arena == kCopy) slots = ctx.allocT<u8>(nT * slotBytes);
      // (the results and, behind them, the batch's cursor: cleared by one memset)
      static_assert(sizeof(FastEncodeResult) % 8 == 0, "the cursor behind the results is 8-byte aligned");
      fb.result = (FastEncodeResult*)ctx.alloc(nT * sizeof(FastEncodeResult) + 16);
      dOff = ctx.allocT<u64>(nT + 1);
      if ((arena == kCopy && !slots) || !fb.result || !dOff) return false;
    }
    if (form != kOneLaunch) return true;
    FastFused& f = fb.fused;
    f.sizeCell = cells; f.baseCell = f.sizeCell + nCell; f.totalCell = f.baseCell + nGrp; f.raise = f.totalCell + nGrp;
    f.packPart = counters; f.keyPart = f.packPart + nPack + 1;
    if (raster) return true;
    f.nTiles = nTiles; f.cellStride = (u32)cellWords; f.counterStride = (u32)counterWords;
    f.tileElems = tileElems; f.outStride = arena == kCursor ? 0 : slotBytes;
    if (arena != kCursor) return true;
    f.arenaCursor = reinterpret_cast<u64*>(reinterpret_cast<u8*>(fb.result) + nT * sizeof(FastEncodeResult));
    f.tileCell = cells + nT * cellWords;    // (epoch-tagged, behind the tiles' own cells)
    f.tileOffset = dOff;
    f.arenaCapacity = arenaCapacity;
    return true;
  }
  // a launch's tag (never 0, the tag of a cell nobody has written yet), and how long its workgroups wait for each other
  void arm(Context& ctx, Form now)
  {
    const u32 epoch = ctx.nextEpoch();
    if (now == kTwoLaunches) { fb.solo.epoch = epoch; return; }
    const bool giveUp = (fastTestGiveUp() & 1u) != 0;    // (the test knob: nobody ever sees a cell arrive, every waiter gives up after a few polls)
    fb.fused.epoch = epoch;
    fb.fused.publishEpoch = giveUp ? epoch ^ 0x5A5A5A5Au : epoch;
    fb.fused.spinLimit = giveUp ? 8u : (1u << 22);
#ifdef HIPSIM
    // (the emulator runs workgroups one after the other: one that waits for one BEHIND it gives up after a few polls -- the hand-back path's test)
    if (arena == kCursor) fb.fused.spinLimit = 64u;
#endif
  }
  // one kernel per stage (and per profiling group): statistics (+ first-row rounding errors), scan + decide (+ tile placement for
  // batches), pack + checksum -- or all of it in one.  arenaBase: where a batch's first byte goes
  void launch(Context& ctx, const void* dData, u8* out, u64 capacity, u64 arenaBase = 0)
  {
    static const char* kStage[3] = { "fast_stats_sizes", "fast_scan_decide", "fast_pack" };
    hipStream_t st = ctx.activeStream();
    // (one raster, no output buffer: one launch only where the two-launch form cannot go)
    const Form now = (form == kOneLaunch && oneRaster() && !out && nRows % 8 == 0 && nCols % 8 == 0) ? kTwoLaunches : form;
    if (now != kThreeLaunches) arm(ctx, now);
    if (now == kOneLaunch)
    {
      if (arena == kCursor) fb.fused.arenaBase = arenaBase;
      if (!oneRaster()) hipMemsetAsync(fb.result, 0, (size_t)nTiles * sizeof(FastEncodeResult) + 16, st);    // (the kernels raise `stuck`, nobody else clears it; the cursor)
      {
        ProfScope ps(ctx, "fast_encode1");
        launchFastEncode(0, bp, maxZErr, cand, dData, out, capacity, 0, fb, batch, st);
      }
      if (arena != kCopy) return;
      ProfScope ps(ctx, "fast_tile_move");
      launchFastTileCopy(fb.result, dOff, slots, slotBytes, slotBytes, dArena, nTiles, arenaBase, arenaCapacity, st);
      return;
    }
    for (int stage = 0; stage < 3; stage++)
    {
      if (stage == 1 && now == kTwoLaunches) continue;      // (one raster: the pack step scans and decides itself)
      if (stage == 2 && now == kThreeLaunches && !out) continue;    // (no output buffer: the size is known after the decisions)
      ProfScope ps(ctx, kStage[stage]);
      launchFastEncode(stage, bp, maxZErr, cand, dData, out, capacity, arenaBase, fb, batch, st);
    }
  }
  // a batch's results (+ the cursor) and offsets on their way into pinned memory; waits for the stream
  bool fetch(Context& ctx)
  {
    hipStream_t st = ctx.activeStream();
    const size_t resBytes = (size_t)nTiles * sizeof(FastEncodeResult) + (form == kOneLaunch ? 16 : 0), offBytes = ((size_t)nTiles + 1) * 8;
    u8* pin = (u8*)ctx.pinned(resBytes + offBytes);
    if (!pin) return false;
    hipMemcpyAsync(pin, fb.result, resBytes, hipMemcpyDeviceToHost, st);
    if (arena != kSlots) hipMemcpyAsync(pin + resBytes, dOff, offBytes, hipMemcpyDeviceToHost, st);
    if (!ctx.sync()) return false;
    if (ctx.profOn()) ctx.profCollect();
    res = reinterpret_cast<const FastEncodeResult*>(pin);
    off = reinterpret_cast<const u64*>(pin + resBytes);
    if (arena == kCursor) memcpy(&claimed, pin + (size_t)nTiles * sizeof(FastEncodeResult), 8);
    return true;
  }
};

// ---- what became of the rasters of a launch, read from their results once the stream has passed them.  The only place that counts
// streaming encodes: pathCount[0] (calls; every tile of a batch is one) and tileBatchCount[0]
struct FastHarvest
{
  enum Count { kCountNothing, kCountCalls, kCountTiles };
  std::vector<std::pair<int, u32> > back;    // the rasters handed back: index, reason bits (FastRedo) -- 0 where a workgroup gave up waiting
  unsigned long long nDone = 0;
  Count counted = kCountNothing;
  bool arenaFull = false;                    // a tile says that the batch's ARENA is full: the call is over, nothing behind that tile was read
  // sign -1: the batch is run again, what it has counted is taken back
  static void credit(Context& ctx, Count what, unsigned long long n, int sign = 1)
  {
    if (what != kCountNothing) ctx.pathCount[0] += sign > 0 ? n : 0ull - n;
    if (what == kCountTiles) ctx.tileBatchCount[0] += sign > 0 ? n : 0ull - n;
  }
  // res[i] is raster first + i; a raster that is done leaves its size in hSizes and its offset -- off[i], or its slot's -- in hOffsets
  // (where given).  arena: the blobs share an arena that can be full
  void read(Context& ctx, const FastEncodeResult* res, int n, Count what, bool arena = false, int first = 0, u64* hOffsets = nullptr,
            u32* hSizes = nullptr, const u64* off = nullptr, u64 slotBytes = 0)
  {
    back.clear();
    counted = what; arenaFull = false;
    unsigned long long done = 0;
    bool stuck = false;
    for (int i = 0; i < n && !arenaFull; i++)
    {
      const FastEncodeResult& r = res[i];
      if (r.redo || r.stuck)
      {
        stuck = stuck || r.stuck != 0;
        if (arena && (r.redoReason & kRedoArena)) arenaFull = true;
        else back.push_back(std::make_pair(first + i, r.stuck ? 0u : r.redoReason));    // (a tile that does not fit its SLOT says so when it is encoded by itself)
        continue;
      }
      if (hOffsets) hOffsets[first + i] = off ? off[i] : (u64)(first + i) * slotBytes;
      if (hSizes) hSizes[first + i] = r.blobSize;
      done++;
    }
    credit(ctx, what, nDone = done);
    if (stuck && !arenaFull) ctx.wipePersistentState();    // (late workgroups may have left residue in the counters)
  }
};

// a result the kernels write straight into pinned memory, as it is before they do: if a launch fails, what the operation that had the
// memory before left there must not read as this one's verdict -- "redo" sends the request to the general path, which reports what is wrong
static void presetResult(void* slot)
{
  FastEncodeResult init;
  memset(&init, 0, sizeof(init));
  init.redo = 1u; init.redoReason = kRedoNotLaunched;
  memcpy(slot, &init, sizeof(init));
}

bool encodeEnqueueStreaming(Context& ctx, const EncodeRequest& rq, u8* slot)
{
  if (!slot || rq.nBands != 1 || !encodeStreamingOk(rq)) return false;
  ctx.reset();
  FastEncodePlan plan(rq.dt, rq.nRows, rq.nCols, rq.maxZErr);
  if (!ctx.reserve(plan.workspaceBytes() + (1u << 16)) || !plan.layout(ctx)) return false;
  // (one raster: the deciding block and the last workgroup write the result straight into `slot`, pinned host memory -- no
  // kernel reads it, and a copy kernel behind the encode would cost every call 4 us)
  const bool direct = plan.oneRaster();
  if (direct) { presetResult(slot); plan.fb.result = reinterpret_cast<FastEncodeResult*>(slot); }
  (void)hipGetLastError();
  plan.launch(ctx, rq.dData, rq.dOut, rq.dOut ? (u64)rq.outCapacity : ~0ull);
  if (hipGetLastError() != hipSuccess) { ctx.lastError = "lerc_amd: a streaming encode kernel could not be launched"; return false; }
  return direct || hipMemcpyAsync(slot, plan.fb.result, sizeof(FastEncodeResult), hipMemcpyDeviceToHost, ctx.activeStream()) == hipSuccess;
}

void encodeStreamingVerdict(Context& ctx, const EncodeRequest& rq, const u8* slot, bool& redo, u32& status, u32& numBytesNeeded, u32& numBytesWritten)
{
  FastEncodeResult hres;
  memcpy(&hres, slot, sizeof(hres));
  if (ctx.profOn()) ctx.profCollect();
  redo = false; status = kOk;
  FastHarvest got;
  got.read(ctx, &hres, 1, FastHarvest::kCountCalls);
  if (got.back.empty())
  {
    numBytesNeeded = hres.blobSize;
    numBytesWritten = rq.dOut ? hres.blobSize : 0;
    return;
  }
  char msg[160];
  snprintf(msg, sizeof(msg), "streaming encode handed the band to the general kernels (redo %u, reason bits 0x%x, stuck %u, blob %u bytes)",
           hres.redo, hres.redoReason, hres.stuck, hres.blobSize);
  ctx.lastNote = msg;
  if (rq.dOut && hres.redoReason == kRedoCapacity && hres.blobSize > rq.outCapacity) { status = kBufferTooSmall; return; }
  redo = true;
}

// several bands: each is a blob of its own with "bands to follow" in its header (Lerc.cpp:628-789); a band is packed into 16-byte
// aligned scratch (its place in the output is wherever the band before it ended) and copied over.  redo: a band was handed back, the
// general path takes the whole request
static u32 encodeBandStack(Context& ctx, const EncodeRequest& rq, size_t bandCap, bool& redo, u32& numBytesNeeded, u32& numBytesWritten)
{
  hipStream_t st = ctx.activeStream();
  const size_t bandBytes = (size_t)rq.nRows * rq.nCols * dtSize(rq.dt);
  FastEncodePlan plan(rq.dt, rq.nRows, rq.nCols, rq.maxZErr);
  if (!plan.layout(ctx)) return kFailed;
  u8* dBandBlob = rq.dOut ? ctx.allocT<u8>(bandCap) : nullptr;
  FastEncodeResult* pinRes = (FastEncodeResult*)ctx.pinned(sizeof(FastEncodeResult));
  if (!pinRes || (rq.dOut && !dBandBlob)) return kFailed;
  const bool direct = plan.oneRaster();    // (the kernels write the result into pinned memory themselves)
  FastHarvest got;
  u64 total = 0;
  redo = false;
  for (int iBand = 0; iBand < rq.nBands; iBand++)
  {
    plan.batch.nBlobsMore = (u32)(rq.nBands - 1 - iBand);
    if (direct) { presetResult(pinRes); plan.fb.result = pinRes; }
    plan.launch(ctx, (const u8*)rq.dData + (size_t)iBand * bandBytes, dBandBlob, dBandBlob ? (u64)bandCap : ~0ull);
    if (!direct) hipMemcpyAsync(pinRes, plan.fb.result, sizeof(FastEncodeResult), hipMemcpyDeviceToHost, st);
    if (!ctx.sync()) return kFailed;
    got.read(ctx, pinRes, 1, FastHarvest::kCountNothing);
    if (!got.back.empty()) { redo = true; break; }
    const u32 blobBytes = pinRes->blobSize;
    if (total + blobBytes > (u64)UINT_MAX) return kDimsTooLarge;
    if (rq.dOut)
    {
      if (total + blobBytes > rq.outCapacity) return kBufferTooSmall;
      hipMemcpyAsync(rq.dOut + total, dBandBlob, blobBytes, hipMemcpyDeviceToDevice, st);
    }
    total += blobBytes;
  }
  if (ctx.profOn()) ctx.profCollect();
  if (redo) return kOk;
  if (rq.dOut && !ctx.sync()) return kFailed;
  FastHarvest::credit(ctx, FastHarvest::kCountCalls, 1);    // (a call counts once)
  numBytesNeeded = (u32)total;
  numBytesWritten = rq.dOut ? (u32)total : 0;
  return kOk;
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
  const bool noData = anyNoData(rq);
  if (noData && !rq.hNoDataValues) return kWrongParam;
  if (noData) need += (size_t)nPix * rq.nDepth * tb + (size_t)nPix + 8192;
  if (rq.nMasks > 0 || rq.dt >= DT_Float) need += maskRleScratchBytes(maskBytes) + (4u << 20) + 8192;    // a large mask is run-length coded on the device
  if (rq.dt >= DT_Float && (rq.maxZErr == 0 || noData) && rq.version >= 6) need += fplEncodeScratchBytes(nPix * rq.nDepth, tb);
  if (rq.version < 2 || rq.version > kCodecVersion) return kWrongParam;
  if (rq.version < 6 && noData) return kWrongParam;    // Lerc.cpp:341-344
  if (rq.version < 4 && rq.nDepth > 1) return kFailed;    // Lerc2::Set refuses (Lerc2.cpp:85-86)
  // (a size query, dOut == nullptr, takes the streaming path too: its statistics and decisions)
  const bool fastOk = encodeStreamingOk(rq);
  need += fastOk ? FastEncodePlan::stagedBytes(rq.nRows, rq.nCols, 1) : 0;
  const size_t bandCap = (size_t)nPix * tb + 4096;    // a band's blob never exceeds its raw form by more than the small sections
  if (fastOk && rq.nBands > 1 && rq.dOut) need += bandCap + 256;
  if (!ctx.reserve(need)) return kFailed;

  // ---- streaming path: everything is decided on the device, one synchronisation at the end.  If an assumption fails (NaN, all-integer floats,
  // raisable error bound, constant image, 16 x 16 retry, raw fallback) the device says so and the general path below redoes the band.
  if (fastOk)
  {
    bool redo = false;
    u32 status = kOk;
    if (rq.nBands > 1) status = encodeBandStack(ctx, rq, bandCap, redo, numBytesNeeded, numBytesWritten);
    else
    {
      FastEncodeResult* pinRes = (FastEncodeResult*)ctx.pinned(sizeof(FastEncodeResult));
      if (!pinRes || !encodeEnqueueStreaming(ctx, rq, reinterpret_cast<u8*>(pinRes)) || !ctx.sync()) return kFailed;
      encodeStreamingVerdict(ctx, rq, reinterpret_cast<const u8*>(pinRes), redo, status, numBytesNeeded, numBytesWritten);
    }
    if (!redo) return status;
    ctx.reset();
  }
  return encodeBands(ctx, rq, numBytesNeeded, numBytesWritten);
}

// ---- a mosaic's worth of independent tiles in one call: every tile becomes its own blob (own header, ranges, checksum), byte for byte
// what encodeDevice() makes of it; the blobs go into one arena at 16-byte aligned offsets.  Tiles the streaming kernels hand back
// (constant tiles, NaNs, ...) are encoded one by one behind their sub-batch.
struct TileBatchEncoder
{
  Context& ctx; const TilesEncodeRequest& rq;
  const int tb; const u64 tileElems;
  const bool slotted;      // every tile has its place: no arena to fill front to back
  bool direct;             // the one-launch encoder's blobs go straight into the arena (FastEncodePlan::kCursor): no slots, no pass that moves them
  // the one-launch encoder's slots, a tile each: half the tile's raw size -- a tile that needs more is encoded by itself afterwards -- and,
  // for a batch full of such tiles, slots that hold raw blocks
  u64 slotBytes, slotBig;
  u64 end = 0;             // arena bytes in use
  static constexpr int kFewTooBig = 8;    // so many tiles (or a 32nd of the batch, if that is more) that outgrow their slots are encoded one by one

  TileBatchEncoder(Context& c, const TilesEncodeRequest& r)
    : ctx(c), rq(r), tb(dtSize(r.dt)), tileElems((u64)r.nRows * (u64)r.nCols), slotted(r.slotBytes != 0)
  {
    // LERC_AMD_TILE_ARENA=copy keeps the slots + k_fast_tile_copy form (a knob for A/B runs and tests).  Emulator builds keep it unless
    // asked: they run workgroups one after the other, and a tile's workgroups wait for its LAST one's claim (FastEncodePlan::arm)
#ifdef HIPSIM
    static const bool cursorMode = []() { const char* e = getenv("LERC_AMD_TILE_ARENA"); return e && strcmp(e, "cursor") == 0; }();
#else
    static const bool cursorMode = []() { const char* e = getenv("LERC_AMD_TILE_ARENA"); return !(e && strcmp(e, "copy") == 0); }();
#endif
    direct = !slotted && cursorMode;
    slotBytes = slotted ? rq.slotBytes : ((tileElems * tb / 2 + 4096) + 15) & ~15ull;
    slotBig = slotted ? rq.slotBytes : ((tileElems * tb + tileElems / 64 + 4096) + 15) & ~15ull;
  }
  FastEncodePlan::Arena arena() const
  {
    return !fastEncodeOneLaunch() ? FastEncodePlan::kPlaced : slotted ? FastEncodePlan::kSlots : direct ? FastEncodePlan::kCursor : FastEncodePlan::kCopy;
  }
  // tile t by itself, behind what the arena holds (or into its slot)
  u32 encodeOne(int t)
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
  }
  // one launch sequence for tiles [t0, t0 + n), the one-launch encoder's blobs in slots of `slot` bytes; then the tiles it hands back, one
  // by one (they reuse the workspace: the batch is done with it) -- unless the batch is to be run once more, with larger slots
  u32 runBatch(int t0, int n, u64 slot, bool& onceMore)
  {
    FastEncodePlan plan(rq.dt, rq.nRows, rq.nCols, rq.maxZErr, (u32)n, arena(), slot);
    plan.dArena = rq.dArena; plan.arenaCapacity = rq.arenaCapacity;
    if (!ctx.reserve(plan.workspaceBytes()) || !plan.layout(ctx)) return kFailed;
    const u64 end0 = end = (end + 15) & ~15ull;
    u8* out = slotted ? rq.dArena + (size_t)t0 * slot : plan.arena == FastEncodePlan::kCopy ? plan.slots : rq.dArena;
    (void)hipGetLastError();
    plan.launch(ctx, (const u8*)rq.dData + (size_t)t0 * tileElems * tb, out, (slotted || plan.arena == FastEncodePlan::kCopy) ? slot : rq.arenaCapacity, end);
    if (hipGetLastError() != hipSuccess) { ctx.lastError = "lerc_amd: a streaming encode kernel could not be launched"; return kFailed; }
    if (!plan.fetch(ctx)) return kFailed;
    FastHarvest got;
    got.read(ctx, plan.res, n, FastHarvest::kCountTiles, !slotted, t0, rq.hOffsets, rq.hSizes, slotted ? nullptr : plan.off, slot);
    if (got.arenaFull) return kBufferTooSmall;
    if (plan.arena == FastEncodePlan::kCursor) end += plan.claimed;
    else if (!slotted) end = plan.off[n];
    // A tile that compresses to more than half its raw size -- lossless noise, a small error bound -- does not fit the batch's first slots.
    // A few such tiles are encoded one by one behind the batch; a batch full of them is encoded once more with slots that hold raw blocks,
    // instead of tile after tile with a wait each.  (Only where the blobs are moved out of their slots: a caller's slots are what they
    // are, and the cursor form and the three-launch form have none.)
    size_t tooBig = 0;
    for (const auto& r : got.back) if (r.second == kRedoCapacity) tooBig++;    // (and nothing else)
    onceMore = plan.arena == FastEncodePlan::kCopy && slot != slotBig && tooBig > (size_t)std::max(kFewTooBig, n / 32);
    if (onceMore) { FastHarvest::credit(ctx, got.counted, got.nDone, -1); end = end0; return kOk; }
    for (const auto& r : got.back) { const u32 rc = encodeOne(r.first); if (rc != kOk) return rc; }
    return kOk;
  }
  u32 run(bool fastOk, u64& arenaUsed)
  {
    if (slotted && rq.arenaCapacity < (u64)rq.nTiles * rq.slotBytes) return kBufferTooSmall;
    const bool placed = arena() == FastEncodePlan::kPlaced;
    if (!fastOk || (slotted && placed))    // (tile by tile: what the streaming kernels do not take, and -- the three-launch form has no slots -- a slotted batch under its knob)
    {
      for (int t = 0; t < rq.nTiles; t++) { const u32 rc = encodeOne(t); if (rc != kOk) return rc; }
      arenaUsed = slotted ? (u64)rq.nTiles * rq.slotBytes : end;
      return kOk;
    }
    // sub-batches: a tile is a blockIdx.y, at most 65535 of them per launch, and the slots stay below 2 GB; the three-launch form keeps its
    // workspace bounded (block descriptors are 1/16 of the pixels)
    const size_t nT = (size_t)rq.nTiles, perTile = FastEncodePlan::stagedBytes(rq.nRows, rq.nCols, 1) - 65536;
    const int maxBatch = (int)std::max<size_t>(1, placed ? std::min<size_t>(nT, ((size_t)256 << 20) / perTile)
                                                         : std::min<size_t>(std::min<size_t>(nT, 65535), ((size_t)2 << 30) / slotBytes));
    const int maxBig = (int)std::max<size_t>(1, std::min<size_t>(std::min<size_t>(nT, 65535), ((size_t)2 << 30) / slotBig));
    for (int t0 = 0; t0 < rq.nTiles; t0 += maxBatch)
    {
      const int n = std::min(maxBatch, rq.nTiles - t0);
      bool onceMore = false;
      u32 rc = runBatch(t0, n, placed ? 0 : slotBytes, onceMore);
      for (int s0 = t0; onceMore && s0 < t0 + n && rc == kOk; s0 += maxBig) { bool again = false; rc = runBatch(s0, std::min(maxBig, t0 + n - s0), slotBig, again); }
      if (rc != kOk) return rc;
    }
    arenaUsed = slotted ? (u64)rq.nTiles * rq.slotBytes : end;
    return kOk;
  }
};

u32 encodeTilesDevice(Context& ctx, const TilesEncodeRequest& rq, u64& arenaUsed)
{
  arenaUsed = 0;
  if (!rq.dData || !rq.dArena || !rq.hOffsets || !rq.hSizes || rq.nTiles <= 0 || rq.nRows <= 0 || rq.nCols <= 0 || rq.dt < 0 || rq.dt > DT_Double
    || rq.maxZErr < 0 || (rq.slotBytes & 15u) != 0)
    return kWrongParam;
  if (tilesBytesEncodeEligible(rq)) return encodeTilesBytes(ctx, rq, arenaUsed);    // (8-bit: the Huffman decision, a tile per workgroup)
  TileBatchEncoder enc(ctx, rq);
  return enc.run(streamingEligible(rq.dt, rq.nRows, rq.nCols, 1, false, true, rq.maxZErr, rq.dData, rq.dArena, enc.tileElems * enc.tb), arenaUsed);
}

}    // namespace lerc
