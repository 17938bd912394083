// codec_decode_band.cpp -- the general band path of lerc_decode(): a call's bands, stage by stage, into device-resident pixels.
//
// Host logic mirrors Lerc::DecodeTempl (Lerc.cpp:397-521) and Lerc2::Decode (Lerc2.cpp:577-694):
// header + mask + ranges + mode bytes are parsed on the host (tens of bytes; the mask RLE is the
// only sequential piece), everything that touches pixels or the block stream is a HIP kernel.
#include "codec.h"
#include "huffman.h"
#include "fpl.h"
#include "tile_fast.h"

#include <algorithm>
#include <cstdint>
#include <cstdio>

namespace lerc {

bool BlobReader::read(u64 off, size_t len, u8* dst) const
{
  if (off + len > n) return false;
  if (h) { memcpy(dst, h + off, len); return true; }
  if (cache && off >= cacheOff && off + len <= cacheOff + cacheLen) { memcpy(dst, cache + (off - cacheOff), len); return true; }
  u8* pin = ctx ? (u8*)ctx->pinned(len < 4096 ? 4096 : len) : nullptr;    // (a pageable target is staged at ~1 GB/s)
  if (hipMemcpyAsync(pin ? pin : dst, d + off, len, hipMemcpyDeviceToHost, st) != hipSuccess) return false;
  if (!(ctx ? ctx->sync() : hipStreamSynchronize(st) == hipSuccess)) return false;
  if (pin) memcpy(dst, pin, len);
  return true;
}

static bool readBandHeader(const BlobReader& rd, u64 off, BandDesc& b)
{
  u8* buf = b.head;
  const size_t want = std::min<size_t>(sizeof(b.head), rd.n - off);
  b.headLen = want;
  if (off >= rd.n || !rd.read(off, want, buf)) return false;
  if (!readHeader(buf, want, b.hd, b.hdrLen)) return false;
  if (want < b.hdrLen + 4) return false;
  memcpy(&b.numBytesMask, buf + b.hdrLen, 4);
  if (b.numBytesMask < 0) return false;
  b.offset = off;
  return true;
}

u32 walkBands(const BlobReader& rd, u32 blobSize, std::vector<BandDesc>& bands)
{
  bands.clear();
  BandDesc b;
  if (!readBandHeader(rd, 0, b)) return kFailed;
  bands.push_back(b);
  u64 total = (u64)b.hd.blobSize;
  if (total > blobSize) return kFailed;
  bool more = (b.hd.version <= 5) || (b.hd.nBlobsMore > 0);
  BandDesc nb;
  while (more && total < blobSize && readBandHeader(rd, total, nb))
  {
    if (nb.hd.nDepth != b.hd.nDepth || nb.hd.nCols != b.hd.nCols || nb.hd.nRows != b.hd.nRows || nb.hd.dt != b.hd.dt) return kFailed;
    if (total + (u64)nb.hd.blobSize > blobSize) return kFailed;
    more = (nb.hd.version <= 5) || (nb.hd.nBlobsMore > 0);
    bands.push_back(nb);
    total += (u64)nb.hd.blobSize;
  }
  return kOk;
}

int bandsMaskCount(const std::vector<BandDesc>& bands)
{
  int nMasks = 0;
  for (size_t i = 0; i < bands.size(); i++)
  {
    const BandDesc& b = bands[i];
    if (i == 0) { if (b.numBytesMask > 0 || b.hd.numValid == 0) nMasks = 1; }
    else if (b.numBytesMask > 0 || b.hd.numValid != bands[0].hd.numValid) nMasks = 2;
  }
  return nMasks > 1 ? (int)bands.size() : nMasks;
}

namespace {

bool scanOffsetsOn()    // (LERC_AMD_SCAN_OFFSETS=0: masked bands keep to the general discovery)
{
  static const bool on = []() { const char* e = getenv("LERC_AMD_SCAN_OFFSETS"); return !e || atoi(e) != 0; }();
  return on;
}

const size_t kDeviceRleMax = (size_t)4 << 20;    // masks decoded on the device: 16 bytes of tables per byte of the stream
bool maskOnDevice(size_t maskBytes, int numBytesMask) { return maskBytes >= deviceRleFrom() && numBytesMask >= 2 && (size_t)numBytesMask <= kDeviceRleMax; }

// what a call's bands take from the workspace (the tables are sized for ONE band: every band starts where the first one did)
size_t workspaceBytes(const DecodeRequest& rq, const std::vector<BandDesc>& bands)
{
  const int dt = rq.dt, nD = rq.nDepth, nCols = rq.nCols, nRows = rq.nRows, tb = dtSize(rq.dt);
  const i64 nPix = (i64)nRows * nCols;
  const size_t maskBytes = (size_t)((nPix + 7) >> 3);
  size_t need = (rq.dBlob ? 0 : (size_t)rq.blobSize + 256) + 2 * (maskBytes + 64) + (1u << 16)
    + (size_t)nD * 8 + 4 * ((size_t)(nPix >> 5) + 1024) * 4;
  // block offsets: one per sub-block for the smallest legal block size we may meet (decided per band)
  size_t maxSub = 0, maxChunks = 0;
  for (int i = 0; i < rq.nBands; i++)
  {
    const Header& h = bands[i].hd;
    const size_t sub = (size_t)((nRows + h.mbSize - 1) / h.mbSize) * ((nCols + h.mbSize - 1) / h.mbSize) * nD;
    maxSub = std::max(maxSub, sub);
    maxChunks = std::max(maxChunks, (size_t)h.blobSize / 4096 + 2);
  }
  need += maxSub * 4 + maxSub / nD * 2 + 5 * (maxChunks + 1024) * 4 + (dt <= DT_Byte ? huffmanScratchBytes(nPix, nD) : 0);
  {
    size_t cand = 0;    // (k_rank_chunks' table: a word per candidate -- one raw block + 1 of them, 1100 at most, to a chunk of 4 KiB)
    for (int i = 0; i < rq.nBands; i++) cand = std::max(cand, std::min<size_t>(1100, 2 + (size_t)bands[i].hd.mbSize * bands[i].hd.mbSize * tb));
    need += (maxChunks + 2) * (cand + 3) * 4;
  }
  need += fastBandWorkspace(nRows, nCols, rq.blobSize) + 4096;    // streaming path tables
  for (int i = 0; i < rq.nBands; i++)
    if (bands[i].hd.tryHuffmanFlt()) { need += fplDecodeScratchBytes(nPix * nD, tb); break; }
  // masks of some size are decoded where the bits are needed (rle_kernels.hip) instead of on the host between a copy down and a copy up
  size_t rleScratch = 0;
  for (int i = 0; i < rq.nBands; i++)
    if (maskOnDevice(maskBytes, bands[i].numBytesMask))
      rleScratch = std::max(rleScratch, maskRleDecodeScratchBytes((size_t)bands[i].numBytesMask));
  return need + rleScratch + (rleScratch ? 256 : 0);
}

// the valid pixels a mask names (BitMask::CountValidBits over the raster's nPix bits, most significant bit first)
i64 countValidBits(const u8* bits, i64 nPix)
{
  i64 cnt = 0;
  const size_t whole = (size_t)(nPix >> 3);
  size_t i = 0;
  for (; i + 8 <= whole; i += 8) { u64 w8; memcpy(&w8, bits + i, 8); cnt += __builtin_popcountll(w8); }
  for (; i < whole; i++) cnt += __builtin_popcount((unsigned)bits[i]);
  if (nPix & 7) cnt += __builtin_popcount((unsigned)bits[whole] & (0xFF00u >> (nPix & 7)) & 0xFFu);
  return cnt;
}

// ------------------------------------------------------------------------------------------------
// The mask in force (Lerc2::ReadMask, Lerc2.cpp:961-1008), from band to band.  begin() fetches a band's mask bytes -- or starts
// their decoding on the device, beside the call's stream --; finish() decodes them on the host and sends the bits, in tiling mode
// behind the launch of the chunk walk, which needs no mask.
// ------------------------------------------------------------------------------------------------
struct BandMask
{
  Context& ctx;
  BlobReader& rd;
  const hipStream_t st;
  const i64 nPix;
  const size_t maskBytes, rangeBytes;    // rangeBytes: the few header bytes behind a mask, fetched with it
  u8* dBits = nullptr;
  DeviceStatus* dStatus = nullptr;
  bool have = false, allValid = true;
  bool pending = false;          // a band's mask bytes are fetched (rle) but not decoded / sent yet: finish()
  hipStream_t side = nullptr;    // the mask is being decoded on the device beside the call's stream: finish() joins the two
  std::vector<u8> rle;
  bool auxInFlight = false;      // the pinned mask area is the source of a copy that may not have run yet
  std::vector<std::vector<u8> > keepBits;    // pageable sources of enqueued copies, where there is no pinned area
  i64 hostCount = -1;            // set bits among the nPix of a mask the HOST decoded (finish), for soundCount
  bool fromDevice = false;       // the mask's bits come out of launchMaskRleDecode (the verdict on its stream is still out)
  u8* dBytesOut = nullptr;       // the caller's byte mask of this band, until it is written
  const BandDesc* band = nullptr;

  BandMask(Context& c, BlobReader& r, i64 pixels, size_t rangeB)
    : ctx(c), rd(r), st(c.activeStream()), nPix(pixels), maskBytes((size_t)((pixels + 7) >> 3)), rangeBytes(rangeB) {}
  const u8* dMask() const { return allValid ? nullptr : dBits; }
  hipStream_t stream() const { return side ? side : st; }
  u32 begin(const BandDesc& bd, const u8* dBand, u8* dBytesOutBand);
  bool finish(bool joinSide = true);
  bool soundCount(i64& count);
};

u32 BandMask::begin(const BandDesc& bd, const u8* dBand, u8* dBytesOutBand)
{
  band = &bd;
  dBytesOut = dBytesOutBand;
  const u64 at = bd.offset + bd.hdrLen + 4, bandEnd = bd.offset + (u64)(u32)bd.hd.blobSize;
  const int nv = bd.hd.numValid;
  if ((nv == 0 || nv == (int)nPix) && bd.numBytesMask != 0) return kFailed;
  if (nv == 0) { have = true; allValid = false; hipMemsetAsync(dBits, 0, maskBytes, st); }
  else if (nv == (int)nPix) { have = true; allValid = true; }
  else if (bd.numBytesMask > 0)
  {
    // fetched now (with the few header bytes behind it, so that the later reads cost no round trip)
    if (at + (u64)bd.numBytesMask > bandEnd) return kFailed;
    const size_t extra = std::min<size_t>(rangeBytes, (size_t)(bandEnd - (at + (u64)bd.numBytesMask)));
    bool onDevice = maskOnDevice(maskBytes, bd.numBytesMask);
    u8* scratch = onDevice ? ctx.allocT<u8>(maskRleDecodeScratchBytes((size_t)bd.numBytesMask)) : nullptr;
    if (!scratch) onDevice = false;    // (no room for the tables: the host decodes the stream)
    fromDevice = onDevice;
    if (onDevice)
    {
      // decoded on the device, in front of the band's kernels; a damaged stream raises Failed in the status the call ends on.
      // The host fetches the header bytes behind the mask only.
      rle.resize(extra);    // (read first: the copy waits for what the stream holds)
      if (extra && !rd.read(at + (u64)bd.numBytesMask, extra, rle.data())) return kFailed;
      rd.cache = rle.data(); rd.cacheOff = at + (u64)bd.numBytesMask; rd.cacheLen = rle.size();
      // (beside the stream: half a dozen small launches and a chain of dependent loads that keep no CU busy, while the
      // stream goes on with the chunk tables, which need no mask)
      side = ctx.auxEvent() ? ctx.forkSide() : nullptr;
      { ProfScope ps(ctx, "mask_rle_decode"); launchMaskRleDecode(dBand + (at - bd.offset), (u32)bd.numBytesMask, dBits, (u32)maskBytes, scratch, dStatus, stream()); }
    }
    else
    {
      rle.resize((size_t)bd.numBytesMask + extra);
      if (!rd.read(at, rle.size(), rle.data())) return kFailed;
      rd.cache = rle.data(); rd.cacheOff = at; rd.cacheLen = rle.size();
      pending = true;
    }
    have = true; allValid = false;
  }
  else if (!have || allValid) return kFailed;    // "use previous mask" without a usable one
  return kOk;
}

bool BandMask::finish(bool joinSide)
{
  if (pending)
  {
    pending = false;
    // the bits are put together in pinned memory and travel while the host goes on (the area is free again once its
    // event has passed); without it: a pageable vector that lives until the call's final wait
    u8* hostBits = nullptr;
    if (ctx.auxEvent())
    {
      if (auxInFlight && hipEventSynchronize(ctx.auxEvent()) != hipSuccess) return false;
      auxInFlight = false;
      hostBits = (u8*)ctx.pinnedAux(maskBytes);
    }
    const bool pinnedBits = hostBits != nullptr;
    if (!pinnedBits) { keepBits.emplace_back(maskBytes, (u8)0); hostBits = keepBits.back().data(); }
    size_t written = 0;
    if (!rleDecode(rle.data(), (size_t)band->numBytesMask, hostBits, maskBytes, &written)) return false;
    if (pinnedBits && written < maskBytes) memset(hostBits + written, 0, maskBytes - written);
    // what the one-sweep kernel is bounded by -- Lerc2::ReadDataOneSweep asks the mask, not the header (Lerc2.cpp:1379-1385)
    hostCount = countValidBits(hostBits, nPix);
    hipMemcpyAsync(dBits, hostBits, maskBytes, hipMemcpyHostToDevice, st);
    if (pinnedBits) { hipEventRecord(ctx.auxEvent(), st); auxInFlight = true; }
  }
  if (side) ctx.sideInUse();
  if (dBytesOut) { launchBitsToBytes(dMask(), dBytesOut, nPix, stream()); dBytesOut = nullptr; }
  if (side && joinSide)
  {
    if (hipEventRecord(ctx.auxEvent(), side) != hipSuccess || hipStreamWaitEvent(st, ctx.auxEvent(), 0) != hipSuccess) return false;
    side = nullptr;
  }
  return true;
}

// The one-sweep and the Huffman kernels take the mask's word for which pixels the stream holds, and how many: before they
// run, the mask has to be sound -- out of a run-length stream that was intact (on the device that verdict would otherwise come
// with the call's last wait, after kernels had gone by a mask that may be anything) -- and its OWN count of valid pixels is what
// bounds the one-sweep reader (m_bitMask.CountValidBits(), Lerc2.cpp:1379-1385; the header's count is not asked, there or in
// Lerc2::ReadMask, Lerc2.cpp:961-1008: a blob whose header names another number than its mask holds decodes like the
// reference's, or fails like it).  A mask the host decoded has been counted by finish(); one the device decoded costs one
// wait, for masked bands in those modes only.  (The block kernels of the tiling mode check every block against its valid
// count themselves.)
bool BandMask::soundCount(i64& count)
{
  count = (i64)nPix;
  if (!dMask()) return true;
  if (!finish()) return false;
  if (!fromDevice) { count = hostCount >= 0 ? hostCount : (i64)band->hd.numValid; return true; }
  const i64 nGroups = (nPix + 31) >> 5;
  const size_t mark = ctx.used();
  const u32* dBase = enqueueMaskCount(ctx, dMask(), nPix, st);
  u32* pinV = (u32*)ctx.pinned(64);
  if (!dBase || !pinV) return false;
  hipMemcpyAsync(pinV, dBase + nGroups, 4, hipMemcpyDeviceToHost, st);
  hipMemcpyAsync(pinV + 4, dStatus, sizeof(DeviceStatus), hipMemcpyDeviceToHost, st);
  if (!ctx.sync()) return false;
  ctx.rewind(mark);
  const DeviceStatus* hsNow = reinterpret_cast<const DeviceStatus*>(pinV + 4);
  if (hsNow->error) { ctx.lastError = "device kernel reported an error"; return false; }
  count = (i64)pinV[0];
  return true;
}

// ------------------------------------------------------------------------------------------------
// One call.  Everything an enqueued copy reads from is a member, and the destructor waits for the stream before the members go.
// ------------------------------------------------------------------------------------------------
struct Stage    // what a per-band stage says: go on with the next one, the band is done, or the call ends with a status
{
  enum Kind { kGoOn, kBandDone, kStatus } kind;
  u32 rc;
  static Stage goOn() { return { kGoOn, kOk }; }
  static Stage done() { return { kBandDone, kOk }; }
  static Stage fail(u32 status) { return { kStatus, status }; }
  bool on() const { return kind == kGoOn; }
};

struct CallDecoder
{
  // ---- the call
  Context& ctx;
  const DecodeRequest& rq;
  const int fastLevel;
  const bool allowFast;
  const hipStream_t st;
  const int dt, nD, nCols, nRows, tb;
  const i64 nPix;
  BlobReader rd;
  std::vector<BandDesc> bands;
  bool passNoData = false;
  bool enqueued = false;         // something may be in flight that reads the members below
  // ---- device side: the blob, and what the host reads back at the end -- [status 64 B] then one cell per band; one memset before, one copy after
  const u8* dBlob = nullptr;
  size_t cellsBytes = 0;
  u8* dCells = nullptr;
  DeviceStatus* dStatus = nullptr;
  double* dZMax = nullptr;
  u64* dFl = nullptr;
  u8* dPixel = nullptr;
  size_t bandMark = 0;
  // ---- host buffers the enqueued copies read from
  BandMask mask;
  std::vector<std::vector<double> > keepZMax;
  std::vector<u8> pixel, small;
  std::vector<u32> expectChecksum, checksumLen;
  // bands decoded by the streaming kernels: their checksum comes out of the decode kernel itself
  // (a band of its own epoch each: the bands share the context's epoch-tagged cells, and cells left by the band before must
  // not look like this band's)
  struct FastBand { bool used = false; bool offsetsOnly = false; StreamTicket ticket; };    // ticket: of the band's launch (a masked band's scan: its epoch only); offsetsOnly: a masked band whose block offsets the scanning decoder's first half found (its flags count, nothing else of the cell)
  std::vector<FastBand> fast;
  // ---- the band in hand
  int iBand = 0;
  const BandDesc* bd = nullptr;
  const u8* dBand = nullptr;
  u8* dOutBand = nullptr;
  u32 blobEnd = 0;
  u64 at = 0;                    // the next byte of the blob to look at
  bool fastBand = false;
  u32 fastDataBegin = 0;
  std::vector<double> zMinVec, zMaxVec;
  int imageMode = IEM_Tiling;
  BandParams bp;
  DecodeArgs da;
  WalkPlan wp;
  WalkBuffers wb;
  u16* nValidBlk = nullptr;      // valid pixels per block, where the blocks differ

  CallDecoder(Context& c, const DecodeRequest& r, int level)
    : ctx(c), rq(r), fastLevel(level), allowFast(level > 0), st(c.activeStream()), dt(r.dt), nD(r.nDepth), nCols(r.nCols), nRows(r.nRows),
      tb(dtSize(r.dt)), nPix((i64)r.nRows * r.nCols), rd{ r.hBlob, r.dBlob, r.blobSize, st, nullptr, 0, 0, &c },
      mask(c, rd, nPix, (size_t)2 * r.nDepth * dtSize(r.dt) + 2) {}
  ~CallDecoder() { if (enqueued) ctx.sync(); }

  const Header& hd() const { return bd->hd; }
  u32 bandOffset() const { return (u32)(at - bd->offset); }
  u8* cell(int band) const { return dCells + 64 + (size_t)band * kCellBytes; }

  u32 open();                    // headers, request check, workspace
  u32 band(int i);
  Stage pixels();
  void fastEligible();
  void fillConst(bool perDepth);
  Stage constOrEmpty();
  Stage oneSweep();
  Stage entropyModes();
  Stage tilingStreaming();
  Stage tilingTables();
  Stage tilingScanOffsets();
  Stage tilingGeneral();
  u32 verdicts(bool& fellBack);
};

// ---- walk the band headers (Lerc::GetLercInfo), check the caller's request against them, lay out the workspace
u32 CallDecoder::open()
{
  const bool walked = walkBands(rd, rq.blobSize, bands) == kOk;
  if (bands.empty() || bands[0].hd.version < 1)
  {
    u8 magic[10];
    if (rq.blobSize >= 10 && rd.read(0, 10, magic) && memcmp(magic, "CntZImage ", 10) == 0) return decodeLerc1(ctx, rq);    // legacy Lerc1
    return kFailed;    // neither Lerc2 nor Lerc1
  }
  if (!walked) return kFailed;
  int usesNoData = 0;
  for (const BandDesc& b : bands) if (b.hd.passNoData) usesNoData++;
  if (rq.nMasks < bandsMaskCount(bands)) return kWrongParam;
  if (rq.nBands > (int)bands.size()) return kWrongParam;
  passNoData = usesNoData && nD > 1;    // Lerc.cpp:430-441: only the _4D entry points can hand the values out
  if (passNoData)
  {
    if (!rq.hUsesNoData || !rq.hNoDataValues) return kHasNoData;
    memset(rq.hUsesNoData, 0, (size_t)rq.nBands);
    memset(rq.hNoDataValues, 0, (size_t)rq.nBands * sizeof(double));
  }
  if (!ctx.reserve(workspaceBytes(rq, bands))) return kFailed;

  dBlob = rq.dBlob;
  if (!dBlob)
  {
    u8* stage = ctx.allocT<u8>((size_t)rq.blobSize + 16);
    if (!stage) return kFailed;
    hipMemcpyAsync(stage, rq.hBlob, rq.blobSize, hipMemcpyHostToDevice, st);
    dBlob = stage;
  }
  mask.dBits = ctx.allocT<u8>(mask.maskBytes + 64);
  cellsBytes = 64 + (size_t)rq.nBands * kCellBytes;
  dCells = ctx.allocT<u8>(cellsBytes);
  dStatus = reinterpret_cast<DeviceStatus*>(dCells);
  mask.dStatus = dStatus;
  dZMax = ctx.allocT<double>(nD);
  dFl = ctx.allocT<u64>((size_t)kFletcherPartials * rq.nBands);
  dPixel = ctx.allocT<u8>((size_t)nD * 8);
  if (!mask.dBits || !dCells || !dZMax || !dFl || !dPixel) return kFailed;
  hipMemsetAsync(dCells, 0, cellsBytes, st);
  enqueued = true;
  expectChecksum.assign(rq.nBands, 0);
  checksumLen.assign(rq.nBands, 0);
  fast.assign(rq.nBands, FastBand());
  // what a band's kernels take from the workspace (mask tables, chunk tables, block offsets ...) is sized for ONE band: every band
  // starts where the first one did.  The bands' kernels run in the order they are enqueued on the call's stream, and the side
  // stream a mask is decoded on is forked behind everything the band in front enqueued, so a band's tables are dead when the
  // next band's kernels write theirs.
  bandMark = ctx.used();
  return kOk;
}

// Can the streaming kernels take this band?  (unmasked, nDepth 1, 8 x 8 tiling mode, friendly dimensions;
// for such bands the ranges and mode bytes sit inside the header bytes we already hold)
void CallDecoder::fastEligible()
{
  fastDataBegin = 0;
  fastBand = false;
  const Header& h = hd();
  if (!(allowFast && bd->numBytesMask == 0 && h.numValid == (int)nPix && h.zMin != h.zMax && h.version >= 3 && h.maxZErr > 0
    && fastDecodeEligible(dt, h.version, h.mbSize, nRows, nCols, nD, true)
    && ((uintptr_t)dBand & 15) == 0 && ((uintptr_t)dOutBand & 15) == 0))
    return;
  size_t at0 = bd->hdrLen + 4;
  bool rangesDiffer = true;
  if (h.version >= 4)
  {
    if (at0 + 2 * (size_t)tb < bd->headLen) rangesDiffer = memcmp(bd->head + at0, bd->head + at0 + tb, tb) != 0;
    at0 += 2 * (size_t)tb;
  }
  if (rangesDiffer && at0 < bd->headLen && bd->head[at0] == 0 && at0 + 1 < (size_t)h.blobSize)
  {
    fastBand = true;
    fastDataBegin = (u32)(at0 + 1);
  }
}

u32 CallDecoder::band(int i)
{
  ctx.rewind(bandMark);
  iBand = i;
  bd = &bands[i];
  const Header& h = hd();
  if (h.nDepth != nD || h.nCols != nCols || h.nRows != nRows) return kFailed;
  if (h.dt != dt) { ctx.lastError = "data type of the blob differs from the requested one"; return kFailed; }
  dBand = dBlob + bd->offset;
  blobEnd = (u32)h.blobSize;
  rd.cache = bd->head; rd.cacheOff = bd->offset; rd.cacheLen = bd->headLen;
  dOutBand = (u8*)rq.dOut + (size_t)i * nPix * nD * tb;
  fastEligible();
  if (h.version >= 3)
  {
    if (h.blobSize < 14) return kFailed;
    if (!fastBand) { ProfScope ps(ctx, "fletcher_dec"); launchFletcher(dBand + 14, blobEnd - 14, dFl + (size_t)i * kFletcherPartials, st); }
    expectChecksum[i] = h.checksum;
    checksumLen[i] = blobEnd - 14;
  }
  u32 rc = mask.begin(*bd, dBand, (i < rq.nMasks && rq.dValidBytes) ? rq.dValidBytes + (size_t)i * nPix : nullptr);
  if (rc != kOk) return rc;
  at = bd->offset + bd->hdrLen + 4 + (u64)bd->numBytesMask;
  if (passNoData)
  {
    rq.hUsesNoData[i] = h.passNoData ? 1 : 0;
    rq.hNoDataValues[i] = h.noDataValOrig;
  }
  const Stage s = pixels();
  if (s.kind != Stage::kBandDone) return s.kind == Stage::kStatus ? s.rc : kFailed;
  // noData value of this band: the remapped value in the decoded pixels is turned back into the caller's original one
  // (Lerc.cpp:488-510), behind the band's kernels
  if (passNoData && h.passNoData && h.noDataVal != h.noDataValOrig)
    launchNoDataRemap(dt, dOutBand, nullptr, mask.dMask(), nPix, nD, h.noDataVal, h.noDataValOrig, st);
  return kOk;
}

Stage CallDecoder::pixels()
{
  Stage s = constOrEmpty();
  if (s.on()) s = oneSweep();
  if (s.on()) s = entropyModes();
  if (s.on()) s = tilingStreaming();
  if (!s.on()) return s;
  // ---- tiling mode: discover the block offsets, then decode
  if (!(s = tilingTables()).on()) return s;
  // A band with a mask, 8 x 8 blocks, one value a pixel: the scanning decoder's first half cuts the stream into blocks (tile_fast_decode_scan.hip,
  // MODE 1: count bytes of 1 ... 64) instead of the general discovery, which looks at every byte position (0.5 ms for the
  // 96 MB of the masked 8192^2 raster).  It hands a stream it does not follow on: the caller repeats the band with level 0.
  const bool scanOffsets = allowFast && !ctx.scanOffsetsBan && nValidBlk && mask.dMask() && bp.mb == 8 && nD == 1 && tb >= 2 && hd().version >= 3 && scanOffsetsOn();
  if (!(s = scanOffsets ? tilingScanOffsets() : tilingGeneral()).on()) return s;
  da.blockOff = wb.blockOff;
  da.nValidBlk = nValidBlk;
  { ProfScope ps(ctx, "tile_decode"); launchTileDecode(dt, bp, da, dStatus, st); }
  return Stage::done();
}

void CallDecoder::fillConst(bool perDepth)
{
  pixel.resize((size_t)nD * tb);
  for (int m = 0; m < nD; m++)
  {
    // (T)hd.zMin resp. (T)m_zMinVec[m] (Lerc2.cpp:2681-2721)
    const u64 bits = typedBits(perDepth ? zMinVec[m] : hd().zMin, dt);
    putBytes(&pixel[(size_t)m * tb], bits, tb);
  }
  hipMemcpyAsync(dPixel, pixel.data(), pixel.size(), hipMemcpyHostToDevice, st);
  launchFill(dOutBand, dPixel, nD * tb, mask.dMask(), nPix, st);
  hipStreamSynchronize(st);
}

// no valid pixel, one value throughout, one value per depth; reads the ranges on its way
Stage CallDecoder::constOrEmpty()
{
  const Header& h = hd();
  if (h.numValid == 0)
  {
    if (!mask.finish()) return Stage::fail(kFailed);
    hipMemsetAsync(dOutBand, 0, (size_t)nPix * nD * tb, st);
    return Stage::done();
  }
  zMinVec.assign(nD, h.zMin); zMaxVec.assign(nD, h.zMax);
  if (h.zMin == h.zMax) { if (!mask.finish()) return Stage::fail(kFailed); fillConst(false); return Stage::done(); }
  if (h.version >= 4)
  {
    small.resize(2 * (size_t)nD * tb);
    if (!rd.read(at, small.size(), small.data())) return Stage::fail(kFailed);
    for (int m = 0; m < nD; m++)
    {
      zMinVec[m] = typedFromBits(getBytes(&small[(size_t)m * tb], tb), dt);
      zMaxVec[m] = typedFromBits(getBytes(&small[(size_t)(nD + m) * tb], tb), dt);
    }
    at += small.size();
    if (0 == memcmp(zMinVec.data(), zMaxVec.data(), nD * sizeof(double))) { if (!mask.finish()) return Stage::fail(kFailed); fillConst(true); return Stage::done(); }
  }
  return Stage::goOn();
}

// one sweep: valid pixels stored raw in order (Lerc2.cpp:1368-1400) -- as many as the MASK names, not as many as the header
// says: k_one_sweep reads the stream by the mask's ranks, so a header that names fewer pixels than its mask holds in front of a
// stream cut to match must not get past this bound
Stage CallDecoder::oneSweep()
{
  u8 flag = 0;
  if (bandOffset() >= blobEnd || !rd.read(at, 1, &flag)) return Stage::fail(kFailed);
  at += 1;
  if (!flag) return Stage::goOn();
  if (!mask.finish()) return Stage::fail(kFailed);
  i64 nSweep = 0;
  if (!mask.soundCount(nSweep)) return Stage::fail(kFailed);
  if ((u64)bandOffset() + (u64)nSweep * nD * tb > blobEnd) return Stage::fail(kFailed);
  const u8* src = dBlob + at;
  if (!mask.dMask()) hipMemcpyAsync(dOutBand, src, (size_t)nPix * nD * tb, hipMemcpyDeviceToDevice, st);
  else
  {
    hipMemsetAsync(dOutBand, 0, (size_t)nPix * nD * tb, st);
    if (!enqueueMaskedOneSweep(ctx, false, src, dOutBand, mask.dMask(), nPix, nD * tb, st)) return Stage::fail(kFailed);
  }
  return Stage::done();
}

// the image mode byte; Huffman (8-bit types) and lossless float
Stage CallDecoder::entropyModes()
{
  const Header& h = hd();
  imageMode = IEM_Tiling;
  if (h.tryHuffmanInt() || h.tryHuffmanFlt())
  {
    u8 f = 0;
    if (bandOffset() >= blobEnd || !rd.read(at, 1, &f)) return Stage::fail(kFailed);
    at += 1;
    if (f > 3 || (f > 2 && h.version < 6) || (f > 1 && h.version < 4)) return Stage::fail(kFailed);
    imageMode = f;
  }
  if (imageMode == IEM_Tiling) return Stage::goOn();
  if (!mask.finish()) return Stage::fail(kFailed);
  const u8* hBand = rq.hBlob ? rq.hBlob + bd->offset : nullptr;
  if (h.tryHuffmanFlt())
  {
    if (imageMode != IEM_DeltaDeltaHuffman) return Stage::fail(kFailed);    // Lerc2.cpp:674-678
    const u32 rc = decodeLosslessFloat(ctx, dt, hBand, dBand, bandOffset(), blobEnd, nRows, nCols, nD, dOutBand);
    return rc != kOk ? Stage::fail(rc) : Stage::done();
  }
  if (!(imageMode == IEM_DeltaHuffman || (h.version >= 4 && imageMode == IEM_Huffman))) return Stage::fail(kFailed);
  { i64 unused = 0; if (!mask.soundCount(unused)) return Stage::fail(kFailed); }
  const u32 rc = decodeHuffman(ctx, dt, hBand, dBand, bandOffset(), blobEnd, imageMode, mask.dMask(), nRows, nCols, nD, h.version, dOutBand, dStatus, bd->head, bd->headLen);
  return rc != kOk ? Stage::fail(rc) : Stage::done();
}

// tiling mode, a band fastEligible() has picked: the streaming kernels
Stage CallDecoder::tilingStreaming()
{
  const Header& h = hd();
  bp = makeBandParams(dt, nRows, nCols, nD, h.version, h.mbSize, h.maxZErr, mask.allValid);
  bp.zMaxHdr = h.zMax;
  if (fastBand && fastDataBegin == bandOffset())
  {
    FastBand& f = fast[iBand];
    f.ticket.form = fastLevel; f.ticket.epoch = ctx.nextEpoch(); f.ticket.shape = { dt, nRows, nCols };
    if (!launchFastBand(ctx, f.ticket, dBand, blobEnd, dOutBand, cell(iBand))) return Stage::fail(kFailed);
    ctx.lastDecodeStreamed = true;
    f.used = true;
    if (!mask.finish()) return Stage::fail(kFailed);    // all valid: the caller's mask bytes become 1s (Lerc.cpp:464-488 always writes them)
    return Stage::done();
  }
  if (fastBand)    // launched without its checksum kernel, but did not qualify after all
  {
    ProfScope ps(ctx, "fletcher_dec");
    launchFletcher(dBand + 14, blobEnd - 14, dFl + (size_t)iBand * kFletcherPartials, st);
  }
  return Stage::goOn();
}

// the general block kernels' arguments and tables
Stage CallDecoder::tilingTables()
{
  keepZMax.push_back(zMaxVec);
  hipMemcpyAsync(dZMax, keepZMax.back().data(), (size_t)nD * 8, hipMemcpyHostToDevice, st);
  da.blob = dBand; da.dataBegin = bandOffset(); da.blobEnd = blobEnd;
  da.maskBits = mask.dMask(); da.zMaxVec = dZMax; da.out = dOutBand; da.blockOff = nullptr; da.nValidBlk = nullptr;
  wp = makeWalkPlan(bp, da.dataBegin, da.blobEnd, hd().numValid);
  wp.test = fastTestGiveUp() & 24u;
  wb.chunkExit = ctx.allocT<u32>(wp.nChunks + 4);
  wb.chunkEntry = ctx.allocT<u32>(wp.nChunks + 4);
  wb.chunkCount = ctx.allocT<u32>(wp.nChunks + 4);
  wb.chunkBase = ctx.allocT<u32>(wp.nChunks + 8);
  wb.blockOff = ctx.allocT<u32>((size_t)wp.nSub + 4);
  wb.scratch = ctx.allocT<u32>(wp.nChunks / 1024 + 8);
  wb.candTab = wp.tabled ? ctx.allocT<u32>((size_t)wp.nChunks * wp.candWindow + 4) : nullptr;
  wb.chunkSub = wp.tabled ? ctx.allocT<u32>(3 * (size_t)wp.nChunks + 4) : nullptr;
  if (wp.tabled && (!wb.candTab || !wb.chunkSub)) return Stage::fail(kFailed);
  nValidBlk = nullptr;
  if (wp.uniformN == 0)
  {
    nValidBlk = ctx.allocT<u16>((size_t)bp.nTV * bp.nTH + 4);
    if (!nValidBlk) return Stage::fail(kFailed);
  }
  wb.nValidBlk = nValidBlk;
  if (!wb.chunkExit || !wb.chunkEntry || !wb.chunkCount || !wb.chunkBase || !wb.blockOff || !wb.scratch) return Stage::fail(kFailed);
  return Stage::goOn();
}

Stage CallDecoder::tilingScanOffsets()
{
  const u32 nPos = (u32)bp.nTV * (u32)bp.nTH;
  FastDecodeBuffers fbuf;
  memset(&fbuf, 0, sizeof(fbuf));
  const size_t sWg = fastAnyWgStride(blobEnd, tb), sGrp = fastAnyGroupStride(blobEnd, tb);
  fbuf.wgStride = (u32)sWg; fbuf.wgGroupStride = (u32)sGrp;
  fbuf.wgCell = (u64*)ctx.persistentState(1, (sWg + sGrp + 8) * 8);
  fbuf.wgGroupCell = fbuf.wgCell ? fbuf.wgCell + sWg : nullptr;
  fbuf.wgAcc = (u64*)ctx.persistentState(0, (sGrp + 8) * 8);
  if (!fbuf.wgCell || !fbuf.wgAcc) return Stage::fail(kFailed);
  FastBand& f = fast[iBand];
  f.ticket.epoch = ctx.nextEpoch();
  f.offsetsOnly = true;
  fbuf.params = reinterpret_cast<FastDecodeParams*>(cell(iBand) + kCellParams);
  fbuf.fallback = reinterpret_cast<u32*>(cell(iBand) + kCellFallback);
  fbuf.epoch = f.ticket.epoch;
  fbuf.publishEpoch = (fastTestGiveUp() & 2u) ? fbuf.epoch ^ 0x5A5A5A5Au : fbuf.epoch;
  fbuf.spinLimit = (fastTestGiveUp() & 2u) ? 8u : (1u << 22);
  // (the scan needs no mask: it runs while the host decodes the mask's RLE and sends the bits)
  { ProfScope ps(ctx, "scan_offsets");
    launchFastScanOffsets(dt, nRows, nCols, dBand, (u32)hd().version, da.dataBegin, blobEnd, wb.blockOff, nPos, fbuf, st); }
  if (!mask.finish(false)) return Stage::fail(kFailed);
  launchBlockValidCounts(mask.dMask(), bp, nValidBlk, mask.stream());
  if (!mask.finish()) return Stage::fail(kFailed);    // (joins the side stream, if the mask went that way)
  return Stage::goOn();
}

Stage CallDecoder::tilingGeneral()
{
  // the chunk candidates need no mask: they run while the host decodes the mask's RLE and sends the bits
  { ProfScope ps(ctx, "walk_chunks"); launchWalkChunks(bp, wp, da, wb, st); }
  if (!mask.finish(false)) return Stage::fail(kFailed);
  if (nValidBlk) launchBlockValidCounts(mask.dMask(), bp, nValidBlk, mask.stream());
  if (!mask.finish()) return Stage::fail(kFailed);    // (joins the side stream, if the mask went that way)
  { ProfScope ps(ctx, "walk_offsets"); launchWalkRest(bp, wp, da, wb, dStatus, st); }
  return Stage::goOn();
}

// ---- one sync: kernel status + checksums
u32 CallDecoder::verdicts(bool& fellBack)
{
  bool anyGeneric = false;
  for (int i = 0; i < rq.nBands; i++) if (!fast[i].used) anyGeneric = true;
  u8* pin = (u8*)ctx.pinned(cellsBytes);
  if (!pin) return kFailed;
  std::vector<u64> hFl(anyGeneric ? (size_t)kFletcherPartials * rq.nBands : 0);
  hipMemcpyAsync(pin, dCells, cellsBytes, hipMemcpyDeviceToHost, st);
  if (anyGeneric) hipMemcpyAsync(hFl.data(), dFl, hFl.size() * 8, hipMemcpyDeviceToHost, st);
  if (!ctx.sync()) return kFailed;
  const DeviceStatus hs = *reinterpret_cast<const DeviceStatus*>(pin);
  u32 nScanned = 0;
  for (int i = 0; i < rq.nBands; i++)
  {
    if (fast[i].offsetsOnly)
    {
      u32 cells[4];
      memcpy(cells, pin + 64 + (size_t)i * kCellBytes + kCellFallback, 16);
      const u32 bits = fastFlagBits(cells, fast[i].ticket.epoch);
      if (bits & kVerdictGaveUp) ctx.wipePersistentState();
      if (bits)    // the caller repeats with the general kernels' own discovery
      {
        char msg[112];
        snprintf(msg, sizeof(msg), "the scan did not find band %d's blocks (reason bits 0x%x): the general discovery takes it", i, bits);
        ctx.lastNote = msg;
        ctx.scanOffsetsBan = true;    // (for the rest of this call)
        ctx.tiers.refusalCount[1]++;
        fellBack = true;
        return kOk;
      }
      nScanned++;
      continue;
    }
    if (!fast[i].used) continue;
    u32 bandEnd = 0;
    const u32 verdict = fastBandVerdict(pin + 64 + (size_t)i * kCellBytes, fast[i].ticket.epoch, &bandEnd);
    if (verdict & kVerdictGaveUp) ctx.wipePersistentState();    // (a workgroup gave up waiting: the checksum accumulators may hold residue)
    if (verdict & kVerdictBadChecksum) return kFailed;    // decoded, but the checksum is wrong
    // (these launches are sized by the band's true size, which the host has read: the launch that is too small for its band, which
    // judge() forgives a queued decode, cannot arise here.  A header the kernels rule out although the host let it through -- a flag
    // byte of codec 6 -- sends the band on without counting as a launch thrown away, as it does for the blind attempt)
    if (!ctx.tiers.judge(fast[i].ticket, verdict, bandEnd))    // caller repeats with the next tier
    {
      char msg[96];
      snprintf(msg, sizeof(msg), "streaming decode handed band %d to the general kernels (reason bits 0x%x)", i, verdict);
      ctx.lastNote = msg;
      fellBack = true;
      return kOk;
    }
  }
  for (int i = 0; i < rq.nBands; i++)
  {
    if (bands[i].hd.version < 3) continue;
    if (fast[i].used) continue;    // checked on the device
    u64 A = 0, B = 0;
    for (int k = 0; k < kFletcherPartials; k += 2) { A += hFl[(size_t)i * kFletcherPartials + k]; B += hFl[(size_t)i * kFletcherPartials + k + 1]; }
    if (fletcherFinish(A, B, checksumLen[i]) != expectChecksum[i]) return kFailed;
  }
  if (hs.error && nScanned != 0u)
  {
    // The scan's cut of a masked band is a proposal: where it had to guess (a raw block's length is in the mask, not in the stream) the
    // decode kernel, which checks every block against the mask, may refuse it.  The general discovery has the last word.
    ctx.lastNote = "the decode kernels refused the scan's block offsets: the general discovery takes the band";
    ctx.tiers.refusalCount[0]++;
    ctx.scanOffsetsBan = true;
    fellBack = true;
    return kOk;
  }
  if (hs.error) { ctx.lastError = "device kernel reported an error"; return hs.error; }
  ctx.tiers.formCount[0] += nScanned;    // (lerc_amd_decode_forms: out[0] counts masked bands whose blocks the scan found)
  return kOk;
}

}    // namespace

u32 decodeBands(Context& ctx, const DecodeRequest& rq, int fastLevel, bool& fellBack)
{
  fellBack = false;
  ctx.lastDecodeStreamed = false;
  CallDecoder call(ctx, rq, fastLevel);
  u32 rc = call.open();
  if (rc != kOk || !call.enqueued) return rc;    // (!enqueued: a Lerc1 blob, decoded by decodeLerc1)
  for (int iBand = 0; iBand < rq.nBands; iBand++)
    if ((rc = call.band(iBand)) != kOk) return rc;
  return call.verdicts(fellBack);
}

}    // namespace lerc
