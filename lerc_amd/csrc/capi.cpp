// capi.cpp -- extern "C" boundary of liblerc_amd.so (include/lerc_amd.h).
// Argument validation and status codes follow the reference's Lerc_c_api_impl.cpp:33-304; host
// buffers are staged through HBM, all codec work happens in codec_encode.cpp / codec_decode.cpp.
// An entry point is: what it zeroes, one argument check of its family, one request builder, the driver's call.
#include "../../include/lerc_amd.h"
#include "../../include/lerc_amd_device.h"
#include "../../include/lerc_amd_depth.h"
#include "../../include/lerc_amd_nodata.h"
#include "codec.h"

#include <sys/syscall.h>
#include <unistd.h>

#include <algorithm>
#include <cstdio>
#include <deque>
#include <new>
#include <vector>

using namespace lerc;

// an operation of the asynchronous device API that has been enqueued but not waited for
struct AsyncOp
{
  unsigned ticket = 0;
  bool isEncode = false;
  EncodeRequest er;
  DecodeRequest dr;
  bool streamed = false;    // its streaming kernels and the copy of their verdict are on the stream
  StreamTicket launch;      // a decode: what was enqueued (its verdict is judged against this)
  bool done = false;
  u32 status = kOk, bytes = 0;
};

// A decode that ends in Failed leaves zeros in the caller's device buffers: the streaming kernels write pixels while the blob's
// checksum is still being summed (the reference checks first, Lerc2.cpp:592-601, and leaves the buffer alone).
static void wipeDecodeOutputs(Context& ctx, const DecodeRequest& rq)
{
  hipStream_t st = ctx.activeStream();
  const size_t nPix = (size_t)rq.nRows * rq.nCols;
  if (rq.dOut) hipMemsetAsync(rq.dOut, 0, nPix * rq.nDepth * rq.nBands * (size_t)dtSize(rq.dt), st);
  if (rq.dValidBytes && rq.nMasks > 0) hipMemsetAsync(rq.dValidBytes, 0, nPix * (size_t)rq.nMasks, st);
  hipStreamSynchronize(st);
}

struct lerc_amd_context
{
  Context ctx;
  std::deque<AsyncOp> ops;  // in enqueue order; results stay until lerc_amd_finish has handed them out
  unsigned nextTicket = 1;
  // staging buffers for the host-pointer API (grown on demand, owned by the context)
  void* io[3] = { nullptr, nullptr, nullptr };
  size_t ioCap[3] = { 0, 0, 0 };
  ~lerc_amd_context() { for (void* p : io) if (p) hipFree(p); }
  void* stage(int slot, size_t bytes)
  {
    if (bytes <= ioCap[slot]) return io[slot];
    if (io[slot]) { hipStreamSynchronize(ctx.activeStream()); hipFree(io[slot]); io[slot] = nullptr; ioCap[slot] = 0; }
    const size_t want = bytes + bytes / 16 + 4096;
    if (hipMalloc(&io[slot], want) != hipSuccess) return nullptr;
    ioCap[slot] = want;
    return io[slot];
  }
};

namespace {

// The stock entry points are re-entrant across host threads like the reference's (Lerc.cpp:448,640: no global state):
// every thread that calls them owns one context -- workspace slab, three staging buffers, pinned mirror, events --
// and gives it back when the thread ends.  The main thread's holder is destroyed while the process exits, when the HIP
// runtime may be half gone already (hipFree / hipStreamDestroy have been seen to hang there on some ROCm versions): its
// context is left to the operating system, like everything else the process owns.
struct ThreadHolder
{
  lerc_amd_context* h = nullptr;
  ~ThreadHolder()
  {
    const bool mainThread = (long)syscall(SYS_gettid) == (long)getpid();
    if (h && !mainThread)
    {
      hipStreamSynchronize(h->ctx.activeStream());    // (operations still queued: their buffers go away with the context)
      delete h;
    }
    h = nullptr;
  }
};

lerc_amd_context* threadHandle()
{
  static thread_local ThreadHolder holder;
  if (!holder.h) holder.h = new (std::nothrow) lerc_amd_context();
  return (holder.h && holder.h->ctx.ok()) ? holder.h : nullptr;
}

// ---- argument checks: one per call family.  WrongParam is always decided before DimsTooLarge; `alsoOk` carries what only the one
// entry point asks (a pointer its siblings leave to the driver, its slot rule, its mask rule) into the WrongParam half.
bool dimsOk(int nDepth, int nCols, int nRows, size_t elemSize)    // Lerc.cpp:1622-1639
{
  if (nDepth <= 0 || nCols <= 0 || nRows <= 0) return false;
  const u64 nPix = (u64)nRows * nCols, lim = INT_MAX, bpp = elemSize;
  return !(nPix > lim || bpp > lim || bpp * nDepth > lim || bpp * nDepth * nPix > lim);
}

// a single raster of the stock and the device calls: its data pointer, type and four counts; maxZErr where the call has one
bool rasterArgsOk(const void* pData, unsigned dataType, int nDepth, int nCols, int nRows, int nBands, double maxZErr = 0)
{
  return !(!pData || dataType >= DT_Undefined || nDepth <= 0 || nCols <= 0 || nRows <= 0 || nBands <= 0 || maxZErr < 0);
}

// the stock rule for masks: none, one, or one per band -- and a pointer where there are any (a pointer without masks is ignored)
bool masksArgOk(int nMasks, int nBands, const void* pValidBytes)
{
  return (nMasks == 0 || nMasks == 1 || nMasks == nBands) && !(nMasks > 0 && !pValidBytes);
}

// Band stacks are stricter: count and pointer must agree both ways, since a NULL pointer is how these calls say "every pixel valid".
bool bandStackMasksOk(int nMasks, int nBands, const void* dValidBytes)
{
  return (nMasks == 0 || nMasks == 1 || nMasks == nBands) && (nMasks == 0) == (dValidBytes == nullptr);
}

bool slotBytesOk(u64 slotBytes, bool mayBeZero) { return (slotBytes & 15u) == 0 && (mayBeZero || slotBytes != 0); }

// the device calls on one raster: the raster, the masks, then the size
lerc_status deviceRasterArgs(const void* dData, unsigned dataType, int nDepth, int nCols, int nRows, int nBands, int nMasks,
                             const void* dValidBytes, double maxZErr = 0)
{
  if (!rasterArgsOk(dData, dataType, nDepth, nCols, nRows, nBands, maxZErr)) return kWrongParam;
  if (!masksArgOk(nMasks, nBands, dValidBytes)) return kWrongParam;
  return dimsOk(nDepth, nCols, nRows, (size_t)dtSize((int)dataType)) ? kOk : kDimsTooLarge;
}

lerc_status tileBatchArgs(const lerc_amd_context* h, unsigned dataType, int nCols, int nRows, int nTiles, bool alsoOk)
{
  if (!h || dataType >= DT_Undefined || nCols <= 0 || nRows <= 0 || nTiles <= 0 || !alsoOk) return kWrongParam;
  return dimsOk(1, nCols, nRows, (size_t)dtSize((int)dataType)) ? kOk : kDimsTooLarge;
}

// depth tiles: the tile batch checks plus nDepth >= 1; the size counts nDepth values a pixel
lerc_status depthTileArgs(const lerc_amd_context* h, unsigned dataType, int nCols, int nRows, int nDepth, int nTiles, bool alsoOk)
{
  if (!h || dataType >= DT_Undefined || nCols <= 0 || nRows <= 0 || nDepth <= 0 || nTiles <= 0 || !alsoOk) return kWrongParam;
  return dimsOk(nDepth, nCols, nRows, (size_t)dtSize((int)dataType)) ? kOk : kDimsTooLarge;
}

// ---- a pitched raster cut into a grid of tiles (codec_raster_tiles.cpp): pointers, pitches, masks and slots are the driver's to check
bool rasterTileDimsOk(int nCols, int nRows, int tileCols, int tileRows, unsigned int dataType)
{
  return dimsOk(1, std::min(nCols, tileCols), std::min(nRows, tileRows), (size_t)dtSize((int)dataType));
}

lerc_status rasterTilesArgs(const lerc_amd_context* h, unsigned dataType, int nCols, int nRows, int tileCols, int tileRows, bool alsoOk = true)
{
  if (!h || dataType >= DT_Undefined || nCols <= 0 || nRows <= 0 || tileCols <= 0 || tileRows <= 0) return kWrongParam;
  if (!alsoOk) return kWrongParam;
  return rasterTileDimsOk(nCols, nRows, tileCols, tileRows, dataType) ? kOk : kDimsTooLarge;
}

// the depth rasters of lerc_amd_depth.h: the raster tile calls' check, a depth >= 1, and a tile with its depth within INT_MAX
lerc_status rasterDepthArgs(const lerc_amd_context* h, unsigned dataType, int nCols, int nRows, int nDepth, int tileCols, int tileRows, bool alsoOk = true)
{
  if (const lerc_status bad = rasterTilesArgs(h, dataType, nCols, nRows, tileCols, tileRows, nDepth >= 1 && alsoOk)) return bad;
  return dimsOk(nDepth, std::min(nCols, tileCols), std::min(nRows, tileRows), (size_t)dtSize((int)dataType)) ? kOk : kDimsTooLarge;
}

bool usesNoData(const unsigned char* pUsesNoData, int nBands)
{
  if (!pUsesNoData) return false;
  for (int i = 0; i < nBands; i++) if (pUsesNoData[i]) return true;
  return false;
}

// ---- request builders: the C arguments in, a filled request out; each request type is filled here and nowhere else
EncodeRequest encodeRequest(const void* data, unsigned dataType, int nDepth, int nCols, int nRows, int nBands, int nMasks,
                            const unsigned char* validBytes, double maxZErr, unsigned char* out, unsigned outCapacity)
{
  EncodeRequest rq;
  rq.dData = data; rq.dValidBytes = validBytes; rq.dt = (int)dataType; rq.nDepth = nDepth; rq.nCols = nCols; rq.nRows = nRows;
  rq.nBands = nBands; rq.nMasks = nMasks; rq.maxZErr = maxZErr; rq.dOut = out; rq.outCapacity = outCapacity;
  return rq;
}

// (one of hBlob / dBlob)
DecodeRequest decodeRequest(const unsigned char* hBlob, const unsigned char* dBlob, unsigned blobSize, int nMasks, unsigned char* validBytes,
                            int nDepth, int nCols, int nRows, int nBands, unsigned dataType, void* out)
{
  DecodeRequest rq;
  rq.hBlob = hBlob; rq.dBlob = dBlob; rq.blobSize = blobSize; rq.dt = (int)dataType; rq.nDepth = nDepth; rq.nCols = nCols; rq.nRows = nRows;
  rq.nBands = nBands; rq.nMasks = nMasks; rq.dOut = out; rq.dValidBytes = validBytes;
  return rq;
}

TilesEncodeRequest tilesEncodeRequest(const void* dTiles, unsigned dataType, int nCols, int nRows, int nTiles, double maxZErr, unsigned char* dArena,
                                      u64 arenaCapacity, u64* offsets, unsigned* sizes, u64 slotBytes = 0, const unsigned char* dValidBytes = nullptr,
                                      int nBands = 1, int nMasks = -1, int nDepth = 1)
{
  TilesEncodeRequest rq;
  rq.dData = dTiles; rq.dt = (int)dataType; rq.nCols = nCols; rq.nRows = nRows; rq.nTiles = nTiles; rq.maxZErr = maxZErr;
  rq.dArena = dArena; rq.arenaCapacity = arenaCapacity; rq.hOffsets = offsets; rq.hSizes = sizes; rq.slotBytes = slotBytes;
  rq.dValidBytes = dValidBytes; rq.nBands = nBands; rq.nMasks = nMasks; rq.nDepth = nDepth;
  return rq;
}

TilesDecodeRequest tilesDecodeRequest(const unsigned char* dArena, const u64* offsets, const unsigned* sizes, int nTiles, int nCols, int nRows,
                                      unsigned dataType, void* dTiles, unsigned char* dValidBytes = nullptr, int nBands = 1, int nMasks = -1, int nDepth = 1)
{
  TilesDecodeRequest rq;
  rq.dArena = dArena; rq.hOffsets = offsets; rq.hSizes = sizes; rq.dt = (int)dataType; rq.nCols = nCols; rq.nRows = nRows; rq.nTiles = nTiles;
  rq.dOut = dTiles; rq.dValidBytes = dValidBytes; rq.nBands = nBands; rq.nMasks = nMasks; rq.nDepth = nDepth;
  return rq;
}

// how a raster (or a window's buffer) lies in memory, in elements; `any`: the description may be line- or pixel-interleaved
struct RasterLayout
{
  u64 pixelPitch, rowPitch, bandPitch, maskRowPitch;
  bool any;
};
RasterLayout planes(u64 rowPitch, u64 bandPitch, u64 maskRowPitch) { return { 1, rowPitch, bandPitch, maskRowPitch, false }; }
RasterLayout strided(u64 pixelPitch, u64 rowPitch, u64 bandPitch, u64 maskRowPitch) { return { pixelPitch, rowPitch, bandPitch, maskRowPitch, true }; }

// (an encode only reads raster and mask, a decode only reads arena and tables: the request has one set of pointers for both)
RasterTilesRequest rasterTilesRequest(const void* dRaster, unsigned dataType, int nCols, int nRows, int nBands, const RasterLayout& lay, int tileCols,
                                      int tileRows, int nMasks, const unsigned char* dValidBytes, const unsigned char* dArena, const u64* offsets,
                                      const unsigned* sizes, double maxZErr = 0, u64 arenaCapacity = 0, u64 slotBytes = 0)
{
  RasterTilesRequest rq;
  rq.dRaster = const_cast<void*>(dRaster); rq.dValidBytes = const_cast<unsigned char*>(dValidBytes); rq.dt = (int)dataType;
  rq.nCols = nCols; rq.nRows = nRows; rq.nBands = nBands; rq.nMasks = nMasks; rq.tileCols = tileCols; rq.tileRows = tileRows;
  rq.pixelPitch = lay.pixelPitch; rq.anyLayout = lay.any; rq.rowPitch = lay.rowPitch; rq.bandPitch = lay.bandPitch; rq.maskRowPitch = lay.maskRowPitch;
  rq.dArena = const_cast<unsigned char*>(dArena); rq.hOffsets = const_cast<u64*>(offsets); rq.hSizes = const_cast<unsigned*>(sizes);
  rq.maxZErr = maxZErr; rq.arenaCapacity = arenaCapacity; rq.slotBytes = slotBytes;
  return rq;
}

// a depth raster (or a window's buffer): element (row, col, d) at row * rowPitch + col * pixelPitch + d * depthPitch
struct DepthLayout { u64 pixelPitch, rowPitch, depthPitch, maskRowPitch; };

// (nDepth 1: depthPitch is not looked at, and the request is the strided calls' with one band)
RasterTilesRequest rasterDepthRequest(const void* dRaster, unsigned dataType, int nCols, int nRows, int nDepth, const DepthLayout& lay, int tileCols,
                                      int tileRows, int nMasks, const unsigned char* dValidBytes, const unsigned char* dArena, const u64* offsets,
                                      const unsigned* sizes, double maxZErr = 0, u64 arenaCapacity = 0, u64 slotBytes = 0)
{
  RasterTilesRequest rq = rasterTilesRequest(dRaster, dataType, nCols, nRows, 1, strided(lay.pixelPitch, lay.rowPitch, 0, lay.maskRowPitch), tileCols, tileRows,
                                             nMasks, dValidBytes, dArena, offsets, sizes, maxZErr, arenaCapacity, slotBytes);
  rq.nDepth = nDepth; rq.depthPitch = nDepth > 1 ? lay.depthPitch : 1;
  return rq;
}

// ---- what the entry points share behind their drivers' calls
// the tail of a tile encode: slotted tiles lie at t * slotBytes (slotBytes 0: the driver's offsets stand), the arena's use is reported
lerc_status finishTilesEncode(u32 rc, u64 used, u64 slotBytes, int nTiles, u64* offsets, u64* arenaUsed)
{
  if (rc == kOk && slotBytes) for (int t = 0; t < nTiles; t++) offsets[t] = (u64)t * slotBytes;
  if (arenaUsed) *arenaUsed = used;
  return rc;
}

lerc_status encodeRasterTiles(lerc_amd_context* h, const RasterTilesRequest& rq, u64* arenaUsed)
{
  u64 used = 0;
  const u32 rc = encodeRasterTilesDevice(h->ctx, rq, used);
  return finishTilesEncode(rc, used, 0, 0, nullptr, arenaUsed);    // (rooms are handed out per shape class: the driver's offsets stand)
}

// header facts of a blob of any version; legacy Lerc1: the bands have to be decoded to know their ranges (Lerc.cpp:184-266)
u32 blobInfoAnyVersion(const u8* blob, u32 size, BlobInfo& li, double* mins, double* maxs, size_t nElem)
{
  const u32 e = getBlobInfo(blob, size, li, mins, maxs, nElem);
  if (e == kOk || !isLerc1(blob, size)) return e;
  lerc_amd_context* h = threadHandle();
  if (!h) return kFailed;
  return lerc1BlobInfo(h->ctx, blob, size, li, mins, maxs, nElem);
}

// a four-slot diagnostic read-out; no context: zeros.  (Who falls back to the calling thread's context says so at the call.)
using Counters = const unsigned long long (&)[4];
void readCounters(lerc_amd_context* h, Counters (*of)(Context&), unsigned long long out[4])
{
  for (int i = 0; i < 4; i++) out[i] = h ? of(h->ctx)[i] : 0;
}
lerc_amd_context* orThisThreads(lerc_amd_context* h) { return h ? h : threadHandle(); }    // the context behind the stock entry points

// shared by lerc_encode / lerc_computeCompressedSize and their kin: `host` holds the caller's HOST pointers in dData / dValidBytes
// until they are staged; pOut == nullptr: the size only
lerc_status encodeHost(const EncodeRequest& host, unsigned char* pOut, unsigned outSize, unsigned* result)
{
  lerc_amd_context* h = threadHandle();
  if (!h) return kFailed;
  Context& ctx = h->ctx;
  hipStream_t st = ctx.activeStream();
  const int nDepth = host.nDepth, nBands = host.nBands, nMasks = host.nMasks;
  const size_t tb = (size_t)dtSize(host.dt);
  if (!dimsOk(nDepth, host.nCols, host.nRows, tb)) return kDimsTooLarge;
  const size_t nPix = (size_t)host.nRows * host.nCols;
  const size_t dataBytes = nPix * nDepth * tb * nBands, maskBytes = (size_t)nMasks * nPix;
  u8* dData = (u8*)h->stage(0, dataBytes);
  u8* dMask = nMasks ? (u8*)h->stage(1, maskBytes) : nullptr;
  if (!dData || (nMasks && !dMask)) return kFailed;
  hipMemcpyAsync(dData, host.dData, dataBytes, hipMemcpyHostToDevice, st);
  if (nMasks) hipMemcpyAsync(dMask, host.dValidBytes, maskBytes, hipMemcpyHostToDevice, st);

  EncodeRequest rq = host;
  rq.dData = dData; rq.dValidBytes = dMask;
  u32 needed = 0, written = 0;
  if (!pOut)
  {
    const u32 rc = encodeDevice(ctx, rq, needed, written);
    if (rc == kOk) *result = needed;
    return rc;
  }
  // a blob never exceeds raw pixels + mask RLE + header + the per-depth ranges of codec >= 4 (2 * nDepth values) + a few
  // hundred bytes per band (one-sweep fallback, Lerc2.cpp:364)
  const u64 bound = (u64)nBands * (nPix * nDepth * tb + nPix / 4 + 2 * (u64)nDepth * tb + 4096);
  const u32 cap = (u32)std::min<u64>(outSize, bound);
  u8* dOut = (u8*)h->stage(2, cap);
  if (!dOut) return kFailed;
  rq.dOut = dOut; rq.outCapacity = cap;
  memset(pOut, 0, outSize);    // Lerc.cpp:374
  // Small single-band rasters the streaming kernels take: the blob's way back is enqueued behind the kernels before its
  // size is known -- the whole (small) output buffer into pinned memory -- and this thread waits once instead of twice;
  // the bytes that count are then copied on the host.  (Two waits and the gap between them are a third of such a call.)
  if (nBands == 1 && nMasks == 0 && cap <= (2u << 20))
  {
    u8* slot = (u8*)ctx.pinned(Context::kAsyncSlotBytes);
    u8* hStage = (u8*)ctx.pinnedAux(cap);
    if (slot && hStage && encodeEnqueueStreaming(ctx, rq, slot))
    {
      if (hipMemcpyAsync(hStage, dOut, cap, hipMemcpyDeviceToHost, st) != hipSuccess || !ctx.sync()) return kFailed;
      bool redo = false;
      u32 status = kOk;
      encodeStreamingVerdict(ctx, rq, slot, redo, status, needed, written);
      if (!redo)
      {
        if (status != kOk) return (lerc_status)status;
        memcpy(pOut, hStage, written);
        *result = written;
        return kOk;
      }
    }
  }
  const u32 rc = encodeDevice(ctx, rq, needed, written);
  if (rc != kOk) return rc;
  if (hipMemcpyAsync(pOut, dOut, written, hipMemcpyDeviceToHost, st) != hipSuccess) return kFailed;
  if (hipStreamSynchronize(st) != hipSuccess) return kFailed;    // (not the polling Context::sync(): the copy into the caller's pageable
                                                                 // buffer is driven by this wait)
  *result = written;
  return kOk;
}

// The stock encodes and size queries, all eight: *result is zeroed, then the checks of Lerc_c_api_impl.cpp / Lerc.cpp:339-386.
// codecVersion < 0 or the current one: the _4D call, noData arrays and all; an older one: EncodeInternal_v5, which has none.
lerc_status encodeStock(const void* pData, int codecVersion, unsigned dataType, int nDepth, int nCols, int nRows, int nBands, int nMasks,
                        const unsigned char* pValidBytes, double maxZErr, bool wantBlob, unsigned char* pOut, unsigned outSize, unsigned* result,
                        const unsigned char* pUsesNoData, const double* noDataValues)
{
  if (!result) return kWrongParam;
  *result = 0;
  if (codecVersion > kCodecVersion) return kWrongParam;
  if (!rasterArgsOk(pData, dataType, nDepth, nCols, nRows, nBands, maxZErr) || (wantBlob && (!pOut || !outSize))) return kWrongParam;
  if (!masksArgOk(nMasks, nBands, pValidBytes)) return kWrongParam;
  const bool older = codecVersion >= 0 && codecVersion < kCodecVersion;
  if (older && codecVersion < 2) return kWrongParam;    // Lerc2::SetEncoderToOldVersion (Lerc2.cpp:52-62)
  if (!older && usesNoData(pUsesNoData, nBands) && !noDataValues) return kWrongParam;
  EncodeRequest host = encodeRequest(pData, dataType, nDepth, nCols, nRows, nBands, nMasks, pValidBytes, maxZErr, nullptr, 0);
  if (older) host.version = codecVersion;
  else { host.hUsesNoData = pUsesNoData; host.hNoDataValues = noDataValues; }
  return encodeHost(host, wantBlob ? pOut : nullptr, outSize, result);
}

// `host` holds the caller's HOST pointers: the blob in hBlob, where pixels and valid bytes go in dOut / dValidBytes
lerc_status decodeHost(const DecodeRequest& host, bool toDouble)
{
  lerc_amd_context* h = threadHandle();
  if (!h) return kFailed;
  Context& ctx = h->ctx;
  hipStream_t st = ctx.activeStream();
  void* pData = host.dOut;
  unsigned char* pValidBytes = host.dValidBytes;
  const int nMasks = host.nMasks;
  const size_t tb = (size_t)dtSize(host.dt);
  if (!dimsOk(host.nDepth, host.nCols, host.nRows, tb)) return kDimsTooLarge;
  const size_t nPix = (size_t)host.nRows * host.nCols, nVals = nPix * host.nDepth * host.nBands;
  const size_t outBytes = nVals * tb, maskBytes = (size_t)nMasks * nPix;
  const bool widen = toDouble && host.dt != DT_Double;
  u8* dOut = (u8*)h->stage(0, outBytes + (widen ? nVals * 8 + 256 : 0));
  u8* dMask = nMasks ? (u8*)h->stage(1, maskBytes) : nullptr;
  if (!dOut || (nMasks && !dMask)) return kFailed;

  if (isLerc1(host.hBlob, host.blobSize))
  {
    // Lerc1 leaves pixels that are not valid as the caller's buffer had them (Lerc::Convert, Lerc.cpp:795-845): the staging
    // buffer starts out as a copy of it (lerc_decodeToDouble decodes into the tail of the double buffer, Lerc_c_api_impl.cpp:288-300)
    const u8* src = (const u8*)pData + (widen ? nVals * (8 - tb) : 0);
    hipMemcpyAsync(dOut, src, outBytes, hipMemcpyHostToDevice, st);
  }
  DecodeRequest rq = host;
  rq.dOut = dOut; rq.dValidBytes = dMask;
  StreamTicket tried;    // (form kFormGeneral: nothing enqueued -- no form has refused the blob, nothing was written)
  // What the streaming kernels can take (speculativeDecodeEligible: the header says so) goes up, through the kernels and back in
  // one go: upload, kernels, verdict and the pixels' way back are enqueued together and this thread waits once (two waits and the
  // gap between them are a quarter of a small raster's call).
  Header hd;
  size_t used = 0;
  if (!widen && readHeader(host.hBlob, host.blobSize, hd, used) && speculativeDecodeEligible(hd, rq))
  {
    u8* dBlob = (u8*)h->stage(2, (size_t)host.blobSize + 256);
    if (dBlob && hipMemcpyAsync(dBlob, host.hBlob, host.blobSize, hipMemcpyHostToDevice, st) == hipSuccess)
    {
      DecodeRequest rs = rq;
      rs.hBlob = nullptr; rs.dBlob = dBlob;
      bool handled = false;
      const u32 src = decodeSpeculativeToHost(ctx, rs, pData, outBytes, nMasks ? pValidBytes : nullptr, maskBytes, handled, tried);
      if (src != kOk) return src;
      if (handled) return kOk;
    }
  }
  const bool triedOne = tried.form > kFormGeneral;
  if (triedOne) rq.startAt(ctx.tiers.below(tried.form, tried.shape));    // (that streaming form has just refused this blob)
  const u32 rc = decodeDevice(ctx, rq);
  if (rc != kOk)
  {
    // (the reference checks the checksum before it writes a pixel, Lerc2.cpp:592-601; here the streaming kernels' pixels were on
    // their way into the caller's buffers while the checksum was being summed: what did not pass is wiped -- a failed decode
    // leaves zeros, never pixels of a blob that is damaged)
    if (triedOne)
    {
      memset(pData, 0, toDouble ? nVals * sizeof(double) : outBytes);
      if (nMasks && pValidBytes) memset(pValidBytes, 0, maskBytes);
    }
    return rc;
  }
  if (widen)
  {
    double* dWide = (double*)(dOut + ((outBytes + 255) / 256) * 256);
    launchWidenToDouble(host.dt, dOut, dWide, (i64)nVals, st);
    hipMemcpyAsync(pData, dWide, nVals * 8, hipMemcpyDeviceToHost, st);
  }
  else hipMemcpyAsync(pData, dOut, outBytes, hipMemcpyDeviceToHost, st);
  if (nMasks) hipMemcpyAsync(pValidBytes, dMask, maskBytes, hipMemcpyDeviceToHost, st);
  return hipStreamSynchronize(st) == hipSuccess ? (lerc_status)kOk : (lerc_status)kFailed;
}

}    // namespace

extern "C" {

lerc_status lerc_computeCompressedSize_4D(const void* pData, unsigned int dataType, int nDepth, int nCols, int nRows,
  int nBands, int nMasks, const unsigned char* pValidBytes, double maxZErr, unsigned int* numBytes,
  const unsigned char* pUsesNoData, const double* noDataValues)
{
  return encodeStock(pData, -1, dataType, nDepth, nCols, nRows, nBands, nMasks, pValidBytes, maxZErr, false, nullptr, 0, numBytes, pUsesNoData,
                     noDataValues);
}

lerc_status lerc_encode_4D(const void* pData, unsigned int dataType, int nDepth, int nCols, int nRows, int nBands,
  int nMasks, const unsigned char* pValidBytes, double maxZErr, unsigned char* pOutBuffer, unsigned int outBufferSize,
  unsigned int* nBytesWritten, const unsigned char* pUsesNoData, const double* noDataValues)
{
  return encodeStock(pData, -1, dataType, nDepth, nCols, nRows, nBands, nMasks, pValidBytes, maxZErr, true, pOutBuffer, outBufferSize, nBytesWritten,
                     pUsesNoData, noDataValues);
}

lerc_status lerc_computeCompressedSizeForVersion(const void* pData, int codecVersion, unsigned int dataType, int nDepth,
  int nCols, int nRows, int nBands, int nMasks, const unsigned char* pValidBytes, double maxZErr, unsigned int* numBytes)
{
  return encodeStock(pData, codecVersion, dataType, nDepth, nCols, nRows, nBands, nMasks, pValidBytes, maxZErr, false, nullptr, 0, numBytes, nullptr,
                     nullptr);
}

lerc_status lerc_encodeForVersion(const void* pData, int codecVersion, unsigned int dataType, int nDepth, int nCols,
  int nRows, int nBands, int nMasks, const unsigned char* pValidBytes, double maxZErr, unsigned char* pOutBuffer,
  unsigned int outBufferSize, unsigned int* nBytesWritten)
{
  return encodeStock(pData, codecVersion, dataType, nDepth, nCols, nRows, nBands, nMasks, pValidBytes, maxZErr, true, pOutBuffer, outBufferSize,
                     nBytesWritten, nullptr, nullptr);
}

lerc_status lerc_computeCompressedSize(const void* pData, unsigned int dataType, int nDepth, int nCols, int nRows,
  int nBands, int nMasks, const unsigned char* pValidBytes, double maxZErr, unsigned int* numBytes)
{
  return lerc_computeCompressedSizeForVersion(pData, -1, dataType, nDepth, nCols, nRows, nBands, nMasks, pValidBytes,
                                              maxZErr, numBytes);
}

lerc_status lerc_encode(const void* pData, unsigned int dataType, int nDepth, int nCols, int nRows, int nBands,
  int nMasks, const unsigned char* pValidBytes, double maxZErr, unsigned char* pOutBuffer, unsigned int outBufferSize,
  unsigned int* nBytesWritten)
{
  return lerc_encodeForVersion(pData, -1, dataType, nDepth, nCols, nRows, nBands, nMasks, pValidBytes, maxZErr, pOutBuffer,
                               outBufferSize, nBytesWritten);
}

lerc_status lerc_getBlobInfo(const unsigned char* pLercBlob, unsigned int blobSize, unsigned int* infoArray,
  double* dataRangeArray, int infoArraySize, int dataRangeArraySize)
{
  if (!pLercBlob || !blobSize || (!infoArray && !dataRangeArray) || ((infoArraySize <= 0) && (dataRangeArraySize <= 0)))
    return kWrongParam;
  BlobInfo li;
  const u32 e = blobInfoAnyVersion(pLercBlob, blobSize, li, nullptr, nullptr, 0);
  if (e != kOk) return e;
  if (infoArray)
  {
    const unsigned v[11] = { (unsigned)li.version, (unsigned)li.dt, (unsigned)li.nDepth, (unsigned)li.nCols, (unsigned)li.nRows,
      (unsigned)li.nBands, (unsigned)li.numValid, li.blobSize, (unsigned)li.nMasks, (unsigned)li.nDepth, (unsigned)li.nUsesNoData };
    if (infoArraySize > 0) memset(infoArray, 0, infoArraySize * sizeof(unsigned));
    for (int i = 0; i < infoArraySize && i < 11; i++) infoArray[i] = v[i];
  }
  if (dataRangeArray)
  {
    if (dataRangeArraySize > 0) memset(dataRangeArray, 0, dataRangeArraySize * sizeof(double));
    const bool nd = (li.nDepth > 1) && (li.nUsesNoData > 0);
    const double v[3] = { !nd ? li.zMin : -1, !nd ? li.zMax : -1, li.maxZErr };
    for (int i = 0; i < dataRangeArraySize && i < 3; i++) dataRangeArray[i] = v[i];
  }
  return kOk;
}

lerc_status lerc_getDataRanges(const unsigned char* pLercBlob, unsigned int blobSize, int nDepth, int nBands,
  double* pMins, double* pMaxs)
{
  if (!pLercBlob || !blobSize || !pMins || !pMaxs || nDepth <= 0 || nBands <= 0) return kWrongParam;
  BlobInfo li;
  return blobInfoAnyVersion(pLercBlob, blobSize, li, pMins, pMaxs, (size_t)nDepth * (size_t)nBands);
}

lerc_status lerc_decode_4D(const unsigned char* pLercBlob, unsigned int blobSize, int nMasks, unsigned char* pValidBytes,
  int nDepth, int nCols, int nRows, int nBands, unsigned int dataType, void* pData, unsigned char* pUsesNoData,
  double* noDataValues)
{
  if (!pLercBlob || !blobSize || !rasterArgsOk(pData, dataType, nDepth, nCols, nRows, nBands)) return kWrongParam;
  if (!masksArgOk(nMasks, nBands, pValidBytes)) return kWrongParam;
  DecodeRequest host = decodeRequest(pLercBlob, nullptr, blobSize, nMasks, pValidBytes, nDepth, nCols, nRows, nBands, dataType, pData);
  host.hUsesNoData = pUsesNoData; host.hNoDataValues = noDataValues;
  return decodeHost(host, false);
}

lerc_status lerc_decode(const unsigned char* pLercBlob, unsigned int blobSize, int nMasks, unsigned char* pValidBytes,
  int nDepth, int nCols, int nRows, int nBands, unsigned int dataType, void* pData)
{
  return lerc_decode_4D(pLercBlob, blobSize, nMasks, pValidBytes, nDepth, nCols, nRows, nBands, dataType, pData, nullptr, nullptr);
}

lerc_status lerc_decodeToDouble_4D(const unsigned char* pLercBlob, unsigned int blobSize, int nMasks,
  unsigned char* pValidBytes, int nDepth, int nCols, int nRows, int nBands, double* pData, unsigned char* pUsesNoData,
  double* noDataValues)
{
  if (!pLercBlob || !blobSize || !rasterArgsOk(pData, DT_Double, nDepth, nCols, nRows, nBands)) return kWrongParam;    // (the type is the blob's)
  if (!masksArgOk(nMasks, nBands, pValidBytes)) return kWrongParam;
  BlobInfo li;
  const u32 e = blobInfoAnyVersion(pLercBlob, blobSize, li, nullptr, nullptr, 0);
  if (e != kOk) return e;
  if (li.nDepth != nDepth || li.nCols != nCols || li.nRows != nRows || li.nBands != nBands) return kFailed;
  DecodeRequest host = decodeRequest(pLercBlob, nullptr, blobSize, nMasks, pValidBytes, nDepth, nCols, nRows, nBands, (unsigned)li.dt, pData);
  host.hUsesNoData = pUsesNoData; host.hNoDataValues = noDataValues;
  return decodeHost(host, true);
}

lerc_status lerc_decodeToDouble(const unsigned char* pLercBlob, unsigned int blobSize, int nMasks,
  unsigned char* pValidBytes, int nDepth, int nCols, int nRows, int nBands, double* pData)
{
  return lerc_decodeToDouble_4D(pLercBlob, blobSize, nMasks, pValidBytes, nDepth, nCols, nRows, nBands, pData, nullptr, nullptr);
}

// ---- device-pointer extension -------------------------------------------------------------------
lerc_amd_context* lerc_amd_create(void* hipStream)
{
  lerc_amd_context* h = new (std::nothrow) lerc_amd_context();
  if (!h) return nullptr;
  if (!h->ctx.ok()) { delete h; return nullptr; }
  h->ctx.setStream((hipStream_t)hipStream);
  return h;
}

void lerc_amd_destroy(lerc_amd_context* h) { delete h; }

void lerc_amd_set_stream(lerc_amd_context* h, void* hipStream) { if (h) h->ctx.setStream((hipStream_t)hipStream); }

const char* lerc_amd_last_error(lerc_amd_context* h)
{
  h = orThisThreads(h);
  return h ? h->ctx.lastError.c_str() : "no context";
}

lerc_status lerc_amd_encode_device(lerc_amd_context* h, const void* dData, unsigned int dataType, int nDepth, int nCols,
  int nRows, int nBands, int nMasks, const unsigned char* dValidBytes, double maxZErr, unsigned char* dOutBuffer,
  unsigned int outBufferSize, unsigned int* nBytesWritten)
{
  if (!h || !nBytesWritten) return kWrongParam;
  *nBytesWritten = 0;
  if (const lerc_status bad = deviceRasterArgs(dData, dataType, nDepth, nCols, nRows, nBands, nMasks, dValidBytes, maxZErr)) return bad;
  const EncodeRequest rq = encodeRequest(dData, dataType, nDepth, nCols, nRows, nBands, nMasks, dValidBytes, maxZErr, dOutBuffer, outBufferSize);
  u32 needed = 0, written = 0;
  const u32 rc = encodeDevice(h->ctx, rq, needed, written);
  if (rc == kOk) *nBytesWritten = dOutBuffer ? written : needed;
  return rc;
}

lerc_status lerc_amd_decode_device(lerc_amd_context* h, const unsigned char* dLercBlob, unsigned int blobSize, int nMasks,
  unsigned char* dValidBytes, int nDepth, int nCols, int nRows, int nBands, unsigned int dataType, void* dData)
{
  if (!h || !dLercBlob || !blobSize) return kWrongParam;
  if (const lerc_status bad = deviceRasterArgs(dData, dataType, nDepth, nCols, nRows, nBands, nMasks, dValidBytes)) return bad;
  const DecodeRequest rq = decodeRequest(nullptr, dLercBlob, blobSize, nMasks, dValidBytes, nDepth, nCols, nRows, nBands, dataType, dData);
  const u32 rc = decodeDevice(h->ctx, rq);
  if (rc == kFailed) wipeDecodeOutputs(h->ctx, rq);
  return rc;
}

// ---- asynchronous device API: operations queue up on the context's stream, the host runs ahead -------------------------
namespace {

// A streamed operation's verdict, read once the stream has passed it.  false: the streaming kernels handed it back.
bool encodeVerdict(Context& ctx, AsyncOp& op)
{
  bool redo = false;
  u32 needed = 0, written = 0;
  encodeStreamingVerdict(ctx, op.er, ctx.asyncSlot(op.ticket), redo, op.status, needed, written);
  op.bytes = op.er.dOut ? written : needed;
  return !redo;
}

bool decodeVerdict(Context& ctx, AsyncOp& op)
{
  if (!decodeStreamingVerdict(ctx, ctx.asyncSlot(op.ticket), op.launch)) return false;
  ctx.pathCount[2]++;
  return true;
}

// The blob's true length: an asynchronous decode may have been given the capacity of the buffer an encode still in flight was
// writing to; the synchronous path wants the blob's own size, which its header on the device holds.
void trimToBlobSize(DecodeRequest& dr)
{
  if (!dr.dBlob || dr.hBlob || dr.blobSize < 70) return;
  u8 head[64];
  if (hipMemcpy(head, dr.dBlob, sizeof(head), hipMemcpyDeviceToHost) != hipSuccess) return;
  BlobInfo info;
  if (getBlobInfo(head, sizeof(head), info) == kOk && info.blobSize >= 70 && info.blobSize <= dr.blobSize) dr.blobSize = info.blobSize;
}

// The operation once more, through the synchronous path.
void encodeAgain(Context& ctx, AsyncOp& op)
{
  u32 needed = 0, written = 0;
  op.status = encodeDevice(ctx, op.er, needed, written);
  op.bytes = op.er.dOut ? written : needed;
}

void decodeAgain(Context& ctx, AsyncOp& op)
{
  trimToBlobSize(op.dr);
  if (op.streamed) op.dr.startAt(ctx.tiers.below(op.launch.form, op.launch.shape));    // (that streaming form has just refused this blob)
  op.status = decodeDevice(ctx, op.dr);
  if (op.status == kFailed) wipeDecodeOutputs(ctx, op.dr);
}

// Brings every operation of the context to its result.  The stream is waited for once; verdicts are then read in enqueue
// order.  After the first operation that needs repeating -- the streaming kernels handed it back, or it never was theirs --
// everything behind it is repeated too: it may have worked on what that one had not produced yet.
void completeAll(lerc_amd_context* h)
{
  bool pending = false;
  for (const AsyncOp& op : h->ops) pending = pending || !op.done;
  if (!pending) return;
  Context& ctx = h->ctx;
  bool repeat = !ctx.sync();
  for (AsyncOp& op : h->ops)
  {
    if (op.done) continue;
    repeat = repeat || !op.streamed || !(op.isEncode ? encodeVerdict(ctx, op) : decodeVerdict(ctx, op));
    if (repeat) { if (op.isEncode) encodeAgain(ctx, op); else decodeAgain(ctx, op); }
    op.done = true;
  }
}

// Queues the operation under a new ticket -> the queued operation, whose pinned result slot is ctx.asyncSlot(ticket).
AsyncOp& pushOp(lerc_amd_context* h, const AsyncOp& op)
{
  // results nobody asked for do not pile up: beyond the pinned slots' number the oldest are brought to their end and dropped
  if (h->ops.size() >= (size_t)Context::kAsyncSlots - 1) { completeAll(h); while (h->ops.size() >= (size_t)Context::kAsyncSlots / 2) h->ops.pop_front(); }
  h->ops.push_back(op);
  AsyncOp& q = h->ops.back();
  q.ticket = h->nextTicket++;
  if (h->nextTicket == 0) h->nextTicket = 1;
  return q;
}

}    // namespace

lerc_status lerc_amd_encode_device_async(lerc_amd_context* h, const void* dData, unsigned int dataType, int nDepth, int nCols,
  int nRows, int nBands, int nMasks, const unsigned char* dValidBytes, double maxZErr, unsigned char* dOutBuffer,
  unsigned int outBufferSize, unsigned int* ticket)
{
  if (!h || !ticket) return kWrongParam;
  *ticket = 0;
  if (const lerc_status bad = deviceRasterArgs(dData, dataType, nDepth, nCols, nRows, nBands, nMasks, dValidBytes, maxZErr)) return bad;
  AsyncOp op;
  op.isEncode = true;
  op.er = encodeRequest(dData, dataType, nDepth, nCols, nRows, nBands, nMasks, dValidBytes, maxZErr, dOutBuffer, outBufferSize);
  AsyncOp& q = pushOp(h, op);
  q.streamed = encodeEnqueueStreaming(h->ctx, q.er, h->ctx.asyncSlot(q.ticket));
  if (!q.streamed) completeAll(h);    // not a request the streaming kernels take: done on the spot (in order, behind what is in flight)
  *ticket = q.ticket;
  return kOk;
}

lerc_status lerc_amd_decode_device_async(lerc_amd_context* h, const unsigned char* dLercBlob, unsigned int blobSizeBound, int nMasks,
  unsigned char* dValidBytes, int nDepth, int nCols, int nRows, int nBands, unsigned int dataType, void* dData, unsigned int* ticket)
{
  if (!h || !ticket) return kWrongParam;
  *ticket = 0;
  if (!dLercBlob || !blobSizeBound) return kWrongParam;
  if (const lerc_status bad = deviceRasterArgs(dData, dataType, nDepth, nCols, nRows, nBands, nMasks, dValidBytes)) return bad;
  AsyncOp op;
  op.dr = decodeRequest(nullptr, dLercBlob, blobSizeBound, nMasks, dValidBytes, nDepth, nCols, nRows, nBands, dataType, dData);
  AsyncOp& q = pushOp(h, op);
  q.streamed = decodeEnqueueStreaming(h->ctx, q.dr, h->ctx.asyncSlot(q.ticket), q.launch);
  if (!q.streamed) completeAll(h);
  *ticket = q.ticket;
  return kOk;
}

lerc_status lerc_amd_finish(lerc_amd_context* h, unsigned int ticket, unsigned int* nBytes)
{
  if (!h) return kWrongParam;
  if (nBytes) *nBytes = 0;
  completeAll(h);
  if (ticket == 0) { h->ops.clear(); return kOk; }    // "everything": results are dropped
  for (auto it = h->ops.begin(); it != h->ops.end(); ++it)
    if (it->ticket == ticket)
    {
      const u32 rc = it->status;
      if (nBytes) *nBytes = it->bytes;
      h->ops.erase(it);
      return rc;
    }
  return kWrongParam;    // no such operation (handed out before, or dropped behind more than kAsyncSlots / 2 newer ones)
}

// ---- tile batches (codec_tiles_batch.cpp): these calls check their pointers themselves
lerc_status lerc_amd_encode_tiles_device(lerc_amd_context* h, const void* dTiles, unsigned int dataType, int nCols, int nRows, int nTiles,
  double maxZErr, unsigned char* dArena, unsigned long long arenaCapacity, unsigned long long* offsets, unsigned int* sizes,
  unsigned long long* arenaUsed)
{
  if (const lerc_status bad = tileBatchArgs(h, dataType, nCols, nRows, nTiles, dTiles && dArena && offsets && sizes && !(maxZErr < 0))) return bad;
  u64 used = 0;
  const u32 rc = encodeTilesDevice(h->ctx, tilesEncodeRequest(dTiles, dataType, nCols, nRows, nTiles, maxZErr, dArena, arenaCapacity, offsets, sizes), used);
  return finishTilesEncode(rc, used, 0, nTiles, offsets, arenaUsed);
}

lerc_status lerc_amd_encode_tiles_device_slots(lerc_amd_context* h, const void* dTiles, unsigned int dataType, int nCols, int nRows, int nTiles,
  double maxZErr, unsigned char* dSlots, unsigned long long slotBytes, unsigned int* sizes)
{
  if (const lerc_status bad = tileBatchArgs(h, dataType, nCols, nRows, nTiles, dTiles && dSlots && sizes && !(maxZErr < 0) && slotBytesOk(slotBytes, false)))
    return bad;
  std::vector<u64> offsets((size_t)nTiles);
  u64 used = 0;    // (not reported: every slot is the caller's, t * slotBytes is where tile t lies)
  return encodeTilesDevice(h->ctx, tilesEncodeRequest(dTiles, dataType, nCols, nRows, nTiles, maxZErr, dSlots, (u64)nTiles * slotBytes, offsets.data(),
                                                      sizes, slotBytes), used);
}

lerc_status lerc_amd_decode_tiles_device_slots(lerc_amd_context* h, const unsigned char* dSlots, unsigned long long slotBytes,
  const unsigned int* sizes, int nTiles, int nCols, int nRows, unsigned int dataType, void* dTiles)
{
  if (const lerc_status bad = tileBatchArgs(h, dataType, nCols, nRows, nTiles, dSlots && sizes && dTiles && slotBytesOk(slotBytes, false))) return bad;
  std::vector<u64> offsets((size_t)nTiles);
  for (int t = 0; t < nTiles; t++) offsets[(size_t)t] = (u64)t * slotBytes;
  return decodeTilesDevice(h->ctx, tilesDecodeRequest(dSlots, offsets.data(), sizes, nTiles, nCols, nRows, dataType, dTiles));
}

lerc_status lerc_amd_decode_tiles_device(lerc_amd_context* h, const unsigned char* dArena, const unsigned long long* offsets,
  const unsigned int* sizes, int nTiles, int nCols, int nRows, unsigned int dataType, void* dTiles)
{
  if (const lerc_status bad = tileBatchArgs(h, dataType, nCols, nRows, nTiles, dArena && offsets && sizes && dTiles)) return bad;
  return decodeTilesDevice(h->ctx, tilesDecodeRequest(dArena, offsets, sizes, nTiles, nCols, nRows, dataType, dTiles));
}

lerc_status lerc_amd_encode_tiles_device_masked(lerc_amd_context* h, const void* dTiles, unsigned int dataType, int nCols, int nRows, int nTiles,
  const unsigned char* dValidBytes, double maxZErr, unsigned char* dArena, unsigned long long arenaCapacity, unsigned long long slotBytes,
  unsigned long long* offsets, unsigned int* sizes, unsigned long long* arenaUsed)
{
  if (const lerc_status bad = tileBatchArgs(h, dataType, nCols, nRows, nTiles,
                                            dTiles && dArena && offsets && sizes && !(maxZErr < 0) && slotBytesOk(slotBytes, true)))
    return bad;
  u64 used = 0;
  const u32 rc = encodeTilesDeviceMasked(h->ctx, tilesEncodeRequest(dTiles, dataType, nCols, nRows, nTiles, maxZErr, dArena, arenaCapacity, offsets, sizes,
                                                                    slotBytes, dValidBytes), used);
  return finishTilesEncode(rc, used, slotBytes, nTiles, offsets, arenaUsed);
}

lerc_status lerc_amd_decode_tiles_device_masked(lerc_amd_context* h, const unsigned char* dArena, const unsigned long long* offsets,
  const unsigned int* sizes, int nTiles, int nCols, int nRows, unsigned int dataType, void* dTiles, unsigned char* dValidBytes)
{
  if (const lerc_status bad = tileBatchArgs(h, dataType, nCols, nRows, nTiles, dArena && offsets && sizes && dTiles)) return bad;
  return decodeTilesDeviceMasked(h->ctx, tilesDecodeRequest(dArena, offsets, sizes, nTiles, nCols, nRows, dataType, dTiles, dValidBytes));
}

lerc_status lerc_amd_encode_tiles_device_bands(lerc_amd_context* h, const void* dTiles, unsigned int dataType, int nCols, int nRows, int nBands,
  int nTiles, int nMasks, const unsigned char* dValidBytes, double maxZErr, unsigned char* dArena, unsigned long long arenaCapacity,
  unsigned long long slotBytes, unsigned long long* offsets, unsigned int* sizes, unsigned long long* arenaUsed)
{
  if (const lerc_status bad = tileBatchArgs(h, dataType, nCols, nRows, nTiles, dTiles && dArena && offsets && sizes && nBands > 0 && !(maxZErr < 0)
                                            && slotBytesOk(slotBytes, true) && bandStackMasksOk(nMasks, nBands, dValidBytes)))
    return bad;
  u64 used = 0;
  const u32 rc = encodeTilesDeviceBands(h->ctx, tilesEncodeRequest(dTiles, dataType, nCols, nRows, nTiles, maxZErr, dArena, arenaCapacity, offsets, sizes,
                                                                   slotBytes, dValidBytes, nBands, nMasks), used);
  return finishTilesEncode(rc, used, slotBytes, nTiles, offsets, arenaUsed);
}

lerc_status lerc_amd_decode_tiles_device_bands(lerc_amd_context* h, const unsigned char* dArena, const unsigned long long* offsets,
  const unsigned int* sizes, int nTiles, int nCols, int nRows, int nBands, unsigned int dataType, void* dTiles, int nMasks, unsigned char* dValidBytes)
{
  if (const lerc_status bad = tileBatchArgs(h, dataType, nCols, nRows, nTiles,
                                            dArena && offsets && sizes && dTiles && nBands > 0 && bandStackMasksOk(nMasks, nBands, dValidBytes)))
    return bad;
  return decodeTilesDeviceBands(h->ctx, tilesDecodeRequest(dArena, offsets, sizes, nTiles, nCols, nRows, dataType, dTiles, dValidBytes, nBands, nMasks));
}

// ---- depth tiles (lerc_amd_depth.h): one blob with the header's nDepth a tile
lerc_status lerc_amd_encode_tiles_device_depth(lerc_amd_context* h, const void* dTiles, unsigned int dataType, int nCols, int nRows, int nDepth,
  int nTiles, const unsigned char* dValidBytes, double maxZErr, unsigned char* dArena, unsigned long long arenaCapacity, unsigned long long slotBytes,
  unsigned long long* offsets, unsigned int* sizes, unsigned long long* arenaUsed)
{
  if (const lerc_status bad = depthTileArgs(h, dataType, nCols, nRows, nDepth, nTiles,
                                            dTiles && dArena && offsets && sizes && !(maxZErr < 0) && slotBytesOk(slotBytes, true)))
    return bad;
  u64 used = 0;
  const u32 rc = encodeTilesDeviceDepth(h->ctx, tilesEncodeRequest(dTiles, dataType, nCols, nRows, nTiles, maxZErr, dArena, arenaCapacity, offsets, sizes,
                                                                   slotBytes, dValidBytes, 1, -1, nDepth), used);
  return finishTilesEncode(rc, used, slotBytes, nTiles, offsets, arenaUsed);
}

lerc_status lerc_amd_decode_tiles_device_depth(lerc_amd_context* h, const unsigned char* dArena, const unsigned long long* offsets,
  const unsigned int* sizes, int nTiles, int nCols, int nRows, int nDepth, unsigned int dataType, void* dTiles, unsigned char* dValidBytes)
{
  if (const lerc_status bad = depthTileArgs(h, dataType, nCols, nRows, nDepth, nTiles, dArena && offsets && sizes && dTiles)) return bad;
  return decodeTilesDeviceDepth(h->ctx, tilesDecodeRequest(dArena, offsets, sizes, nTiles, nCols, nRows, dataType, dTiles, dValidBytes, 1, -1, nDepth));
}

void lerc_amd_tile_batch_counters(lerc_amd_context* h, unsigned long long out[4])
{
  readCounters(h, [](Context& c) -> Counters { return c.tileBatchCount; }, out);
}

// ---- a pitched raster cut into a grid of tiles (codec_raster_tiles.cpp)
lerc_status lerc_amd_encode_raster_tiles_device(lerc_amd_context* h, const void* dRaster, unsigned int dataType, int nCols, int nRows, int nBands,
  unsigned long long rowPitch, unsigned long long bandPitch, int tileCols, int tileRows, int nMasks, const unsigned char* dValidBytes,
  unsigned long long maskRowPitch, double maxZErr, unsigned char* dArena, unsigned long long arenaCapacity, unsigned long long slotBytes,
  unsigned long long* offsets, unsigned int* sizes, unsigned long long* arenaUsed)
{
  if (arenaUsed) *arenaUsed = 0;
  if (const lerc_status bad = rasterTilesArgs(h, dataType, nCols, nRows, tileCols, tileRows)) return bad;
  return encodeRasterTiles(h, rasterTilesRequest(dRaster, dataType, nCols, nRows, nBands, planes(rowPitch, bandPitch, maskRowPitch), tileCols, tileRows,
                                                 nMasks, dValidBytes, dArena, offsets, sizes, maxZErr, arenaCapacity, slotBytes), arenaUsed);
}

lerc_status lerc_amd_decode_raster_tiles_device(lerc_amd_context* h, const unsigned char* dArena, const unsigned long long* offsets,
  const unsigned int* sizes, unsigned int dataType, int nCols, int nRows, int nBands, unsigned long long rowPitch, unsigned long long bandPitch,
  int tileCols, int tileRows, void* dRaster, int nMasks, unsigned char* dValidBytes, unsigned long long maskRowPitch)
{
  if (const lerc_status bad = rasterTilesArgs(h, dataType, nCols, nRows, tileCols, tileRows)) return bad;
  return decodeRasterTilesDevice(h->ctx, rasterTilesRequest(dRaster, dataType, nCols, nRows, nBands, planes(rowPitch, bandPitch, maskRowPitch), tileCols,
                                                            tileRows, nMasks, dValidBytes, dArena, offsets, sizes));
}

// ---- the same with a pixel pitch: line- and pixel-interleaved rasters (pixelPitch 1 and band-sequential: the calls above)
lerc_status lerc_amd_encode_raster_tiles_device_strided(lerc_amd_context* h, const void* dRaster, unsigned int dataType, int nCols, int nRows, int nBands,
  unsigned long long pixelPitch, unsigned long long rowPitch, unsigned long long bandPitch, int tileCols, int tileRows, int nMasks, const unsigned char* dValidBytes,
  unsigned long long maskRowPitch, double maxZErr, unsigned char* dArena, unsigned long long arenaCapacity, unsigned long long slotBytes,
  unsigned long long* offsets, unsigned int* sizes, unsigned long long* arenaUsed)
{
  if (arenaUsed) *arenaUsed = 0;
  if (const lerc_status bad = rasterTilesArgs(h, dataType, nCols, nRows, tileCols, tileRows)) return bad;
  return encodeRasterTiles(h, rasterTilesRequest(dRaster, dataType, nCols, nRows, nBands, strided(pixelPitch, rowPitch, bandPitch, maskRowPitch), tileCols,
                                                 tileRows, nMasks, dValidBytes, dArena, offsets, sizes, maxZErr, arenaCapacity, slotBytes), arenaUsed);
}

lerc_status lerc_amd_decode_raster_tiles_device_strided(lerc_amd_context* h, const unsigned char* dArena, const unsigned long long* offsets,
  const unsigned int* sizes, unsigned int dataType, int nCols, int nRows, int nBands, unsigned long long pixelPitch, unsigned long long rowPitch, unsigned long long bandPitch,
  int tileCols, int tileRows, void* dRaster, int nMasks, unsigned char* dValidBytes, unsigned long long maskRowPitch)
{
  if (const lerc_status bad = rasterTilesArgs(h, dataType, nCols, nRows, tileCols, tileRows)) return bad;
  return decodeRasterTilesDevice(h->ctx, rasterTilesRequest(dRaster, dataType, nCols, nRows, nBands, strided(pixelPitch, rowPitch, bandPitch, maskRowPitch),
                                                            tileCols, tileRows, nMasks, dValidBytes, dArena, offsets, sizes));
}

// ---- depth rasters, every tile one blob with the header's nDepth (lerc_amd_depth.h): the layouts are the driver's to check; the two
// calls without a depthPitch take packed pixels only and refuse every other description here
lerc_status lerc_amd_encode_raster_tiles_device_depth(lerc_amd_context* h, const void* dRaster, unsigned int dataType, int nCols, int nRows, int nDepth,
  unsigned long long pixelPitch, unsigned long long rowPitch, int tileCols, int tileRows, int nMasks, const unsigned char* dValidBytes,
  unsigned long long maskRowPitch, double maxZErr, unsigned char* dArena, unsigned long long arenaCapacity, unsigned long long slotBytes,
  unsigned long long* offsets, unsigned int* sizes, unsigned long long* arenaUsed)
{
  if (arenaUsed) *arenaUsed = 0;
  if (const lerc_status bad = rasterDepthArgs(h, dataType, nCols, nRows, nDepth, tileCols, tileRows, pixelPitch == (u64)nDepth)) return bad;
  return encodeRasterTiles(h, rasterDepthRequest(dRaster, dataType, nCols, nRows, nDepth, { pixelPitch, rowPitch, 1, maskRowPitch }, tileCols, tileRows, nMasks,
                                                 dValidBytes, dArena, offsets, sizes, maxZErr, arenaCapacity, slotBytes), arenaUsed);
}

lerc_status lerc_amd_decode_raster_tiles_device_depth(lerc_amd_context* h, const unsigned char* dArena, const unsigned long long* offsets,
  const unsigned int* sizes, unsigned int dataType, int nCols, int nRows, int nDepth, unsigned long long pixelPitch, unsigned long long rowPitch,
  int tileCols, int tileRows, void* dRaster, int nMasks, unsigned char* dValidBytes, unsigned long long maskRowPitch)
{
  if (const lerc_status bad = rasterDepthArgs(h, dataType, nCols, nRows, nDepth, tileCols, tileRows, pixelPitch == (u64)nDepth)) return bad;
  return decodeRasterTilesDevice(h->ctx, rasterDepthRequest(dRaster, dataType, nCols, nRows, nDepth, { pixelPitch, rowPitch, 1, maskRowPitch }, tileCols, tileRows,
                                                            nMasks, dValidBytes, dArena, offsets, sizes));
}

lerc_status lerc_amd_encode_raster_tiles_device_depth_strided(lerc_amd_context* h, const void* dRaster, unsigned int dataType, int nCols, int nRows,
  int nDepth, unsigned long long pixelPitch, unsigned long long rowPitch, unsigned long long depthPitch, int tileCols, int tileRows, int nMasks,
  const unsigned char* dValidBytes, unsigned long long maskRowPitch, double maxZErr, unsigned char* dArena, unsigned long long arenaCapacity,
  unsigned long long slotBytes, unsigned long long* offsets, unsigned int* sizes, unsigned long long* arenaUsed)
{
  if (arenaUsed) *arenaUsed = 0;
  if (const lerc_status bad = rasterDepthArgs(h, dataType, nCols, nRows, nDepth, tileCols, tileRows)) return bad;
  return encodeRasterTiles(h, rasterDepthRequest(dRaster, dataType, nCols, nRows, nDepth, { pixelPitch, rowPitch, depthPitch, maskRowPitch }, tileCols, tileRows,
                                                 nMasks, dValidBytes, dArena, offsets, sizes, maxZErr, arenaCapacity, slotBytes), arenaUsed);
}

lerc_status lerc_amd_decode_raster_tiles_device_depth_strided(lerc_amd_context* h, const unsigned char* dArena, const unsigned long long* offsets,
  const unsigned int* sizes, unsigned int dataType, int nCols, int nRows, int nDepth, unsigned long long pixelPitch, unsigned long long rowPitch,
  unsigned long long depthPitch, int tileCols, int tileRows, void* dRaster, int nMasks, unsigned char* dValidBytes, unsigned long long maskRowPitch)
{
  if (const lerc_status bad = rasterDepthArgs(h, dataType, nCols, nRows, nDepth, tileCols, tileRows)) return bad;
  return decodeRasterTilesDevice(h->ctx, rasterDepthRequest(dRaster, dataType, nCols, nRows, nDepth, { pixelPitch, rowPitch, depthPitch, maskRowPitch }, tileCols,
                                                            tileRows, nMasks, dValidBytes, dArena, offsets, sizes));
}

lerc_status lerc_amd_encode_raster_tiles_device_depth_range(lerc_amd_context* h, const void* dRaster, unsigned int dataType, int nCols, int nRows,
  int nDepth, unsigned long long pixelPitch, unsigned long long rowPitch, unsigned long long depthPitch, int tileCols, int tileRows, int tileCol0,
  int tileRow0, int nTileCols, int nTileRows, int nMasks, const unsigned char* dValidBytes, unsigned long long maskRowPitch, double maxZErr,
  unsigned char* dArena, unsigned long long arenaCapacity, unsigned long long slotBytes, unsigned long long* offsets, unsigned int* sizes,
  unsigned long long* arenaUsed)
{
  if (arenaUsed) *arenaUsed = 0;
  const bool rangeOk = !(tileCol0 < 0 || tileRow0 < 0 || nTileCols <= 0 || nTileRows <= 0);    // (inside the grid: the driver's check)
  if (const lerc_status bad = rasterDepthArgs(h, dataType, nCols, nRows, nDepth, tileCols, tileRows, rangeOk)) return bad;
  RasterTilesRequest rq = rasterDepthRequest(dRaster, dataType, nCols, nRows, nDepth, { pixelPitch, rowPitch, depthPitch, maskRowPitch }, tileCols, tileRows,
                                             nMasks, dValidBytes, dArena, offsets, sizes, maxZErr, arenaCapacity, slotBytes);
  rq.tileCol0 = tileCol0; rq.tileRow0 = tileRow0; rq.nTileCols = nTileCols; rq.nTileRows = nTileRows;
  return encodeRasterTiles(h, rq, arenaUsed);
}

lerc_status lerc_amd_decode_raster_window_device_depth(lerc_amd_context* h, const unsigned char* dArena, const unsigned long long* offsets,
  const unsigned int* sizes, unsigned int dataType, int nCols, int nRows, int nDepth, int tileCols, int tileRows, int winCol0, int winRow0,
  int winCols, int winRows, void* dWindow, unsigned long long pixelPitch, unsigned long long rowPitch, unsigned long long depthPitch, int nMasks,
  unsigned char* dValidBytes, unsigned long long maskRowPitch)
{
  if (const lerc_status bad = rasterDepthArgs(h, dataType, nCols, nRows, nDepth, tileCols, tileRows)) return bad;
  RasterWindow win;
  win.col0 = winCol0; win.row0 = winRow0; win.cols = winCols; win.rows = winRows;
  return decodeRasterWindowDevice(h->ctx, rasterDepthRequest(dWindow, dataType, nCols, nRows, nDepth, { pixelPitch, rowPitch, depthPitch, maskRowPitch }, tileCols,
                                                             tileRows, nMasks, dValidBytes, dArena, offsets, sizes), win);
}

// ---- a range of the grid's tiles coded, and a window of the mosaic decoded into a buffer of its own
lerc_status lerc_amd_encode_raster_tiles_device_range(lerc_amd_context* h, const void* dRaster, unsigned int dataType, int nCols, int nRows, int nBands,
  unsigned long long pixelPitch, unsigned long long rowPitch, unsigned long long bandPitch, int tileCols, int tileRows, int tileCol0, int tileRow0,
  int nTileCols, int nTileRows, int nMasks, const unsigned char* dValidBytes, unsigned long long maskRowPitch, double maxZErr, unsigned char* dArena,
  unsigned long long arenaCapacity, unsigned long long slotBytes, unsigned long long* offsets, unsigned int* sizes, unsigned long long* arenaUsed)
{
  if (arenaUsed) *arenaUsed = 0;
  const bool rangeOk = !(tileCol0 < 0 || tileRow0 < 0 || nTileCols <= 0 || nTileRows <= 0);    // (inside the grid: the driver's check)
  if (const lerc_status bad = rasterTilesArgs(h, dataType, nCols, nRows, tileCols, tileRows, rangeOk)) return bad;
  RasterTilesRequest rq = rasterTilesRequest(dRaster, dataType, nCols, nRows, nBands, strided(pixelPitch, rowPitch, bandPitch, maskRowPitch), tileCols,
                                             tileRows, nMasks, dValidBytes, dArena, offsets, sizes, maxZErr, arenaCapacity, slotBytes);
  rq.tileCol0 = tileCol0; rq.tileRow0 = tileRow0; rq.nTileCols = nTileCols; rq.nTileRows = nTileRows;
  return encodeRasterTiles(h, rq, arenaUsed);
}

lerc_status lerc_amd_decode_raster_window_device(lerc_amd_context* h, const unsigned char* dArena, const unsigned long long* offsets,
  const unsigned int* sizes, unsigned int dataType, int nCols, int nRows, int nBands, int tileCols, int tileRows, int winCol0, int winRow0,
  int winCols, int winRows, void* dWindow, unsigned long long pixelPitch, unsigned long long rowPitch, unsigned long long bandPitch, int nMasks,
  unsigned char* dValidBytes, unsigned long long maskRowPitch)
{
  if (const lerc_status bad = rasterTilesArgs(h, dataType, nCols, nRows, tileCols, tileRows)) return bad;
  RasterWindow win;
  win.col0 = winCol0; win.row0 = winRow0; win.cols = winCols; win.rows = winRows;
  return decodeRasterWindowDevice(h->ctx, rasterTilesRequest(dWindow, dataType, nCols, nRows, nBands, strided(pixelPitch, rowPitch, bandPitch, maskRowPitch),
                                                             tileCols, tileRows, nMasks, dValidBytes, dArena, offsets, sizes), win);
}

// ---- validity by a noData value (lerc_amd_nodata.h): one band staged with a mask of the cut's making; the value must be an element of
// the type, which is asked with the other arguments, before the size
lerc_status lerc_amd_encode_raster_tiles_device_nodata(lerc_amd_context* h, const void* dRaster, unsigned int dataType, int nCols, int nRows,
  unsigned long long pixelPitch, unsigned long long rowPitch, int tileCols, int tileRows, int tileCol0, int tileRow0, int nTileCols, int nTileRows,
  double noData, double maxZErr, unsigned char* dArena, unsigned long long arenaCapacity, unsigned long long slotBytes, unsigned long long* offsets,
  unsigned int* sizes, unsigned long long* arenaUsed)
{
  if (arenaUsed) *arenaUsed = 0;
  const bool whole = tileCol0 == 0 && tileRow0 == 0 && nTileCols == -1 && nTileRows == -1;
  const bool rangeOk = whole || !(tileCol0 < 0 || tileRow0 < 0 || nTileCols <= 0 || nTileRows <= 0);    // (inside the grid: the driver's check)
  if (const lerc_status bad = rasterTilesArgs(h, dataType, nCols, nRows, tileCols, tileRows, rangeOk && rasterNoDataOk((int)dataType, noData))) return bad;
  RasterTilesRequest rq = rasterTilesRequest(dRaster, dataType, nCols, nRows, 1, strided(pixelPitch, rowPitch, 0, 0), tileCols, tileRows, 1, nullptr, dArena,
                                             offsets, sizes, maxZErr, arenaCapacity, slotBytes);
  rq.tileCol0 = tileCol0; rq.tileRow0 = tileRow0; rq.nTileCols = nTileCols; rq.nTileRows = nTileRows;
  rq.useNoData = true; rq.noData = noData;
  return encodeRasterTiles(h, rq, arenaUsed);
}

lerc_status lerc_amd_decode_raster_window_device_nodata(lerc_amd_context* h, const unsigned char* dArena, const unsigned long long* offsets,
  const unsigned int* sizes, unsigned int dataType, int nCols, int nRows, int tileCols, int tileRows, int winCol0, int winRow0, int winCols,
  int winRows, void* dWindow, unsigned long long pixelPitch, unsigned long long rowPitch, double noData, unsigned char* dValidBytes,
  unsigned long long maskRowPitch)
{
  if (const lerc_status bad = rasterTilesArgs(h, dataType, nCols, nRows, tileCols, tileRows, rasterNoDataOk((int)dataType, noData))) return bad;
  RasterWindow win;
  win.col0 = winCol0; win.row0 = winRow0; win.cols = winCols; win.rows = winRows;
  RasterTilesRequest rq = rasterTilesRequest(dWindow, dataType, nCols, nRows, 1, strided(pixelPitch, rowPitch, 0, maskRowPitch), tileCols, tileRows, 1,
                                             dValidBytes, dArena, offsets, sizes);
  rq.useNoData = true; rq.noData = noData;
  return decodeRasterWindowDevice(h->ctx, rq, win);
}

void lerc_amd_raster_tiles_counters(lerc_amd_context* h, unsigned long long out[4])
{
  readCounters(h, [](Context& c) -> Counters { return c.rasterTilesCount; }, out);
}

void lerc_amd_profile_enable(lerc_amd_context* h, int on) { if (h) h->ctx.profEnable(on != 0); }

int lerc_amd_profile_read(lerc_amd_context* h, char* buf, int cap, int reset)
{
  if (!h || !buf || cap <= 0) return -1;
  const std::string r = h->ctx.profReport(reset != 0);
  const int n = (int)std::min<size_t>(r.size(), (size_t)cap - 1);
  memcpy(buf, r.data(), n);
  buf[n] = 0;
  return n;
}

const char* lerc_amd_last_note(lerc_amd_context* h)
{
  h = orThisThreads(h);
  return h ? h->ctx.lastNote.c_str() : "";
}

void lerc_amd_path_counters(lerc_amd_context* h, unsigned long long out[4])
{
  readCounters(orThisThreads(h), [](Context& c) -> Counters { return c.pathCount; }, out);
}

void lerc_amd_decode_forms(lerc_amd_context* h, unsigned long long out[4])
{
  readCounters(orThisThreads(h), [](Context& c) -> Counters { return c.tiers.formCount; }, out);
}

unsigned int lerc_amd_gather_blobs(lerc_amd_context* h, void* ncclComm, int root, const void* dMessage, unsigned long long nBytes,
                                   void* dRootBuffer, unsigned long long rootCapacity, unsigned long long* hLengths, unsigned long long* hOffsets,
                                   void* stream)
{
  if (!h || !ncclComm) return kWrongParam;
  std::string err;
  const u32 rc = gatherBlobsRccl(ncclComm, root, dMessage, nBytes, dRootBuffer, rootCapacity, (u64*)hLengths, (u64*)hOffsets, (hipStream_t)stream, err);
  if (rc != kOk) h->ctx.lastError = err;
  return rc;
}

void lerc_amd_decode_refusals(lerc_amd_context* h, unsigned long long out[4])
{
  readCounters(orThisThreads(h), [](Context& c) -> Counters { return c.tiers.refusalCount; }, out);
}

unsigned int lerc_amd_mask_rle_device(lerc_amd_context* h, const unsigned char* dBits, unsigned int nBytes, unsigned char* dOut,
                                      unsigned int cap, unsigned int* size)
{
  if (!h || !dBits || !dOut || !size || nBytes == 0 || ((uintptr_t)dBits & 15)) return kWrongParam;
  Context& ctx = h->ctx;
  ctx.reset();
  if (!ctx.reserve(maskRleScratchBytes(nBytes) + 4096)) return kFailed;
  u8* scratch = ctx.allocT<u8>(maskRleScratchBytes(nBytes));
  u32* dSize = ctx.allocT<u32>(4);
  u32* pin = (u32*)ctx.pinned(64);
  if (!scratch || !dSize || !pin) return kFailed;
  launchMaskRle(dBits, nBytes, dOut, cap, dSize, scratch, ctx.activeStream());
  hipMemcpyAsync(pin, dSize, 4, hipMemcpyDeviceToHost, ctx.activeStream());
  if (!ctx.sync()) return kFailed;
  if (pin[0] == 0xFFFFFFFFu) return kBufferTooSmall;
  *size = pin[0];
  return kOk;
}

unsigned int lerc_amd_mask_rle_decode_device(lerc_amd_context* h, const unsigned char* dRle, unsigned int rleBytes, unsigned char* dBits,
                                             unsigned int nBytes)
{
  if (!h || !dRle || !dBits || rleBytes < 2 || nBytes == 0) return kWrongParam;
  Context& ctx = h->ctx;
  ctx.reset();
  const size_t need = maskRleDecodeScratchBytes(rleBytes);
  if (!ctx.reserve(need + 4096)) return kFailed;
  u8* scratch = ctx.allocT<u8>(need);
  DeviceStatus* dStatus = reinterpret_cast<DeviceStatus*>(ctx.allocT<u8>(64));
  DeviceStatus* pin = (DeviceStatus*)ctx.pinned(64);
  if (!scratch || !dStatus || !pin) return kFailed;
  hipMemsetAsync(dStatus, 0, 64, ctx.activeStream());
  launchMaskRleDecode(dRle, rleBytes, dBits, nBytes, scratch, dStatus, ctx.activeStream());
  hipMemcpyAsync(pin, dStatus, sizeof(DeviceStatus), hipMemcpyDeviceToHost, ctx.activeStream());
  if (!ctx.sync()) return kFailed;
  return pin->error ? pin->error : kOk;
}

const char* lerc_amd_build_info(void)
{
#ifdef HIPSIM
  return "lerc_amd 0.1 hipsim (CPU SIMT emulator -- test build, not the product)";
#else
  return "lerc_amd 0.1 gfx950 hip";
#endif
}

}    // extern "C"
