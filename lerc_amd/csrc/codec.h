// codec.h -- host side of the MI355X LERC path: per-call context, header / mask / mode-decision logic
// and the kernel pipelines behind lerc_encode() / lerc_decode().
//
// Reference counterparts: Lerc::EncodeInternal (Lerc.cpp:628-789), Lerc::DecodeTempl (:397-521),
// Lerc2::ComputeNumBytesNeededToWrite (Lerc2.cpp:179-381), Lerc2::Encode (:396-480), Lerc2::Decode
// (:577-694).  Pixel-touching work is never done here: it is enqueued as HIP kernels (kernels.h).
#pragma once
#include "kernels.h"

#include <string>
#include <functional>
#include <vector>

namespace lerc {

// Lerc2::HeaderInfo (Lerc2.h:102-131)
struct Header
{
  int version = kCodecVersion;
  u32 checksum = 0;
  int nRows = 0, nCols = 0, nDepth = 1, numValid = 0, mbSize = 8, blobSize = 0, dt = DT_Undefined, nBlobsMore = 0;
  u8 passNoData = 0, isInt = 0, rsv3 = 0, rsv4 = 0;
  double maxZErr = 0, zMin = 0, zMax = 0, noDataVal = 0, noDataValOrig = 0;
  bool tryHuffmanInt() const { return version >= 2 && (dt == DT_Byte || dt == DT_Char) && maxZErr == 0.5; }
  bool tryHuffmanFlt() const { return version >= 6 && (dt == DT_Float || dt == DT_Double) && maxZErr == 0; }
};
u32 headerBytes(int version);
void writeHeader(u8* dst, const Header& h);
bool readHeader(const u8* src, size_t n, Header& h, size_t& used);

// RLE of the validity bit mask (host; the mask is << 1 % of the bytes and inherently sequential)
void rleEncode(const u8* src, size_t n, std::vector<u8>& out);
bool rleEncodeWhenReady(const u8* b, size_t n, const std::function<bool()>& ready, std::vector<u8>& out);    // (pieces by several threads, started before the bytes are there)
bool rleDecode(const u8* src, size_t n, u8* dst, size_t dstSize, size_t* written = nullptr);    // (what the stream does not fill stays as it was)

// ---- which decoder takes a band (codec_decode.cpp holds the rules; DESIGN.md 4.2c states them in one place)
// The streaming forms, fastest first; each follows streams the one above it cannot, and every one checks what it decodes, so a
// wrong choice costs launches, never pixels.  (DecodeRequest::maxForm and lerc_amd_decode_forms speak in these numbers.)
enum DecodeForm : int
{
  kFormGeneral = 0,      // no streaming kernels: header read on the host, general discovery
  kFormTwoLaunch = 1,    // discovery + decode as two launches over chunks of 2 KiB (tile_fast_decode.hip)
  kFormWalk = 2,         // the walking one-launch decoder (tile_fast_decode_one.hip)
  kFormScan = 3,         // the scanning decoder, counts late (tile_fast_decode_scan.hip)
  kFormScanEarly = 4     // the scanning decoder with early counts
};

struct RasterShape
{
  int dt = -1, nRows = 0, nCols = 0;    // dt < 0: of any type
  bool covers(const RasterShape& o) const { return nRows == o.nRows && nCols == o.nCols && (dt < 0 || dt == o.dt); }
};

// "The next n decodes of shape S do X": the bands of one job are alike, another job's are not.
struct ShapeWindow
{
  RasterShape shape;
  u32 n = 0;    // calls left (the size guess: the bytes; 0: nothing is remembered)
  void open(const RasterShape& s, u32 count) { shape = s; n = count; }
  bool holds(const RasterShape& s) const { return n > 0 && shape.covers(s); }
  bool take(const RasterShape& s) { if (!holds(s)) return false; n--; return true; }    // one call of the window used up
};

// What one launch of the streaming decoders was, kept by whoever waits for its verdict (several may be in flight on a stream):
// a verdict is judged against this, never against what the context enqueued last.
struct StreamTicket
{
  int form = kFormGeneral;
  u32 epoch = 0;            // the value the launch's flags are raised with (tile_fast.h)
  RasterShape shape;
  u32 gridBytes = 0;        // blob bytes the scanning decoder's launch held pieces for (0: not that decoder)
};

// The tier memory of a context.  pick / below choose, judge is the only place that turns a verdict into memory and counters.
struct DecodeTiers
{
  ShapeWindow offScan;      // keep off the scanning decoder: it has just handed a band of that shape on (kScanSkip calls, any type)
  ShapeWindow countLate;    // the scanning decoder counts late: an early count was wrong (lateSpan calls, any type)
  ShapeWindow notBlind;     // go to the header-reading path at once: the header refused the last blind attempt (8 calls)
  ShapeWindow sizeGuess;    // n = bytes of the last band of that shape the streaming kernels decoded (launchFastBands sizes a launch by it)
  static constexpr u32 kScanSkip = 16, kScanLate = 64, kScanLateMax = 4096, kBlindSkip = 8;    // how long the windows are
  u32 lateSpan = kScanLate; // what the next wrong early count opens countLate with (grows: 64, 256, ... 4096)
  unsigned long long formCount[4] = { 0, 0, 0, 0 };       // lerc_amd_decode_forms: [0] masked bands whose blocks the scan found, [1 .. 3] bands / tiles decoded by that form (4 counts as 3)
  unsigned long long refusalCount[4] = { 0, 0, 0, 0 };    // attempts thrown away (lerc_amd_decode_refusals): [0] the decode kernels refused the masked scan's block offsets, [1] the masked scan handed a band on, [2] a streaming decode tier handed a band on, [3] unused

  int pick(int maxForm, const RasterShape& s);    // the form a request starts with: the highest one <= maxForm that is switched on, takes the raster and is not kept off by a window
  int below(int form, const RasterShape& s) { return form > kFormTwoLaunch ? pick(form - 1, s) : kFormGeneral; }    // ... after `form` has refused
  // a single band's verdict (fastBandVerdict; blobEnd: the band's size by its header).  true: decoded, checksum good
  bool judge(const StreamTicket& t, u32 verdict, u32 blobEnd);
  // a batch's: tiles served, and whether so many went on that the form is not for these tiles (the caller's trigger)
  void judgeBatch(const StreamTicket& t, u32 nServed, bool manyWentOn);
private:
  void handedOn(const StreamTicket& t);
};

// ---- growable device workspace + stream, one per host thread (C API) or per handle (device API)
class Context
{
public:
  Context();
  ~Context();
  bool ok() const { return m_ok; }
  hipStream_t stream() const { return m_stream; }
  // a caller-provided stream; nullptr means the HIP default (NULL) stream, exactly like a HIP API call would
  void setStream(hipStream_t s) { m_userStream = s; m_userSet = true; }
  hipStream_t activeStream() const { return m_userSet ? m_userStream : m_stream; }

  // bump allocation out of one device slab; reserve() may re-allocate (invalidates earlier pointers)
  bool reserve(size_t bytes);
  void poisonScratch(size_t bytes);          // test aid, see codec_common.cpp
  void reset() { m_used = 0; }
  size_t used() const { return m_used; }
  void rewind(size_t mark) { m_used = mark; }    // gives back everything allocated since used() returned mark
  void* alloc(size_t bytes, size_t align = 256);
  template<class T> T* allocT(size_t n) { return (T*)alloc(n * sizeof(T)); }

  // small pinned host mirror for results read back after a sync
  void* pinned(size_t bytes);
  // pinned result slots of operations that are enqueued but not waited for yet (asynchronous device API)
  static const int kAsyncSlots = 64;
  static const size_t kAsyncSlotBytes = 512;
  u8* asyncSlot(unsigned ticket);
  // a second pinned area (the validity bits of a band on their way to the host while kernels run) and its event
  void* pinnedAux(size_t bytes);
  hipEvent_t auxEvent();
  // a stream beside the active one for that copy (it branches off behind what is enqueued so far: forkSide()); nullptr: none to be had
  hipStream_t forkSide();
  // more work has gone onto that stream since the last sync(): the next sync() / reset() waits for it again
  void sideInUse() { if (m_sideStream) m_sideUsed = true; }
  bool sync();                               // wait for the active stream (polls first: see codec_common.cpp)
  // Device memory that keeps its contents from call to call (the two-launch encoder's arrival counters and cells,
  // tile_fast.h): zero when handed out for the first time and whenever it had to grow.  Two areas: [0] counters, which the
  // kernels leave zero, and [1] cells tagged with the call's epoch, which they leave as they are.
  u8* persistentState(int area, size_t bytes);
  // after a kernel has reported a hand-off it gave up on ("stuck"): late workgroups may have left residue in the counters,
  // so both areas are wiped (after waiting for the stream) before the next call uses them
  void wipePersistentState();
  // a value no earlier call of this context has used and that no fill pattern looks like: kernels raise flags by
  // writing it into cells that are never cleared (tile_fast.h)
  // the raster tile calls' staging buffer (codec_raster_tiles.cpp): outside the bump workspace, which the tile batches reset per
  // sub-batch; grows on demand (contents are not kept), freed with the context
  u8* rasterStage(size_t bytes);
  u32 nextEpoch() { m_epoch += 0x9E3779B9u; if ((m_epoch & 0xFFFFu) == (m_epoch >> 16) || m_epoch == 0u) m_epoch += 0x9E3779B9u; return m_epoch; }

  std::string lastError;
  std::string lastNote;      // diagnostics that are not errors (why a call left the streaming path)

  // which kernels served the calls so far: [0] encode streaming, [1] encode general, [2] decode streaming, [3] decode general
  unsigned long long pathCount[4] = { 0, 0, 0, 0 };
  unsigned long long tileBatchCount[4] = { 0, 0, 0, 0 };    // tiles of batch calls (lerc_amd_tile_batch_counters): [0] encoded by the batch's own launches, [1] encoded one by one behind it, [2] / [3] the same for decodes
  unsigned long long rasterTilesCount[4] = { 0, 0, 0, 0 };  // tiles of the raster tile calls (lerc_amd_raster_tiles_counters): [0] cut through the staging buffer, [1] encoded where they lie, [2] pasted from the staging buffer, [3] decoded where they lie
  bool lastDecodeStreamed = false;
  DecodeTiers tiers;                   // which streaming decoder a band starts with, and the counters of what became of it
  bool scanOffsetsBan = false;         // this call: a masked band's scan for block offsets has failed, the general discovery takes the bands

  // optional per-kernel timing with HIP events on the active stream (bench.py: roofline of the dominant kernel)
  void profEnable(bool on) { m_prof = on; }
  bool profOn() const { return m_prof; }
  void profBegin(const char* name);
  void profEnd();
  void profCollect();                        // call after a stream sync
  std::string profReport(bool reset);        // "name total_ms launches" per line

private:
  struct ProfEntry { const char* name; hipEvent_t a, b; bool ownsA, ownsB; };
  bool m_lastEndFresh = false;               // nothing was enqueued since the last profEnd()
  struct ProfAcc { std::string name; double ms; int n; };
  bool m_prof = false;
  std::vector<ProfEntry> m_pending;
  std::vector<hipEvent_t> m_eventPool;
  std::vector<ProfAcc> m_acc;
  hipEvent_t profEvent();

  u8* m_asyncPinned = nullptr;
  u8* m_state[2] = { nullptr, nullptr };
  size_t m_stateCap[2] = { 0, 0 };
  unsigned long long m_stateCalls = 0;
  bool m_ok = false;
  u32 m_epoch = 0x1234567u;
  hipStream_t m_stream = nullptr, m_userStream = nullptr;
  bool m_userSet = false;
  u8* m_slab = nullptr;
  u8* m_rasterStage = nullptr;
  size_t m_rasterStageCap = 0;
  size_t m_cap = 0, m_used = 0;
  void* m_pinned = nullptr;
  size_t m_pinnedCap = 0;
  void* m_pinnedAux = nullptr;
  size_t m_pinnedAuxCap = 0;
  hipEvent_t m_auxEvent = nullptr, m_forkEvent = nullptr;
  hipStream_t m_sideStream = nullptr;
  bool m_sideUsed = false;
};

// RAII bracket around one kernel launch (or a short group of launches)
struct ProfScope
{
  Context& c;
  ProfScope(Context& ctx, const char* name) : c(ctx) { if (c.profOn()) c.profBegin(name); }
  ~ProfScope() { if (c.profOn()) c.profEnd(); }
};

// the mosaic job's exchange step over RCCL (gather_rccl.cpp)
u32 gatherBlobsRccl(void* comm, int root, const void* dMessage, u64 nBytes, void* dRootBuffer, u64 rootCapacity, u64* hLengths, u64* hOffsets,
                    hipStream_t st, std::string& err);

// ---- whole-call entry points on DEVICE-resident pixel data -------------------------------------
struct EncodeRequest
{
  const void* dData = nullptr;        // device: [nBands][nRows][nCols][nDepth]
  const u8* dValidBytes = nullptr;    // device byte masks (nMasks of them) or nullptr
  int dt = DT_Undefined, nDepth = 1, nCols = 0, nRows = 0, nBands = 1, nMasks = 0;
  double maxZErr = 0;
  u8* dOut = nullptr;                 // device output buffer (nullptr: size only)
  u32 outCapacity = 0;
  const u8* hUsesNoData = nullptr;    // host [nBands] or nullptr: band carries a noData value (lerc_encode_4D)
  const double* hNoDataValues = nullptr;
  int version = kCodecVersion;        // codec version of the blobs to write: 3..6 (lerc_encodeForVersion)
};
// returns an ErrCode; numBytesNeeded is always the exact blob size on kOk
u32 encodeDevice(Context& ctx, const EncodeRequest& rq, u32& numBytesNeeded, u32& numBytesWritten);

// nTiles rasters of one shape, contiguous on the device, each to become (or coming from) its own blob in an arena
struct TilesEncodeRequest
{
  const void* dData = nullptr;        // device: [nTiles][nRows][nCols]
  int dt = 0, nCols = 0, nRows = 0, nTiles = 0;
  double maxZErr = 0;
  u8* dArena = nullptr;               // device
  u64 arenaCapacity = 0;
  u64* hOffsets = nullptr;            // host [nTiles]: where tile t's blob starts in the arena (16-byte aligned)
  u32* hSizes = nullptr;              // host [nTiles]
  u64 slotBytes = 0;                  // != 0: tile t's blob goes to dArena + t * slotBytes (a multiple of 16), nothing is moved afterwards
  const u8* dValidBytes = nullptr;    // device [nTiles][nRows][nCols], 0 = invalid: a mask per tile (encodeTilesDeviceMasked); nullptr: every pixel valid
  // band stacks (encodeTilesDeviceBands): dData [nTiles][nBands][nRows][nCols], dValidBytes [nTiles][nMasks][nRows][nCols]; nMasks < 0: the
  // single-band calls' meaning (a mask per tile where the call takes masks)
  int nBands = 1, nMasks = -1;
  int nDepth = 1;                     // depth tiles (encodeTilesDeviceDepth): dData [nTiles][nRows][nCols][nDepth], one blob with nDepth a tile
};
struct TilesDecodeRequest
{
  const u8* dArena = nullptr;         // device
  const u64* hOffsets = nullptr;      // host [nTiles]
  const u32* hSizes = nullptr;        // host [nTiles]
  int dt = 0, nCols = 0, nRows = 0, nTiles = 0;
  void* dOut = nullptr;               // device: [nTiles][nRows][nCols]
  u8* dValidBytes = nullptr;          // device [nTiles][nRows][nCols], written 1 / 0 for every tile (decodeTilesDeviceMasked); nullptr: blobs with a mask are refused
  int nBands = 1, nMasks = -1;        // band stacks (decodeTilesDeviceBands), as in TilesEncodeRequest
  int nDepth = 1;                     // depth tiles (decodeTilesDeviceDepth): dOut [nTiles][nRows][nCols][nDepth]
};

struct DecodeRequest
{
  const u8* hBlob = nullptr;          // host copy of the blob (may be nullptr when only dBlob is known)
  const u8* dBlob = nullptr;          // device copy of the blob (nullptr: staged from hBlob)
  u32 blobSize = 0;
  int dt = DT_Undefined, nDepth = 1, nCols = 0, nRows = 0, nBands = 1, nMasks = 0;
  void* dOut = nullptr;               // device: decoded pixels
  u8* dValidBytes = nullptr;          // device: nMasks byte masks, or nullptr
  bool noStreaming = false;            // go straight to the general kernels (a batch has already tried the streaming ones)
  int maxForm = kFormScanEarly;        // the first streaming form to try (DecodeForm)
  void startAt(int form) { maxForm = form; noStreaming = form <= kFormGeneral; }    // (DecodeTiers::below of the form that has just refused this blob)
  u8* hUsesNoData = nullptr;           // host [nBands] out (lerc_decode_4D), or nullptr
  double* hNoDataValues = nullptr;
};
u32 decodeDevice(Context& ctx, const DecodeRequest& rq);

// ---- the general band path (codec_encode_band.cpp, codec_decode_band.cpp): every call the streaming kernels do not take blind
u32 encodeBands(Context& ctx, const EncodeRequest& rq, u32& numBytesNeeded, u32& numBytesWritten);    // band after band (BandEncoder)
// (fastLevel: the streaming form where a band qualifies, DecodeForm; fellBack: a streaming form handed a band on, the caller repeats one tier down)
u32 decodeBands(Context& ctx, const DecodeRequest& rq, int fastLevel, bool& fellBack);
bool fastEncodeOneLaunch();    // LERC_AMD_ENCODE_LAUNCHES=2 keeps the two-launch form for a single raster (codec_encode.cpp)
// a band's result cell of the streaming decoders (codec_decode.cpp; device, zeroed before the launches, copied back in one piece):
//   [FastDecodeParams, 128 B reserved][fallback bits 16 B][pad to 192]
constexpr size_t kCellParams = 0, kCellFallback = 128, kCellBytes = 192;
size_t fastBandWorkspace(int nRows, int nCols, u32 sizeGiven, u32 nTiles = 1);
bool launchFastBand(Context& ctx, StreamTicket& t, const u8* dBand, u32 sizeGiven, void* dOutBand, u8* dCell, u8* hCell = nullptr);
u32 fastFlagBits(const u32* cells, u32 epoch);    // reason bits of a tile's / band's four epoch tagged flag cells
u32 fastBandVerdict(const u8* hCell, u32 epoch, u32* blobEnd = nullptr);    // 0 = decoded and checksum good, else the reason bits (tile_fast.h: kVerdict...)

// ---- small pieces both directions share (codec_common.cpp)
// masks of this many bytes or more are run-length coded / decoded on the device (rle_kernels.hip); LERC_AMD_DEVICE_RLE=0: never,
// =<bytes>: from masks of that many bytes on -- a test knob; default: 256 KB, as for the helper threads
size_t deviceRleFrom();
// valid pixels in front of every group of 32 (dBase[nGroups]: all of them): three allocations, two launches; nullptr: no room
u32* enqueueMaskCount(Context& ctx, const u8* dBits, i64 nPix, hipStream_t st);
// one sweep under a mask: the count above, then k_one_sweep packs (src: pixels, dst: stream) or unpacks the valid pixels
bool enqueueMaskedOneSweep(Context& ctx, bool pack, const u8* src, u8* dst, const u8* dBits, i64 nPix, int bytesPerPixel, hipStream_t st);
// what every user of the block kernels fills alike; callers set intLossless, tryDiff, zMaxHdr, checkOverflow where they differ from 0
BandParams makeBandParams(int dt, int nRows, int nCols, int nD, int version, int mb, double maxZErr, bool allValid);
// what the streaming encode kernels assume of a raster they take blind (codec_encode.cpp): one band of codec 6, every pixel valid, 8 x 8
// blocks, the error bound as Lerc2 rounds it for integer types; and the TryRaiseMaxZError candidates worth a look, bit c = candidate c
BandParams fastBandParams(int dt, int nRows, int nCols, double maxZErr);
u32 raiseCandidates(int dt, double maxZErr);

// The same two calls in two halves, for callers that keep several operations in flight on the stream (the asynchronous
// device API, capi.cpp): the enqueue half puts the streaming kernels and the copy of their verdict into `slot` (pinned,
// Context::kAsyncSlotBytes) on the stream and returns true -- or false when the request is not one the streaming kernels
// take blind (then nothing was enqueued); the verdict half is called once the stream has passed that point.
bool encodeEnqueueStreaming(Context& ctx, const EncodeRequest& rq, u8* slot);
// redo: the general path has to repeat the request; else status / sizes are final
void encodeStreamingVerdict(Context& ctx, const EncodeRequest& rq, const u8* slot, bool& redo, u32& status, u32& numBytesNeeded, u32& numBytesWritten);
bool decodeEnqueueStreaming(Context& ctx, const DecodeRequest& rq, u8* slot, StreamTicket& ticket);
bool decodeStreamingVerdict(Context& ctx, const u8* slot, const StreamTicket& ticket, u32* bits = nullptr);    // true: decoded, checksum good (bits: why not)
// may a host-pointer decode go through decodeSpeculativeToHost?  hd: the blob's first header; rq: the call (shape, type, blobSize, noData arrays)
bool speculativeDecodeEligible(const Header& hd, const DecodeRequest& rq);
// host-pointer calls: streaming kernels + the results' way back to the host enqueued together, one wait (rq holds a device copy of the blob)
u32 decodeSpeculativeToHost(Context& ctx, const DecodeRequest& rq, void* hOut, size_t outBytes, u8* hMask, size_t maskBytes, bool& handled, StreamTicket& ticket);    // ticket.form > 0: the streaming kernels were enqueued (and may have written pixels)
u32 encodeTilesDevice(Context& ctx, const TilesEncodeRequest& rq, u64& arenaUsed);
u32 decodeTilesDevice(Context& ctx, const TilesDecodeRequest& rq);
// the same with a validity mask per tile (codec_tiles_batch.cpp, tile_mask_batch.hip); without mask pointers they ARE the two calls above
u32 encodeTilesDeviceMasked(Context& ctx, const TilesEncodeRequest& rq, u64& arenaUsed);
u32 decodeTilesDeviceMasked(Context& ctx, const TilesDecodeRequest& rq);
// tiles that are band stacks, one blob a tile (codec_tiles_batch.cpp); with one band they ARE the calls above
u32 encodeTilesDeviceBands(Context& ctx, const TilesEncodeRequest& rq, u64& arenaUsed);
u32 decodeTilesDeviceBands(Context& ctx, const TilesDecodeRequest& rq);
// depth tiles: [nTiles][nRows][nCols][nDepth], a mask [nRows][nCols] per tile or none, one blob with the header's nDepth a tile
u32 encodeTilesDeviceDepth(Context& ctx, const TilesEncodeRequest& rq, u64& arenaUsed);
u32 decodeTilesDeviceDepth(Context& ctx, const TilesDecodeRequest& rq);

// 8-bit tiles, every pixel valid, lossless (codec_tiles_batch.cpp, tile_byte_batch.hip): encodeTilesDevice / decodeTilesDevice hand such requests on
bool tilesBytesEncodeEligible(const TilesEncodeRequest& rq);
bool tilesBytesDecodeEligible(const TilesDecodeRequest& rq);
u32 encodeTilesBytes(Context& ctx, const TilesEncodeRequest& rq, u64& arenaUsed);
u32 decodeTilesBytes(Context& ctx, const TilesDecodeRequest& rq);

// ---- a pitched device raster cut into a grid of tiles, every tile a blob (codec_raster_tiles.cpp, raster_tiles.hip): per shape class
// of the grid (interior, right column, bottom row, corner) the tiles are staged as [n][nBands][r][c] and handed to the calls above
struct RasterTilesRequest
{
  void* dRaster = nullptr;            // device: nBands planes of nRows rows, pitched (encode: read only)
  u8* dValidBytes = nullptr;          // device: one byte mask [nRows][maskRowPitch] for the raster (nMasks == 1), or nullptr
  int dt = 0, nCols = 0, nRows = 0, nBands = 1, nMasks = 0, tileCols = 0, tileRows = 0;
  u64 rowPitch = 0, bandPitch = 0, maskRowPitch = 0;    // in elements
  u64 pixelPitch = 1;                 // elements from column to column: 1 planes (band-sequential, or line-interleaved), >= 2 pixel-interleaved (bandPitch 1)
  bool anyLayout = false;             // the _strided entry points: line- and pixel-interleaved descriptions are admitted
  u8* dArena = nullptr;               // device (decode: read only)
  u64* hOffsets = nullptr;            // host [nTY * nTX], tile (ty, tx) at ty * nTX + tx
  u32* hSizes = nullptr;
  // encode only
  double maxZErr = 0;
  u64 arenaCapacity = 0, slotBytes = 0;
  // the tiles of the grid the call is about, [tileRow0, tileRow0 + nTileRows) x [tileCol0, tileCol0 + nTileCols); a negative count: all
  // from the first on (the default: the whole grid).  hOffsets / hSizes stay full-grid tables, only the range's entries are touched
  int tileCol0 = 0, tileRow0 = 0, nTileCols = -1, nTileRows = -1;
  // depth tiles (the _depth entry points): > 1: one band (nBands 1) whose element (row, col, d) lies at row * rowPitch + col * pixelPitch
  // + d * depthPitch, in one of the four layouts of lerc_amd_depth.h -- packed or gapped pixels (depthPitch 1), planes or lines
  // (pixelPitch 1) --; every tile is one blob with the header's nDepth.  nDepth 1: depthPitch is not looked at
  int nDepth = 1;
  u64 depthPitch = 1;
  // validity by value (the _nodata entry points, lerc_amd_nodata.h): one band, nDepth 1, staged as nMasks 1 -- the mask is made by the
  // cut (a pixel is invalid when it equals (T)noData, or is a NaN where noData is NaN) and consumed by the paste, which writes noData
  // at invalid pixels; dValidBytes: encode NULL, decode the window's valid bytes or NULL.  noData is exactly representable in the type
  bool useNoData = false;
  double noData = 0;
};
// whether noData is an element of type dt: (double)(T)noData == noData, or NaN for the two float types
bool rasterNoDataOk(int dt, double noData);
u32 encodeRasterTilesDevice(Context& ctx, const RasterTilesRequest& rq, u64& arenaUsed);
u32 decodeRasterTilesDevice(Context& ctx, const RasterTilesRequest& rq);
// A window of the mosaic, in raster coordinates.  decodeRasterWindowDevice: rq describes the mosaic (nCols, nRows, the tile sizes, the
// full-grid tables) and, with dRaster, the pitches and dValidBytes / maskRowPitch, the DESTINATION, which holds the window only; the
// tiles the window touches are decoded, through the staging buffer always, and pasted clipped (raster_window.hip)
struct RasterWindow { int col0 = 0, row0 = 0, cols = 0, rows = 0; };
u32 decodeRasterWindowDevice(Context& ctx, const RasterTilesRequest& rq, const RasterWindow& win);

// header-only queries (host)
struct BlobInfo
{
  int version = 0, nDepth = 0, nCols = 0, nRows = 0, numValid = 0, nBands = 0, nMasks = 0, nUsesNoData = 0, dt = 0;
  u32 blobSize = 0;
  double zMin = 0, zMax = 0, maxZErr = 0;
};
u32 getBlobInfo(const u8* blob, u32 n, BlobInfo& info, double* mins = nullptr, double* maxs = nullptr, size_t nElem = 0);

// reads small pieces of a blob that lives on the host, the device, or both (codec_decode_band.cpp)
struct BlobReader
{
  const u8* h;
  const u8* d;
  u32 n;
  hipStream_t st;
  // bytes already fetched (the head of the current band): served without another device round trip
  const u8* cache = nullptr;
  u64 cacheOff = 0;
  size_t cacheLen = 0;
  Context* ctx = nullptr;    // small device reads go through its pinned mirror (a pageable target costs a staging copy)
  bool read(u64 off, size_t len, u8* dst) const;
};
struct BandDesc
{
  u64 offset = 0;
  Header hd;
  size_t hdrLen = 0;
  int numBytesMask = 0;
  u8 head[2048];         // first bytes of the band (header, and for unmasked bands ranges + mode bytes + a Huffman code table)
  size_t headLen = 0;
};
// The chain of band headers (Lerc::GetLercInfo, Lerc.cpp:92-182): kOk with every band that is there; kFailed where the first is no
// Lerc2 header (bands stays empty), does not fit blobSize (bands holds it alone), or a later one is of another shape or does not fit
u32 walkBands(const BlobReader& rd, u32 blobSize, std::vector<BandDesc>& bands);
int bandsMaskCount(const std::vector<BandDesc>& bands);    // how many masks a caller must have room for: 0, 1 or one per band

// legacy Lerc1 ("CntZImage") blobs: decode only, on the device (lerc1_host.cpp)
bool isLerc1(const u8* hBlob, u32 n);
u32 decodeLerc1(Context& ctx, const DecodeRequest& rq);
u32 lerc1BlobInfo(Context& ctx, const u8* hBlob, u32 n, BlobInfo& info, double* mins, double* maxs, size_t nElem);

}    // namespace lerc
