// check_capi_boundary.cpp -- the C boundary (lerc_amd/csrc/capi.cpp) under the host sanitizers: refused calls of every call family
// (a pointer nulled, counts at 0 and -1, dataType 8, maxZErr -1, the slot and mask rules, dimensions beyond INT_MAX) and a handful of
// valid ones, through the C symbols, on the emulator build's sources compiled with -fsanitize=address,undefined
// (make -C lerc_amd/csrc boundary).  Host code only; the statuses are those of tests/capi_boundary_common.py's table.
#include "../include/lerc_amd.h"
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

static int failures = 0;
#define EXPECT(call, want) do { const unsigned got_ = (call); if (got_ != (unsigned)(want)) { failures++; printf("line %d: %u, expected %u\n", __LINE__, got_, (unsigned)(want)); } } while (0)

int main()
{
  typedef unsigned long long u64;
  const int R = 8, C = 16, BIG = 50000;
  std::vector<float> a(3 * R * C), back(3 * R * C);
  for (size_t i = 0; i < a.size(); i++) a[i] = 700.f + 9.f * sinf(0.37f * (float)i) + (float)(i % 7);
  std::vector<unsigned char> mask(3 * R * C, 1), blob(4096), blob2(4096);
  unsigned n = 77, m = 77;

  // ---- the stock host calls
  EXPECT(lerc_computeCompressedSize(a.data(), 6, 1, C, R, 1, 0, nullptr, 0.01, &n), 0);
  EXPECT(lerc_encode(a.data(), 6, 1, C, R, 1, 0, nullptr, 0.01, blob.data(), 4096, &m), 0);
  if (n != m || n == 0) { failures++; printf("size %u, written %u\n", n, m); }
  EXPECT(lerc_encode(nullptr, 6, 1, C, R, 1, 0, nullptr, 0.01, blob2.data(), 4096, &m), 2);
  if (m != 0) { failures++; printf("a refused encode left %u in nBytesWritten\n", m); }
  EXPECT(lerc_encode(a.data(), 8, 1, C, R, 1, 0, nullptr, 0.01, blob2.data(), 4096, &m), 2);
  EXPECT(lerc_encode(a.data(), 6, 0, C, R, 1, 0, nullptr, 0.01, blob2.data(), 4096, &m), 2);
  EXPECT(lerc_encode(a.data(), 6, 1, -1, R, 1, 0, nullptr, 0.01, blob2.data(), 4096, &m), 2);
  EXPECT(lerc_encode(a.data(), 6, 1, C, R, 1, 0, nullptr, -1, blob2.data(), 4096, &m), 2);
  EXPECT(lerc_encode(a.data(), 6, 1, C, R, 1, 0, nullptr, 0.01, nullptr, 4096, &m), 2);
  EXPECT(lerc_encode(a.data(), 6, 1, C, R, 1, 0, nullptr, 0.01, blob2.data(), 0, &m), 2);
  EXPECT(lerc_encode(a.data(), 6, 1, C, R, 1, 0, nullptr, 0.01, blob2.data(), 4096, nullptr), 2);
  EXPECT(lerc_encode(a.data(), 6, 1, C, R, 3, 2, mask.data(), 0.01, blob2.data(), 4096, &m), 2);
  EXPECT(lerc_encode(a.data(), 6, 1, C, R, 1, 1, nullptr, 0.01, blob2.data(), 4096, &m), 2);
  EXPECT(lerc_encode(a.data(), 6, 1, BIG, BIG, 1, 0, nullptr, 0.01, blob2.data(), 4096, &m), 6);
  EXPECT(lerc_encode(a.data(), 6, 1, C, R, 3, 1, mask.data(), 0.01, blob2.data(), 4096, &m), 0);
  for (int v : { 7, 1, 0 }) EXPECT(lerc_encodeForVersion(a.data(), v, 6, 1, C, R, 1, 0, nullptr, 0.01, blob2.data(), 4096, &m), 2);
  EXPECT(lerc_encodeForVersion(a.data(), 3, 6, 1, C, R, 1, 0, nullptr, 0.01, blob2.data(), 4096, &m), 0);
  EXPECT(lerc_computeCompressedSizeForVersion(a.data(), 3, 6, 1, C, 0, 1, 0, nullptr, 0.01, &m), 2);
  const unsigned char flags[3] = { 1, 0, 0 };
  EXPECT(lerc_encode_4D(a.data(), 6, 1, C, R, 1, 0, nullptr, 0.01, blob2.data(), 4096, &m, flags, nullptr), 2);
  unsigned info[11];
  double range[3], mins[1], maxs[1];
  EXPECT(lerc_getBlobInfo(blob.data(), n, info, range, 11, 3), 0);
  EXPECT(lerc_getBlobInfo(blob.data(), n, nullptr, nullptr, 11, 3), 2);
  EXPECT(lerc_getBlobInfo(blob.data(), 0, info, range, 11, 3), 2);
  EXPECT(lerc_getDataRanges(blob.data(), n, 1, 1, mins, maxs), 0);
  EXPECT(lerc_getDataRanges(blob.data(), n, 0, 1, mins, maxs), 2);
  EXPECT(lerc_decode(blob.data(), n, 0, nullptr, 1, C, R, 1, 6, back.data()), 0);
  for (int i = 0; i < R * C; i++) if (fabsf(back[i] - a[i]) > 0.0101f) { failures++; printf("pixel %d: %f, was %f\n", i, back[i], a[i]); break; }
  EXPECT(lerc_decode(nullptr, n, 0, nullptr, 1, C, R, 1, 6, back.data()), 2);
  EXPECT(lerc_decode(blob.data(), n, 0, nullptr, 1, C, R, 1, 8, back.data()), 2);
  EXPECT(lerc_decode(blob.data(), n, 1, nullptr, 1, C, R, 1, 6, back.data()), 2);
  EXPECT(lerc_decode(blob.data(), n, 0, nullptr, 1, BIG, BIG, 1, 6, back.data()), 6);
  std::vector<double> wide(R * C);
  EXPECT(lerc_decodeToDouble(blob.data(), n, 0, nullptr, 1, C, R, 1, wide.data()), 0);
  EXPECT(lerc_decodeToDouble(blob.data(), n, 0, nullptr, 1, C, R, 0, wide.data()), 2);
  EXPECT(lerc_decodeToDouble(blob.data(), n, 0, nullptr, 1, BIG, BIG, 1, wide.data()), 1);

  // ---- the device calls (the emulator's device memory is host memory)
  lerc_amd_context* h = lerc_amd_create(nullptr);
  if (!h) { printf("no context\n"); return 1; }
  EXPECT(lerc_amd_encode_device(h, a.data(), 6, 1, C, R, 1, 0, nullptr, 0.01, blob2.data(), 4096, &m), 0);
  if (m != n || memcmp(blob.data(), blob2.data(), n)) { failures++; printf("the device call's blob differs from the host call's\n"); }
  EXPECT(lerc_amd_encode_device(nullptr, a.data(), 6, 1, C, R, 1, 0, nullptr, 0.01, blob2.data(), 4096, &m), 2);
  EXPECT(lerc_amd_encode_device(h, a.data(), 6, 1, C, R, 0, 0, nullptr, 0.01, blob2.data(), 4096, &m), 2);
  EXPECT(lerc_amd_encode_device(h, a.data(), 6, 1, BIG, BIG, 1, 0, nullptr, 0.01, blob2.data(), 4096, &m), 6);
  EXPECT(lerc_amd_decode_device(h, blob.data(), n, 0, nullptr, 1, C, R, 1, 6, back.data()), 0);
  EXPECT(lerc_amd_decode_device(h, blob.data(), 0, 0, nullptr, 1, C, R, 1, 6, back.data()), 2);
  EXPECT(lerc_amd_decode_device(h, blob.data(), n, 2, mask.data(), 1, C, R, 3, 6, back.data()), 2);
  unsigned ticket = 0, t2 = 0;
  EXPECT(lerc_amd_encode_device_async(h, a.data(), 6, 1, C, R, 1, 0, nullptr, 0.01, blob2.data(), 4096, &ticket), 0);
  EXPECT(lerc_amd_decode_device_async(h, blob2.data(), 4096, 0, nullptr, 1, C, R, 1, 6, back.data(), &t2), 0);
  EXPECT(lerc_amd_encode_device_async(h, a.data(), 6, 1, C, R, 1, 0, nullptr, -1, blob2.data(), 4096, &m), 2);
  EXPECT(lerc_amd_decode_device_async(h, blob2.data(), 4096, 0, nullptr, 1, C, R, 1, 6, nullptr, &m), 2);
  EXPECT(lerc_amd_finish(h, ticket, &m), 0);
  if (m != n) { failures++; printf("the queued encode wrote %u bytes\n", m); }
  EXPECT(lerc_amd_finish(h, t2, nullptr), 0);
  EXPECT(lerc_amd_finish(h, 0x7FFFFFF0u, &m), 2);
  EXPECT(lerc_amd_finish(nullptr, 0, &m), 2);

  // ---- tile batches: two tiles of 8 x 16
  std::vector<unsigned char> arena(8192);
  u64 offs[2], used = 0;
  unsigned sizes[2];
  EXPECT(lerc_amd_encode_tiles_device(h, a.data(), 6, C, R, 2, 0.01, arena.data(), 8192, offs, sizes, &used), 0);
  EXPECT(lerc_amd_encode_tiles_device(h, a.data(), 6, C, R, 0, 0.01, arena.data(), 8192, offs, sizes, &used), 2);
  EXPECT(lerc_amd_encode_tiles_device(h, a.data(), 6, C, R, 2, 0.01, nullptr, 8192, offs, sizes, &used), 2);
  EXPECT(lerc_amd_encode_tiles_device(h, a.data(), 6, BIG, BIG, 2, 0.01, arena.data(), 8192, offs, sizes, &used), 6);
  EXPECT(lerc_amd_decode_tiles_device(h, arena.data(), offs, sizes, 2, C, R, 6, back.data()), 0);
  EXPECT(lerc_amd_decode_tiles_device(h, arena.data(), offs, nullptr, 2, C, R, 6, back.data()), 2);
  EXPECT(lerc_amd_decode_tiles_device_masked(h, arena.data(), offs, sizes, 2, C, R, 6, back.data(), mask.data()), 0);
  std::vector<unsigned char> slots(2 * 2048);
  EXPECT(lerc_amd_encode_tiles_device_slots(h, a.data(), 6, C, R, 2, 0.01, slots.data(), 2048, sizes), 0);
  EXPECT(lerc_amd_encode_tiles_device_slots(h, a.data(), 6, C, R, 2, 0.01, slots.data(), 8, sizes), 2);
  EXPECT(lerc_amd_encode_tiles_device_slots(h, a.data(), 6, C, R, 2, 0.01, slots.data(), 0, sizes), 2);
  EXPECT(lerc_amd_decode_tiles_device_slots(h, slots.data(), 2048, sizes, 2, C, R, 6, back.data()), 0);
  EXPECT(lerc_amd_decode_tiles_device_slots(h, slots.data(), 0, sizes, 2, C, R, 6, back.data()), 2);
  EXPECT(lerc_amd_encode_tiles_device_masked(h, a.data(), 6, C, R, 2, mask.data(), 0.01, slots.data(), 4096, 2048, offs, sizes, &used), 0);
  EXPECT(lerc_amd_encode_tiles_device_masked(h, a.data(), 6, C, R, 2, mask.data(), 0.01, slots.data(), 4096, 8, offs, sizes, &used), 2);
  EXPECT(lerc_amd_encode_tiles_device_bands(h, a.data(), 6, C, R, 1, 2, 1, mask.data(), 0.01, arena.data(), 8192, 0, offs, sizes, &used), 0);
  EXPECT(lerc_amd_encode_tiles_device_bands(h, a.data(), 6, C, R, 1, 2, 0, mask.data(), 0.01, arena.data(), 8192, 0, offs, sizes, &used), 2);
  EXPECT(lerc_amd_encode_tiles_device_bands(h, a.data(), 6, C, R, 1, 2, 1, nullptr, 0.01, arena.data(), 8192, 0, offs, sizes, &used), 2);
  EXPECT(lerc_amd_decode_tiles_device_bands(h, arena.data(), offs, sizes, 2, C, R, 1, 6, back.data(), 1, mask.data()), 0);
  EXPECT(lerc_amd_decode_tiles_device_bands(h, arena.data(), offs, sizes, 2, C, R, 0, 6, back.data(), 1, mask.data()), 2);

  // ---- a 24 x 40 raster in tiles of 16 x 16, rows 45 elements apart
  const int RR = 24, RC = 40, P = 45;
  std::vector<float> raster(RR * P + 7), win(13 * 26 + 7);
  for (size_t i = 0; i < raster.size(); i++) raster[i] = 500.f + (float)(i % 11);
  std::vector<unsigned char> rarena(6 * 2048);
  u64 roffs[6];
  unsigned rsizes[6];
  used = 77;
  EXPECT(lerc_amd_encode_raster_tiles_device(h, raster.data(), 6, RC, RR, 1, P, RR * P, 16, 16, 0, nullptr, 0, 0.01, rarena.data(), 6 * 2048, 0, roffs, rsizes, &used), 0);
  EXPECT(lerc_amd_encode_raster_tiles_device(h, raster.data(), 6, RC, RR, 1, P, RR * P, 0, 16, 0, nullptr, 0, 0.01, rarena.data(), 6 * 2048, 0, roffs, rsizes, &used), 2);
  if (used != 0) { failures++; printf("a refused raster encode left %llu in arenaUsed\n", used); }
  EXPECT(lerc_amd_encode_raster_tiles_device(h, nullptr, 6, RC, RR, 1, P, RR * P, 16, 16, 0, nullptr, 0, 0.01, rarena.data(), 6 * 2048, 0, roffs, rsizes, &used), 2);
  EXPECT(lerc_amd_encode_raster_tiles_device_strided(h, raster.data(), 6, BIG, BIG, 1, 1, P, RR * P, BIG, BIG, 0, nullptr, 0, 0.01, rarena.data(), 6 * 2048, 0, roffs, rsizes, &used), 6);
  EXPECT(lerc_amd_encode_raster_tiles_device_range(h, raster.data(), 6, RC, RR, 1, 1, P, RR * P, 16, 16, -1, 1, 2, 1, 0, nullptr, 0, 0.01, rarena.data(), 6 * 2048, 0, roffs, rsizes, &used), 2);
  EXPECT(lerc_amd_encode_raster_tiles_device_range(h, raster.data(), 6, RC, RR, 1, 1, P, RR * P, 16, 16, 1, 1, 2, 1, 0, nullptr, 0, 0.01, rarena.data(), 6 * 2048, 0, roffs, rsizes, &used), 0);
  EXPECT(lerc_amd_encode_raster_tiles_device(h, raster.data(), 6, RC, RR, 1, P, RR * P, 16, 16, 0, nullptr, 0, 0.01, rarena.data(), 6 * 2048, 0, roffs, rsizes, &used), 0);
  EXPECT(lerc_amd_decode_raster_window_device(h, rarena.data(), roffs, rsizes, 6, RC, RR, 1, 16, 16, 7, 5, 21, 13, win.data(), 1, 26, 13 * 26, 0, nullptr, 0), 0);
  for (int i = 0; i < 13; i++) for (int j = 0; j < 21; j++)
    if (fabsf(win[i * 26 + j] - raster[(5 + i) * P + 7 + j]) > 0.0101f) { failures++; printf("window pixel (%d, %d)\n", i, j); i = 13; break; }
  EXPECT(lerc_amd_decode_raster_window_device(h, rarena.data(), roffs, rsizes, 6, RC, RR, 1, 16, 16, 7, 5, 0, 13, win.data(), 1, 26, 13 * 26, 0, nullptr, 0), 2);
  EXPECT(lerc_amd_decode_raster_tiles_device_strided(h, rarena.data(), roffs, rsizes, 8, RC, RR, 1, 1, P, RR * P, 16, 16, raster.data(), 0, nullptr, 0), 2);
  EXPECT(lerc_amd_decode_raster_tiles_device(h, rarena.data(), nullptr, rsizes, 6, RC, RR, 1, P, RR * P, 16, 16, raster.data(), 0, nullptr, 0), 2);
  u64 counts[4];
  lerc_amd_raster_tiles_counters(h, counts);
  lerc_amd_raster_tiles_counters(nullptr, counts);
  lerc_amd_path_counters(nullptr, counts);
  EXPECT(lerc_amd_gather_blobs(h, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, nullptr, nullptr), 2);
  EXPECT(lerc_amd_mask_rle_device(h, nullptr, 64, blob2.data(), 256, &m), 2);
  EXPECT(lerc_amd_mask_rle_decode_device(h, blob2.data(), 1, mask.data(), 64), 2);
  lerc_amd_destroy(h);
  printf(failures ? "check_capi_boundary: %d FAILURES\n" : "check_capi_boundary: ok\n", failures);
  return failures ? 1 : 0;
}
