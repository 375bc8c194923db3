// derive.hip — dictionary twin of a raw INT / LONG / FLOAT / DOUBLE column, derived on the device
// (GROUP BY on a raw column groups by value: NoDictionarySingleColumnGroupKeyGenerator.java:98-143
// keeps a value -> group id map per segment; here each segment gets, once, a sorted dictionary of its
// distinct values and a fixed-bit dictId forward index, so raw group-by columns take the dictionary
// plans). Values are compared by Java's identity for FLOAT / DOUBLE (Float.floatToIntBits /
// Double.doubleToLongBits equality: every NaN one value, -0.0 != 0.0) and ordered by Double.compare.
//
//   1. order_keys_kernel:   big-endian staged values -> order-preserving uint64 keys
//   2. rocprim radix sort of the keys (a copy)
//   3. unique_flags_kernel + exclusive scan: distinct keys in order, their count = cardinality
//   4. dict_ids_kernel:     per doc, the dictId (binary search in the distinct keys)
//   5. dict_values_kernel:  distinct keys -> big-endian dictionary values (the staged dictionary format)
// The fixed-bit packing reuses pack_dict_ids_kernel (kernels.hip).
//
// A transformed GROUP BY key (dateTrunc / timeConvert / dateTimeConvert of an INT / LONG column) gets its twin the
// same way: step 1 becomes transform_keys_kernel, which writes the order-preserving key of f(value), and the
// dictionary's values are LONG. A dictionary-encoded or sorted source derives over its dictionary's values (the
// `ids` are then the old dictId -> twin dictId table) and maps the docs through that table
// (remap_dict_ids_kernel / sorted_dict_ids_kernel).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "../../include/pinot_amd.h"
#include "device_types.h"
#include "kernels.h"
#define PAMD_HLL_HD __host__ __device__
#include "hll.h"

namespace pamd {

__device__ __forceinline__ uint64_t java_double_order_dev(double v) {
  // Double.compare order: NaN (canonical, above +inf); -0.0 < 0.0
  uint64_t b = (uint64_t)__double_as_longlong(v);
  if (v != v) b = 0x7FF8000000000000ull;
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

__global__ void order_keys_kernel(const uint8_t* be, int type, int64_t n, uint64_t* keys) {
  for (int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; d < n; d += (int64_t)gridDim.x * blockDim.x) {
    uint64_t k;
    if (type == T_INT || type == T_FLOAT) {
      const uint32_t u = __builtin_bswap32(reinterpret_cast<const uint32_t*>(be)[d]);
      if (type == T_INT) k = (uint64_t)(int64_t)(int32_t)u ^ (1ull << 63);
      else k = java_double_order_dev((double)__uint_as_float(u));
    } else {
      const uint32_t* w = reinterpret_cast<const uint32_t*>(be) + 2 * d;
      const uint64_t u = ((uint64_t)__builtin_bswap32(w[0]) << 32) | __builtin_bswap32(w[1]);
      k = type == T_LONG ? (u ^ (1ull << 63)) : java_double_order_dev(__longlong_as_double((long long)u));
    }
    keys[d] = k;
  }
}

// ------------------------------------------------------------------------------------------------
// GROUP BY key transforms (pinot_amd_query_add_group_by_transform): dateTrunc / timeConvert /
// dateTimeConvert of an INT / LONG value, in Java long arithmetic. Products that Java lets wrap are computed
// unsigned; every fixed divisor is a compile-time constant (a switch on the unit), only a granularity whose
// size is not 1 divides by a run-time value.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ int64_t wrap_mul(int64_t a, int64_t b) { return (int64_t)((uint64_t)a * (uint64_t)b); }
__device__ __forceinline__ int64_t wrap_add(int64_t a, int64_t b) { return (int64_t)((uint64_t)a + (uint64_t)b); }

// TimeUnit.convert(v, from) of unit `to` (TimeUnit ordinals, NANOSECONDS = 0 .. DAYS = 6). Scaling down is a
// chain of truncating divisions by the steps between neighbouring units (truncation composes); scaling up
// saturates (the JDK's bounds check equals mathematical saturation: no ratio is a power of two).
__device__ __forceinline__ int64_t time_unit_convert(int64_t v, int from, int to) {
  if (to > from) {
    if (from <= 0 && to > 0) v /= 1000;
    if (from <= 1 && to > 1) v /= 1000;
    if (from <= 2 && to > 2) v /= 1000;
    if (from <= 3 && to > 3) v /= 60;
    if (from <= 4 && to > 4) v /= 60;
    if (from <= 5 && to > 5) v /= 24;
    return v;
  }
  if (to == from) return v;
  int64_t ratio = 1;
  if (to <= 0 && from > 0) ratio *= 1000;
  if (to <= 1 && from > 1) ratio *= 1000;
  if (to <= 2 && from > 2) ratio *= 1000;
  if (to <= 3 && from > 3) ratio *= 60;
  if (to <= 4 && from > 4) ratio *= 60;
  if (to <= 5 && from > 5) ratio *= 24;
  int64_t r;
  if (__builtin_mul_overflow(v, ratio, &r)) r = v < 0 ? INT64_MIN : INT64_MAX;
  return r;
}

// floor(a / C) * C for a constant C > 0 (Joda PreciseDateTimeField.roundFloor: toward -inf)
template <int64_t C>
__device__ __forceinline__ int64_t floor_to(int64_t a) {
  int64_t q = a / C;
  if (a % C < 0) --q;
  return wrap_mul(q, C);
}

// days since 1970-01-01 of the first day of civil (y, m) and back, proleptic Gregorian (ISOChronology), 64-bit;
// eras of 400 years = 146097 days starting on March 1
__device__ __forceinline__ int64_t days_from_civil(int64_t y, int m) {
  y -= m <= 2;
  const int64_t era = (y >= 0 ? y : y - 399) / 400;
  const int64_t yoe = y - era * 400;
  const int64_t doy = (153 * (m > 2 ? m - 3 : m + 9) + 2) / 5;
  const int64_t doe = yoe * 365 + yoe / 4 - yoe / 100 + doy;
  return era * 146097 + doe - 719468;
}
__device__ __forceinline__ void civil_from_days(int64_t z, int64_t* y, int* m) {
  z += 719468;
  const int64_t era = (z >= 0 ? z : z - 146096) / 146097;
  const int64_t doe = z - era * 146097;
  const int64_t yoe = (doe - doe / 1460 + doe / 36524 - doe / 146096) / 365;
  const int64_t doy = doe - (365 * yoe + yoe / 4 - yoe / 100);
  const int64_t mp = (5 * doy + 2) / 153;
  *m = (int)(mp < 10 ? mp + 3 : mp - 9);
  *y = yoe + era * 400 + (*m <= 2);
}

__device__ __forceinline__ int64_t date_trunc_floor(int64_t ms, int unit) {
  constexpr int64_t kDay = 86400000;
  switch (unit) {
    case PINOT_AMD_TRUNC_SECOND: return floor_to<1000>(ms);
    case PINOT_AMD_TRUNC_MINUTE: return floor_to<60000>(ms);
    case PINOT_AMD_TRUNC_HOUR: return floor_to<3600000>(ms);
    case PINOT_AMD_TRUNC_DAY: return floor_to<kDay>(ms);
    case PINOT_AMD_TRUNC_WEEK: return wrap_add(floor_to<7 * kDay>(wrap_add(ms, 3 * kDay)), -3 * kDay);  // Monday
    case PINOT_AMD_TRUNC_MONTH:
    case PINOT_AMD_TRUNC_QUARTER:
    case PINOT_AMD_TRUNC_YEAR: {
      int64_t days = ms / kDay;
      if (ms % kDay < 0) --days;
      int64_t y;
      int m;
      civil_from_days(days, &y, &m);
      if (unit == PINOT_AMD_TRUNC_YEAR) m = 1;
      if (unit == PINOT_AMD_TRUNC_QUARTER) m = (m - 1) / 3 * 3 + 1;
      return wrap_mul(days_from_civil(y, m), kDay);
    }
    default: return ms;  // millisecond
  }
}

__device__ __forceinline__ int64_t key_transform_value(int64_t v, const DevKeyTransform& tf) {
  constexpr int kMillis = PINOT_AMD_MILLISECONDS;
  switch (tf.kind) {
    case PINOT_AMD_KEY_DATETRUNC:
      return time_unit_convert(date_trunc_floor(time_unit_convert(v, tf.in_unit, kMillis), tf.trunc_unit), kMillis,
                               tf.out_unit);
    case PINOT_AMD_KEY_TIMECONVERT: return time_unit_convert(v, tf.in_unit, tf.out_unit);
    default: {  // DATETIMECONVERT
      const int64_t ms = time_unit_convert(wrap_mul(v, tf.in_size), tf.in_unit, kMillis);
      int64_t q;
      switch (tf.gran_unit) {  // a granularity of size 1: constant divisors
        case PINOT_AMD_MILLISECONDS: q = ms; break;
        case PINOT_AMD_SECONDS: q = ms / 1000 * 1000; break;
        case PINOT_AMD_MINUTES: q = ms / 60000 * 60000; break;
        case PINOT_AMD_HOURS: q = ms / 3600000 * 3600000; break;
        case PINOT_AMD_DAYS: q = ms / 86400000 * 86400000; break;
        default: q = ms / tf.gran_ms * tf.gran_ms; break;
      }
      const int64_t o = time_unit_convert(q, kMillis, tf.out_unit);
      return tf.out_size == 1 ? o : o / tf.out_size;
    }
  }
}

// step 1 of derive_dictionary for a transformed key: source values -> order-preserving keys of f(value).
// src: DERIVE_SRC_BE (staged raw INT / LONG, byte-swapped loads) or DERIVE_SRC_LE64 (dictionary values)
__global__ void transform_keys_kernel(const uint8_t* in, int type, int src, int64_t n, DevKeyTransform tf,
                                      uint64_t* keys) {
  for (int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; d < n; d += (int64_t)gridDim.x * blockDim.x) {
    int64_t v;
    if (src == DERIVE_SRC_LE64) {
      v = reinterpret_cast<const int64_t*>(in)[d];
    } else if (type == T_INT) {
      v = (int64_t)(int32_t)__builtin_bswap32(reinterpret_cast<const uint32_t*>(in)[d]);
    } else {
      const uint2 w = reinterpret_cast<const uint2*>(in)[d];
      v = (int64_t)(((uint64_t)__builtin_bswap32(w.x) << 32) | __builtin_bswap32(w.y));
    }
    keys[d] = (uint64_t)key_transform_value(v, tf) ^ (1ull << 63);
  }
}

// a dictionary column's docs through the old dictId -> twin dictId table (card entries)
__global__ void remap_dict_ids_kernel(int32_t* ids, int64_t n, const int32_t* map, int64_t card) {
  for (int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; d < n; d += (int64_t)gridDim.x * blockDim.x) {
    const int64_t id = ids[d];
    ids[d] = id >= 0 && id < card ? map[id] : 0;
  }
}

// a sorted column's docs: the dictId is the last one whose first docId is <= the doc (starts ascending, starts[0]
// = 0), then the same table
__global__ void sorted_dict_ids_kernel(const int32_t* starts, int64_t card, int64_t n, const int32_t* map,
                                       int32_t* ids) {
  for (int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; d < n; d += (int64_t)gridDim.x * blockDim.x) {
    int64_t lo = 0, hi = card - 1;
    while (lo < hi) {
      const int64_t mid = (lo + hi + 1) >> 1;
      if ((int64_t)starts[mid] <= d) lo = mid; else hi = mid - 1;
    }
    ids[d] = map[lo];
  }
}

__global__ void unique_flags_kernel(const uint64_t* sorted, int64_t n, uint32_t* flags) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    flags[i] = (i == 0 || sorted[i] != sorted[i - 1]) ? 1u : 0u;
}

__global__ void scatter_unique_kernel(const uint64_t* sorted, const uint32_t* flags, const uint32_t* pos, int64_t n,
                                      uint64_t* uniq) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    if (flags[i]) uniq[pos[i]] = sorted[i];
}

__global__ void dict_ids_kernel(const uint64_t* keys, int64_t n, const uint64_t* uniq, int64_t card, int32_t* ids) {
  for (int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; d < n; d += (int64_t)gridDim.x * blockDim.x) {
    const uint64_t k = keys[d];
    int64_t lo = 0, hi = card - 1;
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (uniq[mid] < k) lo = mid + 1; else hi = mid;
    }
    ids[d] = (int32_t)lo;
  }
}

// distinct keys -> dictionary values, big-endian fixed width (4 B INT / FLOAT, 8 B LONG / DOUBLE)
__global__ void dict_values_kernel(const uint64_t* uniq, int64_t card, int type, uint8_t* out) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < card; i += (int64_t)gridDim.x * blockDim.x) {
    const uint64_t k = uniq[i];
    uint64_t u;
    if (type == T_INT || type == T_LONG) {
      u = k ^ (1ull << 63);
    } else {
      const uint64_t b = (k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k;
      if (type == T_FLOAT) {
        const float f = (float)__longlong_as_double((long long)b);
        u = (uint64_t)__float_as_uint(f);
      } else {
        u = b;
      }
    }
    if (type == T_INT || type == T_FLOAT) {
      reinterpret_cast<uint32_t*>(out)[i] = __builtin_bswap32((uint32_t)u);
    } else {
      reinterpret_cast<uint32_t*>(out)[2 * i] = __builtin_bswap32((uint32_t)(u >> 32));
      reinterpret_cast<uint32_t*>(out)[2 * i + 1] = __builtin_bswap32((uint32_t)u);
    }
  }
}

static unsigned grid_of(int64_t n) {
  const int64_t g = (n + 255) / 256;
  return (unsigned)(g < 1 ? 1 : g > 8192 ? 8192 : g);
}

// scratch: caller-provided device buffers sized by derive_dictionary_scratch (keys, sorted keys, flags,
// positions, distinct keys: n entries each, plus the sort / scan temporary storage)
size_t derive_dictionary_scratch(int64_t n) {
  size_t sort_bytes = 0, scan_bytes = 0;
  (void)rocprim::radix_sort_keys(nullptr, sort_bytes, (const uint64_t*)nullptr, (uint64_t*)nullptr, (unsigned int)n, 0,
                                 64);
  (void)rocprim::exclusive_scan(nullptr, scan_bytes, (const uint32_t*)nullptr, (uint32_t*)nullptr, 0u, (size_t)n,
                                rocprim::plus<uint32_t>());
  const size_t tmp = sort_bytes > scan_bytes ? sort_bytes : scan_bytes;
  return (size_t)n * (8 + 8 + 4 + 4 + 8) + tmp + 256;
}

// -> *h_card distinct values; d_ids[n] the items' dictIds; d_dict_be[card * value size] the dictionary.
// tf == nullptr: the dictionary of the source values themselves (big-endian values of `type`). tf != nullptr: the
// dictionary of f(value) of INT / LONG source values stored as `src` says; its values are LONG.
hipError_t derive_dictionary(const uint8_t* d_src, int type, int src, const DevKeyTransform* tf, int64_t n,
                             void* d_scratch, int32_t* d_ids, uint8_t* d_dict_be, int64_t* h_card, hipStream_t st) {
  if (tf ? (type != T_INT && type != T_LONG) : src != DERIVE_SRC_BE) return hipErrorInvalidValue;
  if (n <= 0) {
    *h_card = 0;
    return hipSuccess;
  }
  uint8_t* p = reinterpret_cast<uint8_t*>(d_scratch);
  uint64_t* keys = reinterpret_cast<uint64_t*>(p);
  uint64_t* sorted = keys + n;
  uint32_t* flags = reinterpret_cast<uint32_t*>(sorted + n);
  uint32_t* pos = flags + n;
  uint64_t* uniq = reinterpret_cast<uint64_t*>(pos + n);
  void* tmp = reinterpret_cast<void*>(((uintptr_t)(uniq + n) + 255) & ~(uintptr_t)255);
  size_t sort_bytes = 0, scan_bytes = 0;
  hipError_t e = rocprim::radix_sort_keys(nullptr, sort_bytes, keys, sorted, (unsigned int)n, 0, 64, st);
  if (e != hipSuccess) return e;
  e = rocprim::exclusive_scan(nullptr, scan_bytes, flags, pos, 0u, (size_t)n, rocprim::plus<uint32_t>(), st);
  if (e != hipSuccess) return e;
  if (tf) hipLaunchKernelGGL(transform_keys_kernel, dim3(grid_of(n)), dim3(256), 0, st, d_src, type, src, n, *tf, keys);
  else hipLaunchKernelGGL(order_keys_kernel, dim3(grid_of(n)), dim3(256), 0, st, d_src, type, n, keys);
  e = rocprim::radix_sort_keys(tmp, sort_bytes, keys, sorted, (unsigned int)n, 0, 64, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(unique_flags_kernel, dim3(grid_of(n)), dim3(256), 0, st, sorted, n, flags);
  e = rocprim::exclusive_scan(tmp, scan_bytes, flags, pos, 0u, (size_t)n, rocprim::plus<uint32_t>(), st);
  if (e != hipSuccess) return e;
  uint32_t last[2];
  e = hipMemcpyAsync(&last[0], pos + n - 1, 4, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(&last[1], flags + n - 1, 4, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return e;
  const int64_t card = (int64_t)last[0] + last[1];
  hipLaunchKernelGGL(scatter_unique_kernel, dim3(grid_of(n)), dim3(256), 0, st, sorted, flags, pos, n, uniq);
  hipLaunchKernelGGL(dict_ids_kernel, dim3(grid_of(n)), dim3(256), 0, st, keys, n, uniq, card, d_ids);
  hipLaunchKernelGGL(dict_values_kernel, dim3(grid_of(card)), dim3(256), 0, st, uniq, card, tf ? (int)T_LONG : type,
                     d_dict_be);
  *h_card = card;
  return hipGetLastError();
}

hipError_t launch_remap_dict_ids(int32_t* ids, int64_t n, const int32_t* map, int64_t card, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(remap_dict_ids_kernel, dim3(grid_of(n)), dim3(256), 0, st, ids, n, map, card);
  return hipGetLastError();
}

hipError_t launch_sorted_dict_ids(const int32_t* starts, int64_t card, int64_t n, const int32_t* map, int32_t* ids,
                                  hipStream_t st) {
  if (n <= 0) return hipSuccess;
  if (card < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(sorted_dict_ids_kernel, dim3(grid_of(n)), dim3(256), 0, st, starts, card, n, map, ids);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// Compacted hash-table groups in ascending key order (the order a dense table's groups come in): a
// hash plan's packed key words compare, as one (nwk x 64)-bit integer with word nwk - 1 most
// significant, exactly as the group columns' merged ids from the last column to the first, so a stable
// LSD radix sort over the words -- least significant word first, each pass sorting (word, row) pairs in
// the order the previous passes left -- yields the permutation; the rows are then gathered.
// ------------------------------------------------------------------------------------------------
__global__ void key_word_kernel(const uint64_t* keys, int nwk, int w, const uint32_t* idx, int64_t n, uint64_t* out) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    out[i] = keys[(idx ? (int64_t)idx[i] : i) * nwk + w];
}
__global__ void iota_kernel(uint32_t* idx, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    idx[i] = (uint32_t)i;
}
__global__ void gather_rows_kernel(const uint64_t* src, int width, const uint32_t* idx, int64_t n, uint64_t* dst) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n * width; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / width, c = i - r * width;
    dst[i] = src[(int64_t)idx[r] * width + c];
  }
}

size_t sort_rows_scratch(int64_t n) {
  size_t sort_bytes = 0;
  (void)rocprim::radix_sort_pairs(nullptr, sort_bytes, (const uint64_t*)nullptr, (uint64_t*)nullptr,
                                  (const uint32_t*)nullptr, (uint32_t*)nullptr, (unsigned int)n, 0, 64);
  return (size_t)n * (8 + 8 + 4 + 4) + sort_bytes + 512;
}

// keys: n rows of nwk words (row-major), acc: n rows of nacc words; word_bits[w]: bits word w can use.
// Rows written to keys_out / acc_out in ascending key order.
hipError_t sort_rows_by_key(const uint64_t* keys, int nwk, const int* word_bits, const uint64_t* acc, int nacc, int64_t n,
                            void* scratch, uint64_t* keys_out, uint64_t* acc_out, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  uint8_t* p = reinterpret_cast<uint8_t*>(scratch);
  uint64_t* kw = reinterpret_cast<uint64_t*>(p);
  uint64_t* kw2 = kw + n;
  uint32_t* idx = reinterpret_cast<uint32_t*>(kw2 + n);
  uint32_t* idx2 = idx + n;
  void* tmp = reinterpret_cast<void*>(((uintptr_t)(idx2 + n) + 255) & ~(uintptr_t)255);
  size_t sort_bytes = 0;
  hipError_t e = rocprim::radix_sort_pairs(nullptr, sort_bytes, kw, kw2, idx, idx2, (unsigned int)n, 0, 64, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(iota_kernel, dim3(grid_of(n)), dim3(256), 0, st, idx, n);
  for (int w = 0; w < nwk; ++w) {
    hipLaunchKernelGGL(key_word_kernel, dim3(grid_of(n)), dim3(256), 0, st, keys, nwk, w, (const uint32_t*)idx, n, kw);
    const unsigned end_bit = (unsigned)(word_bits[w] < 1 ? 1 : word_bits[w] > 64 ? 64 : word_bits[w]);
    e = rocprim::radix_sort_pairs(tmp, sort_bytes, kw, kw2, idx, idx2, (unsigned int)n, 0u, end_bit, st);
    if (e != hipSuccess) return e;
    uint32_t* t = idx;  // the sorted permutation becomes the next pass's input order
    idx = idx2;
    idx2 = t;
  }
  hipLaunchKernelGGL(gather_rows_kernel, dim3(grid_of(n * nwk)), dim3(256), 0, st, keys, nwk, (const uint32_t*)idx, n, keys_out);
  hipLaunchKernelGGL(gather_rows_kernel, dim3(grid_of(n * nacc)), dim3(256), 0, st, acc, nacc, (const uint32_t*)idx, n, acc_out);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// Multi-value columns (FixedBitMVForwardIndexReader's format, DevMvColumn): value-parallel over tiles of
// kMvTileValues values. A value's doc is tile_first_doc[tile] + (start bits of the tile up to and including the
// value) - 1: the tile's 128 bitmap dwords are staged in LDS with the exclusive prefix of their popcounts, a value
// before the tile's first start bit belongs to the doc straddling in from the previous tile.
//   mv_tile_count_kernel / mv_tile_scan_kernel   staging: start bits per tile, scanned into tile_first_doc
//   mv_validate_kernel                           staging: bit 0, the chunk offset header, the longest doc
//   mv_read_kernel                               getDictIdMV for the whole column (offsets and dictIds)
//   mv_match_kernel                              an ANY-match predicate -> the segment's dense docId bitset
//   mv_reduce_kernel                             per-doc count / sum / min / max (the *MV aggregations' twins)
// ------------------------------------------------------------------------------------------------
constexpr int kMvBmWords = kMvTileValues / 32;       // bitmap dwords of a tile
constexpr int kMvPerThread = kMvTileValues / kBlock;  // values per lane
constexpr int kMvWinWords = kMvTileValues / 32 + 4;   // 32-doc words a tile's docs (<= 4097) can touch
static_assert(kMvBmWords == 128 && kBlock == 256, "the block's first two waves stage a tile's bitmap");

__device__ __forceinline__ uint32_t mv_dict_id(const DevMvColumn& c, int64_t v) {
  const int64_t b = c.raw_bit0 + v * c.bits;
  const uint32_t* w = c.words + (b >> 5);
  const uint64_t win = ((uint64_t)__builtin_bswap32(w[0]) << 32) | (uint64_t)__builtin_bswap32(w[1]);
  return (uint32_t)((win << (uint32_t)(b & 31)) >> (64 - c.bits));
}
// bitmap dword j of the column (MSB = value 32 j), the bits at and beyond num_values cleared
__device__ __forceinline__ uint32_t mv_bitmap_word(const DevMvColumn& c, int64_t j) {
  const int64_t v0 = j * 32;
  if (v0 >= c.num_values) return 0u;
  uint32_t x = __builtin_bswap32(c.words[c.bm_word0 + j]);
  const int64_t rem = c.num_values - v0;
  if (rem < 32) x &= ~0u << (32 - (int)rem);
  return x;
}
// Stages the tile's bitmap in bm[kMvBmWords] with pre[j] = start bits of the tile before dword j; returns the
// tile's start bits. Every thread of the block calls it; the arrays are ready when it returns.
__device__ __forceinline__ uint32_t mv_stage_tile(const DevMvColumn& c, int64_t tile, uint32_t* bm, uint32_t* pre,
                                                  uint32_t* tot) {
  const int tid = (int)threadIdx.x;
  const uint32_t x = tid < kMvBmWords ? mv_bitmap_word(c, tile * kMvBmWords + tid) : 0u;
  const uint32_t p = (uint32_t)__popc(x);
  uint32_t inc = p;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t t = __shfl_up(inc, o, 64);
    if ((tid & 63) >= o) inc += t;
  }
  if (tid == 63) tot[0] = inc;
  __syncthreads();
  if (tid < kMvBmWords) {
    bm[tid] = x;
    const uint32_t e = inc - p + (tid >= 64 ? tot[0] : 0u);
    pre[tid] = e;
    if (tid == kMvBmWords - 1) tot[1] = e + p;
  }
  __syncthreads();
  return tot[1];
}
// start bits of the tile up to and including its value vi (0 .. kMvTileValues)
__device__ __forceinline__ uint32_t mv_rank(const uint32_t* bm, const uint32_t* pre, int vi) {
  return pre[vi >> 5] + (uint32_t)__popc(bm[vi >> 5] >> (31 - (vi & 31)));
}

__global__ void __launch_bounds__(kBlock) mv_tile_count_kernel(DevMvColumn c, int64_t ntiles, int32_t* counts) {
  __shared__ uint32_t bm[kMvBmWords], pre[kMvBmWords], tot[2];
  const int64_t tile = blockIdx.x;
  if (tile >= ntiles) return;
  const uint32_t n = mv_stage_tile(c, tile, bm, pre, tot);
  if (threadIdx.x == 0) counts[tile] = (int32_t)n;
}

// exclusive scan of the tiles' counts in place (one block), total[0] = every start bit
__global__ void __launch_bounds__(kBlock) mv_tile_scan_kernel(int32_t* counts, int64_t ntiles, long long* total) {
  __shared__ long long wsum[kBlock / 64];
  __shared__ long long carry;
  const int tid = (int)threadIdx.x;
  if (tid == 0) carry = 0;
  __syncthreads();
  for (int64_t base = 0; base < ntiles; base += kBlock) {
    const int64_t i = base + tid;
    const long long x = i < ntiles ? (long long)counts[i] : 0;
    long long inc = x;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const long long t = __shfl_up(inc, o, 64);
      if ((tid & 63) >= o) inc += t;
    }
    if ((tid & 63) == 63) wsum[tid >> 6] = inc;
    __syncthreads();
    long long before = carry;
    for (int w = 0; w < (tid >> 6); ++w) before += wsum[w];
    // (a rank beyond int32 cannot be a docId: the host refuses the column from the total)
    if (i < ntiles) counts[i] = (int32_t)min(before + inc - x, (long long)INT32_MAX);
    __syncthreads();
    if (tid == kBlock - 1) carry = before + inc;
    __syncthreads();
  }
  if (tid == 0) total[0] = carry;
}

// flags: 1 = bit 0 unset, 4 = a chunk offset header entry disagrees with the bitmap's rank, 8 = a doc longer
// than max_values. header: the num_chunks big-endian entries at the head of the file.
__global__ void __launch_bounds__(kBlock) mv_validate_kernel(DevMvColumn c, int64_t ntiles, int32_t docs_per_chunk,
                                                             int32_t num_chunks, int32_t max_values, uint32_t* flags) {
  __shared__ uint32_t bm[kMvBmWords], pre[kMvBmWords], tot[2];
  const int64_t tile = blockIdx.x;
  if (tile >= ntiles) return;
  mv_stage_tile(c, tile, bm, pre, tot);
  const int64_t tfd = c.tile_first_doc[tile];
  const int tid = (int)threadIdx.x;
  if (tile == 0 && tid == 0 && !(bm[0] >> 31)) atomicOr(flags, 1u);
  uint32_t bad = 0;
  if (tid < kMvBmWords) {
    uint32_t x = bm[tid];
    while (x) {
      const int b = __clz((int)x);  // position from the MSB = value 32 tid + b of the tile
      x &= ~(0x80000000u >> b);
      const int vi = tid * 32 + b;
      const int64_t v = tile * kMvTileValues + vi;
      const int64_t d = tfd + (int64_t)mv_rank(bm, pre, vi) - 1;
      if (docs_per_chunk > 0 && d % docs_per_chunk == 0) {
        const int64_t k = d / docs_per_chunk;
        if (k >= num_chunks || (int64_t)(int32_t)__builtin_bswap32(c.words[k]) != v) bad |= 4u;
      }
      // the doc's end: the next start bit (in this dword, or the first non-empty dword behind it) or num_values
      int64_t end;
      if (x) {
        end = tile * kMvTileValues + tid * 32 + __clz((int)x);
      } else {
        const int64_t nwords = (c.num_values + 31) / 32;
        // (a valid doc ends within max_values: the walk stops there)
        const int64_t stop = min(nwords, (v + (int64_t)max_values) / 32 + 2);
        end = stop < nwords ? (int64_t)1 << 62 : c.num_values;  // no start bit within reach: too long / the last doc
        for (int64_t j = tile * kMvBmWords + tid + 1; j < stop; ++j) {
          const uint32_t y = mv_bitmap_word(c, j);
          if (y) {
            end = j * 32 + __clz((int)y);
            break;
          }
        }
      }
      if (end - v > (int64_t)max_values) bad |= 8u;
    }
  }
  if (bad) atomicOr(flags, bad);
}

__global__ void __launch_bounds__(kBlock) mv_read_kernel(DevMvColumn c, int64_t ntiles, int32_t* offsets, int32_t* ids) {
  __shared__ uint32_t bm[kMvBmWords], pre[kMvBmWords], tot[2];
  const int64_t tile = blockIdx.x;
  if (tile >= ntiles) return;
  mv_stage_tile(c, tile, bm, pre, tot);
  const int64_t tfd = c.tile_first_doc[tile];
  if (tile == 0 && threadIdx.x == 0 && offsets) offsets[c.num_docs] = (int32_t)c.num_values;
#pragma unroll 4
  for (int j = 0; j < kMvPerThread; ++j) {
    const int vi = j * kBlock + (int)threadIdx.x;
    const int64_t v = tile * kMvTileValues + vi;
    if (v >= c.num_values) break;
    if (ids) ids[v] = (int32_t)mv_dict_id(c, v);
    if (offsets && ((bm[vi >> 5] >> (31 - (vi & 31))) & 1u)) {
      const int64_t d = tfd + (int64_t)mv_rank(bm, pre, vi) - 1;
      if (d >= 0 && d < c.num_docs) offsets[d] = (int32_t)v;
    }
  }
}

// the predicate's dictId set (DevMvSet): a dictId range, the 64-bit accept mask, or a bitmap staged in LDS once per
// block (read from HBM when it does not fit)
__global__ void __launch_bounds__(kBlock) mv_match_kernel(DevMvColumn c, DevMvSet s, int64_t ntiles, uint32_t* bitset) {
  extern __shared__ uint32_t lset[];
  __shared__ uint32_t bm[kMvBmWords], pre[kMvBmWords], tot[2], win[kMvWinWords];
  const int64_t tile = blockIdx.x;
  if (tile >= ntiles) return;
  const int tid = (int)threadIdx.x;
  if (s.mode == MV_SET_LDS)
    for (int i = tid; i < s.set_words; i += kBlock) lset[i] = s.set[i];
  for (int i = tid; i < kMvWinWords; i += kBlock) win[i] = 0u;
  mv_stage_tile(c, tile, bm, pre, tot);  // (its barriers also publish lset and win)
  const int64_t tfd = c.tile_first_doc[tile];
  // the tile's first doc: the straddling one unless the tile's first value starts a doc
  const int64_t dmin = max(tfd - 1 + (int64_t)(bm[0] >> 31), (int64_t)0);
  const int64_t wbase = dmin >> 5;
  const uint64_t accept = s.accept;
#pragma unroll 4
  for (int j = 0; j < kMvPerThread; ++j) {
    const int vi = j * kBlock + tid;
    const int64_t v = tile * kMvTileValues + vi;
    if (v >= c.num_values) break;
    const uint32_t id = mv_dict_id(c, v);
    bool hit;
    switch (s.mode) {
      case MV_SET_RANGE: hit = (int64_t)id >= s.lo && (int64_t)id < s.hi; break;
      case MV_SET_ACCEPT: hit = id < 64u && ((accept >> id) & 1ull); break;
      case MV_SET_LDS: hit = (int64_t)id < s.card && ((lset[id >> 5] >> (id & 31)) & 1u); break;
      default: hit = (int64_t)id < s.card && ((s.set[id >> 5] >> (id & 31)) & 1u); break;
    }
    if (!hit) continue;
    const int64_t d = tfd + (int64_t)mv_rank(bm, pre, vi) - 1;
    const int64_t w = (d >> 5) - wbase;
    if (d >= dmin && d < c.num_docs && w < kMvWinWords) atomicOr(&win[w], 1u << (d & 31));
  }
  __syncthreads();
  // boundary words are shared with the neighbouring tiles: OR, never store
  for (int i = tid; i < kMvWinWords; i += kBlock)
    if (win[i]) atomicOr(&bitset[wbase + i], win[i]);
}

__device__ __forceinline__ uint64_t mv_value_bits(const void* dict, int type, uint32_t id, bool as_double) {
  if (type == T_INT || type == T_LONG) {
    const int64_t x = type == T_INT ? (int64_t)reinterpret_cast<const int32_t*>(dict)[id]
                                    : reinterpret_cast<const int64_t*>(dict)[id];
    return as_double ? (uint64_t)__double_as_longlong((double)x) : (uint64_t)x;
  }
  const double x = type == T_FLOAT ? (double)reinterpret_cast<const float*>(dict)[id]
                                   : reinterpret_cast<const double*>(dict)[id];
  return (uint64_t)__double_as_longlong(x);
}

// One word per doc in out[num_docs], initialised by the host to the op's identity (0, MV_RED_MIN: ~0):
//   MV_RED_COUNT    the doc's values
//   MV_RED_SUM_I64  their exact (wrapping) int64 sum; INT / LONG columns
//   MV_RED_SUM_F64  the bits of their double sum, added in value order by the lane of the doc's first value
//   MV_RED_MIN/MAX  the order-preserving key of the least / greatest value (INT / LONG: value ^ 2^63, FLOAT / DOUBLE:
//                   Double.compare's key, NaN values skipped), the identity when no value entered
// A segmented reduction keyed by doc-in-tile in LDS; the tile's first and last doc may straddle into the
// neighbouring tiles and are flushed with global atomics, the docs between them stored.
__global__ void __launch_bounds__(kBlock) mv_reduce_kernel(DevMvColumn c, const void* dict, int type, int op,
                                                           int64_t ntiles, unsigned long long* out) {
  __shared__ uint32_t bm[kMvBmWords], pre[kMvBmWords], tot[2];
  __shared__ unsigned long long acc[kMvTileValues + 1];
  const int64_t tile = blockIdx.x;
  if (tile >= ntiles) return;
  const int tid = (int)threadIdx.x;
  const unsigned long long ident = op == MV_RED_MIN ? ~0ull : 0ull;
  for (int i = tid; i < kMvTileValues + 1; i += kBlock) acc[i] = ident;
  const uint32_t nstart = mv_stage_tile(c, tile, bm, pre, tot);
  const int64_t tfd = c.tile_first_doc[tile];
  const int64_t lead = 1 - (int64_t)(bm[0] >> 31);  // 1: the tile begins inside the straddling doc
  const int64_t dmin = tfd - lead;
  const int ndocs = (int)nstart + (int)lead;
  const bool fl = type == T_FLOAT || type == T_DOUBLE;
#pragma unroll 2
  for (int j = 0; j < kMvPerThread; ++j) {
    const int vi = j * kBlock + tid;
    const int64_t v = tile * kMvTileValues + vi;
    if (v >= c.num_values) break;
    const int64_t d = tfd + (int64_t)mv_rank(bm, pre, vi) - 1;
    if (d < 0 || d >= c.num_docs) continue;
    if (op == MV_RED_SUM_F64) {
      if (!((bm[vi >> 5] >> (31 - (vi & 31))) & 1u)) continue;
      double sum = 0.0;
      int64_t u = v;
      do {
        sum += __longlong_as_double((long long)mv_value_bits(dict, type, mv_dict_id(c, u), true));
        ++u;
      } while (u < c.num_values && !((__builtin_bswap32(c.words[c.bm_word0 + (u >> 5)]) >> (31 - (int)(u & 31))) & 1u));
      out[d] = (unsigned long long)__double_as_longlong(sum);
      continue;
    }
    unsigned long long* a = &acc[d - dmin];
    if (op == MV_RED_COUNT) {
      atomicAdd(a, 1ull);
      continue;
    }
    const uint64_t bits = mv_value_bits(dict, type, mv_dict_id(c, v), false);
    if (op == MV_RED_SUM_I64) {
      atomicAdd(a, (unsigned long long)bits);
      continue;
    }
    uint64_t key;
    if (fl) {
      const double x = __longlong_as_double((long long)bits);
      if (x != x) continue;  // value < min / value > max: NaN never enters
      key = java_double_order_dev(x);
    } else {
      key = bits ^ (1ull << 63);
    }
    if (op == MV_RED_MIN) atomicMin(a, (unsigned long long)key);
    else atomicMax(a, (unsigned long long)key);
  }
  if (op == MV_RED_SUM_F64) return;
  __syncthreads();
  for (int i = tid; i < ndocs; i += kBlock) {
    const unsigned long long x = acc[i];
    const int64_t d = dmin + i;
    if (d < 0 || d >= c.num_docs) continue;
    if (i > 0 && i < ndocs - 1) {
      out[d] = x;
    } else if (x != ident) {
      if (op == MV_RED_MIN) atomicMin(&out[d], x);
      else if (op == MV_RED_MAX) atomicMax(&out[d], x);
      else atomicAdd(&out[d], x);
    }
  }
}

// ------------------------------------------------------------------------------------------------
// DISTINCTCOUNTHLL twins (hll.h): per value the register index and the rank its hash sets
// (HyperLogLog.offer = offerHashed(MurmurHash.hash(boxed value))). One lane per value; the values of a raw column as
// staged (big-endian), a dictionary's as int64 / double in host order, a STRING dictionary's bytes and offsets as
// dict_regex_match_kernel reads them. INT and FLOAT hash the sign-extended 32 stored bits, LONG and DOUBLE the 64.
// ------------------------------------------------------------------------------------------------
template <int SRC>
__global__ void __launch_bounds__(256) hll_hash_kernel(const void* src_, const int32_t* offs_, int64_t n, int log2m,
                                                       int32_t* idx_, int32_t* rank_) {
  typedef __attribute__((address_space(1))) const uint32_t gu32;
  typedef __attribute__((address_space(1))) const uint64_t gu64;
  typedef __attribute__((address_space(1))) const uint8_t gu8;
  typedef __attribute__((address_space(1))) const int32_t gi32;
  typedef __attribute__((address_space(1))) int32_t go32;
  go32* idx = (go32*)idx_;
  go32* rank = (go32*)rank_;
  for (int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; d < n; d += (int64_t)gridDim.x * blockDim.x) {
    uint32_t h;
    if (SRC == HLL_SRC_BE32) {
      h = hll_hash_value(HLL_INT, (uint64_t)__builtin_bswap32(((gu32*)src_)[d]));
    } else if (SRC == HLL_SRC_BE64) {
      const uint32_t hi = ((gu32*)src_)[2 * d], lo = ((gu32*)src_)[2 * d + 1];
      h = hll_hash_value(HLL_LONG, ((uint64_t)__builtin_bswap32(hi) << 32) | __builtin_bswap32(lo));
    } else if (SRC == HLL_SRC_LE64) {
      h = hll_hash_value(HLL_LONG, ((gu64*)src_)[d]);
    } else if (SRC == HLL_SRC_LE64_F32) {  // a FLOAT dictionary's values held as doubles: back to the float's bits
      const float f = (float)__longlong_as_double((long long)((gu64*)src_)[d]);
      h = hll_hash_value(HLL_FLOAT, (uint64_t)__float_as_uint(f));
    } else {  // HLL_SRC_STRING: MurmurHash.hash(bytes, len, -1), the value ending at its first NUL
      gi32* offs = (gi32*)offs_;
      gu8* p = (gu8*)src_ + offs[d];
      const int32_t cap = offs[d + 1] - offs[d];
      int32_t len = 0;
      while (len < cap && p[len] != 0) ++len;
      h = hll_hash_bytes(p, len);
    }
    uint32_t j, r;
    hll_index_rank(h, log2m, &j, &r);
    idx[d] = (int32_t)j;
    rank[d] = (int32_t)r;
  }
}

// src: n values in the layout `src_kind` names (offs: the n + 1 byte offsets of HLL_SRC_STRING); idx / rank: n entries
hipError_t launch_hll_hash(const void* src, const int32_t* offs, int src_kind, int64_t n, int log2m, int32_t* idx,
                           int32_t* rank, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  if (log2m < kHllMinLog2m || log2m > kHllMaxLog2m || !src || !idx || !rank) return hipErrorInvalidValue;
  const dim3 g(grid_of(n)), b(256);
  switch (src_kind) {
    case HLL_SRC_BE32: hipLaunchKernelGGL(hll_hash_kernel<HLL_SRC_BE32>, g, b, 0, st, src, offs, n, log2m, idx, rank); break;
    case HLL_SRC_BE64: hipLaunchKernelGGL(hll_hash_kernel<HLL_SRC_BE64>, g, b, 0, st, src, offs, n, log2m, idx, rank); break;
    case HLL_SRC_LE64: hipLaunchKernelGGL(hll_hash_kernel<HLL_SRC_LE64>, g, b, 0, st, src, offs, n, log2m, idx, rank); break;
    case HLL_SRC_LE64_F32:
      hipLaunchKernelGGL(hll_hash_kernel<HLL_SRC_LE64_F32>, g, b, 0, st, src, offs, n, log2m, idx, rank);
      break;
    case HLL_SRC_STRING:
      if (!offs) return hipErrorInvalidValue;
      hipLaunchKernelGGL(hll_hash_kernel<HLL_SRC_STRING>, g, b, 0, st, src, offs, n, log2m, idx, rank);
      break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

__global__ void fill_u64_kernel(unsigned long long* p, int64_t n, unsigned long long x) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) p[i] = x;
}

int64_t mv_num_tiles(int64_t num_values) { return (num_values + kMvTileValues - 1) / kMvTileValues; }

hipError_t launch_mv_index(const DevMvColumn& c, int32_t* tile_first_doc, long long* total, hipStream_t st) {
  const int64_t nt = mv_num_tiles(c.num_values);
  if (nt > 0) hipLaunchKernelGGL(mv_tile_count_kernel, dim3((unsigned)nt), dim3(kBlock), 0, st, c, nt, tile_first_doc);
  hipLaunchKernelGGL(mv_tile_scan_kernel, dim3(1), dim3(kBlock), 0, st, tile_first_doc, nt, total);
  return hipGetLastError();
}
hipError_t launch_mv_validate(const DevMvColumn& c, int32_t docs_per_chunk, int32_t num_chunks, int32_t max_values,
                              uint32_t* flags, hipStream_t st) {
  const int64_t nt = mv_num_tiles(c.num_values);
  if (nt <= 0) return hipSuccess;
  hipLaunchKernelGGL(mv_validate_kernel, dim3((unsigned)nt), dim3(kBlock), 0, st, c, nt, docs_per_chunk, num_chunks,
                     max_values, flags);
  return hipGetLastError();
}
hipError_t launch_mv_read(const DevMvColumn& c, int32_t* offsets, int32_t* ids, hipStream_t st) {
  const int64_t nt = mv_num_tiles(c.num_values);
  if (nt <= 0) return hipSuccess;
  hipLaunchKernelGGL(mv_read_kernel, dim3((unsigned)nt), dim3(kBlock), 0, st, c, nt, offsets, ids);
  return hipGetLastError();
}
hipError_t launch_mv_match(const DevMvColumn& c, const DevMvSet& s, uint32_t* bitset, hipStream_t st) {
  const int64_t nt = mv_num_tiles(c.num_values);
  if (nt <= 0) return hipSuccess;
  const size_t lds = s.mode == MV_SET_LDS ? (size_t)s.set_words * 4 : 0;
  hipLaunchKernelGGL(mv_match_kernel, dim3((unsigned)nt), dim3(kBlock), lds, st, c, s, nt, bitset);
  return hipGetLastError();
}
hipError_t launch_mv_reduce(const DevMvColumn& c, const void* dict, int type, int op, unsigned long long* out,
                            hipStream_t st) {
  const int64_t nt = mv_num_tiles(c.num_values);
  if (c.num_docs > 0)
    hipLaunchKernelGGL(fill_u64_kernel, dim3(grid_of(c.num_docs)), dim3(256), 0, st, out, c.num_docs,
                       op == MV_RED_MIN ? ~0ull : 0ull);
  if (nt <= 0) return hipGetLastError();
  hipLaunchKernelGGL(mv_reduce_kernel, dim3((unsigned)nt), dim3(kBlock), 0, st, c, dict, type, op, nt, out);
  return hipGetLastError();
}

}  // namespace pamd
