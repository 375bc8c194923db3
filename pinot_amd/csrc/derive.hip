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

}  // namespace pamd
