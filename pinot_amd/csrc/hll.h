// hll.h — DISTINCTCOUNTHLL (DistinctCountHLLAggregationFunction.java over stream-lib's HyperLogLog and MurmurHash):
// the one restatement of the hashes, the register update and the estimator that the device kernels (derive.hip), the
// host (host.cpp) and a stand-alone checker share. Plain C++ with no HIP header: a device
// translation unit defines PAMD_HLL_HD as `__host__ __device__` before including it.
//
// All hash arithmetic is Java `int`: 32 bits, wrapping (computed unsigned here), `>>>` logical.
#pragma once
#include <stdint.h>

#ifndef PAMD_HLL_HD
#define PAMD_HLL_HD
#define PAMD_HLL_HOST_ONLY 1
#include <cmath>
#include <cstring>
#endif

namespace pamd {

constexpr int kHllMinLog2m = 4, kHllMaxLog2m = 16, kHllDefaultLog2m = 8;  // DEFAULT_HYPERLOGLOG_LOG2M = 8

// MurmurHash.hashLong(long)
PAMD_HLL_HD inline uint32_t hll_hash_long(int64_t d) {
  const uint32_t m = 0x5bd1e995u;
  uint32_t h = 0;
  uint32_t k = (uint32_t)(uint64_t)d * m;
  k ^= k >> 24;
  h ^= k * m;
  k = (uint32_t)((uint64_t)d >> 32) * m;  // (int) (d >> 32): the high word, whatever the shift's sign fill
  k ^= k >> 24;
  h *= m;
  h ^= k * m;
  h ^= h >> 13;
  h *= m;
  h ^= h >> 15;
  return h;
}

// MurmurHash.hash(byte[] data, int length, int seed), seed = -1 for hash(Object) of a String's / byte[]'s bytes. The
// tail bytes are Java bytes widened to int: sign-extended, no mask.
// (Bytes: any pointer to bytes; a kernel passes a global-address-space one)
template <class Bytes>
PAMD_HLL_HD inline uint32_t hll_hash_bytes(Bytes data, int32_t len, uint32_t seed = 0xffffffffu) {
  const uint32_t m = 0x5bd1e995u;
  uint32_t h = seed ^ (uint32_t)len;
  const int32_t len4 = len >> 2;
  for (int32_t i = 0; i < len4; ++i) {
    const int32_t i4 = i << 2;
    uint32_t k = ((uint32_t)data[i4 + 3] << 24) | ((uint32_t)data[i4 + 2] << 16) | ((uint32_t)data[i4 + 1] << 8) |
                 (uint32_t)data[i4];
    k *= m;
    k ^= k >> 24;
    k *= m;
    h *= m;
    h ^= k;
  }
  const int32_t left = len & 3;
  if (left != 0) {
    if (left >= 3) h ^= (uint32_t)(int32_t)(int8_t)data[len - 3] << 16;
    if (left >= 2) h ^= (uint32_t)(int32_t)(int8_t)data[len - 2] << 8;
    if (left >= 1) h ^= (uint32_t)(int32_t)(int8_t)data[len - 1];
    h *= m;
  }
  h ^= h >> 13;
  h *= m;
  h ^= h >> 15;
  return h;
}

// MurmurHash.hash(Object) of the boxed value of a column, from the value's stored bits:
//   INT     hashLong((long) v)                            bits: the int, zero- or sign-extended (the low 32 are read)
//   LONG    hashLong(v)
//   FLOAT   hashLong((long) Float.floatToRawIntBits(f))   bits: the float's 32 bits
//   DOUBLE  hashLong(Double.doubleToRawLongBits(d))       bits: the double's 64 bits
// kind: 0 INT, 1 LONG, 2 FLOAT, 3 DOUBLE (the stored types' order)
enum { HLL_INT = 0, HLL_LONG = 1, HLL_FLOAT = 2, HLL_DOUBLE = 3, HLL_STRING = 4 };
PAMD_HLL_HD inline uint32_t hll_hash_value(int kind, uint64_t bits) {
  if (kind == HLL_INT || kind == HLL_FLOAT) return hll_hash_long((int64_t)(int32_t)(uint32_t)bits);
  return hll_hash_long((int64_t)bits);
}

// HyperLogLog.offerHashed(int): the register and the rank a hash sets (reg[idx] = max(reg[idx], rank));
// 1 <= rank <= 33 - log2m. (`+` binds tighter than `|` in the library's expression.)
PAMD_HLL_HD inline void hll_index_rank(uint32_t x, int log2m, uint32_t* idx, uint32_t* rank) {
  *idx = x >> (32 - log2m);
  const uint32_t w = (x << log2m) | ((1u << (log2m - 1)) + 1u);
  *rank = (uint32_t)__builtin_clz(w) + 1u;  // Integer.numberOfLeadingZeros (w != 0: its bit 0 is set)
}

#ifdef PAMD_HLL_HOST_ONLY
// HyperLogLog.cardinality() from S = sum over the registers of 2^(32 - reg[j]) (so that sum = S / 2^32 exactly: every
// term of the library's double sum is a multiple of 2^-25 and the total is at most 2^16, exact in any order) and the
// number of zero registers. Math.round(+inf) = Long.MAX_VALUE when the small-range branch meets zeros == 0.
inline int64_t hll_estimate(uint64_t S, uint64_t zeros, int log2m) {
  const double m = (double)(1u << log2m);
  if (zeros == (uint64_t)(1u << log2m)) return 0;  // every term 1.0: the formula below gives m * log(1) = 0 too
  const double sum = (double)S / 4294967296.0;
  double alpha_mm;
  switch (log2m) {
    case 4: alpha_mm = 0.673 * m * m; break;
    case 5: alpha_mm = 0.697 * m * m; break;
    case 6: alpha_mm = 0.709 * m * m; break;
    default: alpha_mm = (0.7213 / (1.0 + 1.079 / m)) * m * m; break;
  }
  const double estimate = alpha_mm * (1.0 / sum);
  double v = estimate;
  if (estimate <= 2.5 * m) {
    if (zeros == 0) return INT64_MAX;
    v = m * std::log(m / (double)zeros);
  }
  return (int64_t)std::floor(v + 0.5);  // Math.round of a finite value far inside long's range
}

// the estimator's inputs from a register array (one byte per register)
inline void hll_sum_zeros(const uint8_t* regs, int log2m, uint64_t* S, uint64_t* zeros) {
  uint64_t s = 0, z = 0;
  for (uint32_t j = 0; j < (1u << log2m); ++j) {
    s += (uint64_t)1 << (32 - regs[j]);
    z += regs[j] == 0;
  }
  *S = s;
  *zeros = z;
}
#endif

}  // namespace pamd
