// Stand-alone driver over pinot_amd/csrc/hll.h for tests/test_hll_cpu.py: requests on stdin, answers on stdout.
//   V <kind> <log2m> <bits, hex>    a value of kind 0 INT / 1 LONG / 2 FLOAT / 3 DOUBLE by its stored bits
//   S <log2m> <UTF-8 bytes, hex | ->  a STRING value
//     -> "<hash> <register> <rank>"
//   E <log2m> <registers, hex>      -> "<estimate>"
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../pinot_amd/csrc/hll.h"

static std::vector<uint8_t> unhex(const std::string& h) {
  std::vector<uint8_t> out;
  if (h == "-") return out;
  for (size_t i = 0; i + 1 < h.size(); i += 2) out.push_back((uint8_t)strtoul(h.substr(i, 2).c_str(), nullptr, 16));
  return out;
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string op;
    in >> op;
    if (op == "V" || op == "S") {
      int kind = pamd::HLL_STRING, log2m = 0;
      std::string arg;
      if (op == "V") in >> kind;
      in >> log2m >> arg;
      uint32_t h;
      if (op == "S") {
        const std::vector<uint8_t> b = unhex(arg);
        h = pamd::hll_hash_bytes(b.data(), (int32_t)b.size());
      } else {
        h = pamd::hll_hash_value(kind, strtoull(arg.c_str(), nullptr, 16));
      }
      uint32_t idx, rank;
      pamd::hll_index_rank(h, log2m, &idx, &rank);
      printf("%u %u %u\n", h, idx, rank);
    } else if (op == "E") {
      int log2m = 0;
      std::string arg;
      in >> log2m >> arg;
      const std::vector<uint8_t> regs = unhex(arg);
      if (regs.size() != (size_t)1 << log2m) {
        printf("bad\n");
        continue;
      }
      uint64_t S, zeros;
      pamd::hll_sum_zeros(regs.data(), log2m, &S, &zeros);
      printf("%lld\n", (long long)pamd::hll_estimate(S, zeros, log2m));
    } else if (!op.empty()) {
      printf("bad\n");
    }
  }
  return 0;
}
