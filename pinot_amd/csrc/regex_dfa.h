// regex_dfa.h — REGEXP_LIKE / LIKE patterns compiled to one DFA table that two runners walk: match() on the host and
// dict_regex_match_kernel on the device. No HIP dependency: this translation unit also builds with
// the plain host compiler (tests/test_regex_dfa_cpu.py runs it under the address and undefined-behaviour sanitizers).
//
// The engine restated is java.util.regex as Pinot's JavaUtilPattern uses it: flags 0, or CASE_INSENSITIVE |
// UNICODE_CASE, and Matcher.find() (an unanchored partial match). A pattern is answered exactly as that engine would
// answer it or refused by name; compile() never approximates.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

namespace pamd_regex {

// Caps. The device runner keeps the 256-byte class map and the table (uint16 entries) in LDS: at most 64 KiB together.
constexpr int kMaxDfaStates = 4096;      // rows of the table
constexpr int kMaxTableEntries = 32512;  // rows x classes: 256 B + 2 x 32512 B = 63.75 KiB
constexpr int kMaxNfaStates = 1 << 16;   // Thompson states after the counted repetitions are unrolled
constexpr int kMaxRepeat = 1 << 15;      // n and m of {n}, {n,}, {n,m}

// compile() results
enum : int { kOk = 0, kInvalid = 1 /* not a pattern of the reference engine either */, kUnsupported = 2 /* refused */ };

// A DFA over byte equivalence classes. Table entries are ROW OFFSETS (state x num_classes), so a step is
// row = table[row + class_of[byte]]. Row 0 is the dead state, row num_classes the accepting sink; both loop to
// themselves. The last class, end_class(), is the virtual end-of-input symbol: a runner steps once on it after the
// last byte (this is how '$' and "no match by the end" are decided). The unanchored search is part of the automaton.
struct Dfa {
  uint8_t class_of[256];
  int32_t num_classes = 0;  // byte classes + 1
  int32_t num_states = 0;
  uint16_t start = 0;  // row offset of the start state
  std::vector<uint16_t> table;
  uint16_t dead() const { return 0; }
  uint16_t accept() const { return (uint16_t)num_classes; }
  int end_class() const { return num_classes - 1; }
  size_t lds_bytes() const { return 256 + table.size() * sizeof(uint16_t); }
};

// pattern: UTF-8. err names the refused construct. Returns kOk, kInvalid or kUnsupported.
int compile(const std::string& pattern, bool case_insensitive, Dfa* out, std::string* err);

// the host runner: the subject's bytes (no terminator needed)
bool match(const Dfa& d, const char* s, size_t n);

// RegexpPatternConverterUtils.likeToRegexpLike
std::string like_to_regexp(const std::string& like);

}  // namespace pamd_regex
