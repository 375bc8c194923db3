// A stand-alone driver of pinot_amd/csrc/regex_dfa.cpp for tests/test_regex_dfa_cpu.py (built with the host compiler
// under -fsanitize=address,undefined). Commands on stdin, one per line, fields hex-encoded UTF-8 ("-" = empty):
//   P <0|1> <pattern>   compile (1: case-insensitive)   -> "OK <states> <classes>" | "ERR <code> <message>"
//   S <subject>         match against the last pattern  -> "1" | "0"   ("X" when the last compile failed)
//   L <like pattern>    likeToRegexpLike                -> the hex-encoded regex
#include <stdio.h>

#include <iostream>
#include <string>

#include "../pinot_amd/csrc/regex_dfa.h"

static std::string unhex(const std::string& h) {
  std::string out;
  if (h == "-") return out;
  for (size_t i = 0; i + 1 < h.size(); i += 2) out += (char)std::stoi(h.substr(i, 2), nullptr, 16);
  return out;
}
static std::string hex(const std::string& s) {
  if (s.empty()) return "-";
  static const char* d = "0123456789abcdef";
  std::string out;
  for (unsigned char c : s) {
    out += d[c >> 4];
    out += d[c & 15];
  }
  return out;
}

int main() {
  pamd_regex::Dfa dfa;
  bool have = false;
  std::string line;
  while (std::getline(std::cin, line)) {
    if (line.empty()) continue;
    if (line[0] == 'P') {
      const bool ci = line[2] == '1';
      std::string err;
      const int rc = pamd_regex::compile(unhex(line.substr(4)), ci, &dfa, &err);
      have = rc == pamd_regex::kOk;
      if (have) printf("OK %d %d\n", dfa.num_states, dfa.num_classes);
      else printf("ERR %d %s\n", rc, err.c_str());
    } else if (line[0] == 'S') {
      const std::string s = unhex(line.substr(2));
      if (!have) printf("X\n");
      else printf("%d\n", pamd_regex::match(dfa, s.data(), s.size()) ? 1 : 0);
    } else if (line[0] == 'L') {
      printf("%s\n", hex(pamd_regex::like_to_regexp(unhex(line.substr(2)))).c_str());
    }
  }
  return 0;
}
