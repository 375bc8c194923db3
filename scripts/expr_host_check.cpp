// expr_host_check.cpp — pinot_amd/csrc/expr.h as a stand-alone host program (no GPU, no HIP), for sanitizer runs of
// the expression validation / canonicalisation code and of the generated value functions built as host C++
// (scripts/expr_host_check.py drives it).
//
//   expr_host_check names  < specs     per line: "ok <name>" or "refused <1 EINVAL | 2 EUNSUPPORTED> <message>"
//   expr_host_check host   < specs     a C++ program evaluating every accepted spec (see below)
//   expr_host_check kernel <spec> <enc.type.bits>...   the device evaluator's source for those source shapes
//
// A spec is one line of postfix tokens: c:<column>  l:<16 hex digits of the double>  <kind number>:<num_args>.
// The program `host` prints reads lines "<spec index> <hex bits of c0> <hex bits of c1> ..." and answers each with
// the hex bits of the value (NaN as 7ff8000000000000).
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../pinot_amd/csrc/expr.h"

using namespace pamd;

static int parse_spec(const std::string& line, ExprDef* d, std::string* msg) {
  std::vector<ExprNodeIn> in;
  std::vector<std::string> names;
  std::istringstream ss(line);
  std::string tok;
  std::vector<std::string> toks;
  while (ss >> tok) toks.push_back(tok);
  names.reserve(toks.size());
  for (const std::string& t : toks) {
    const size_t colon = t.find(':');
    if (colon == std::string::npos) {
      *msg = "bad token " + t;
      return XV_EINVAL;
    }
    const std::string head = t.substr(0, colon), rest = t.substr(colon + 1);
    ExprNodeIn n{0, 0, nullptr, 0.0};
    if (head == "c") {
      names.push_back(rest);
      n.kind = X_COLUMN;
      n.column = names.back().c_str();
    } else if (head == "l") {
      const uint64_t b = strtoull(rest.c_str(), nullptr, 16);
      n.kind = X_LITERAL;
      memcpy(&n.literal, &b, 8);
    } else {
      n.kind = atoi(head.c_str());
      n.num_args = atoi(rest.c_str());
    }
    in.push_back(n);
  }
  return expr_canonicalize(in.data(), (int)in.size(), d, msg);
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "kernel" && argc >= 3) {
    ExprDef d;
    std::string msg;
    if (int v = parse_spec(argv[2], &d, &msg)) {
      fprintf(stderr, "refused %d %s\n", v, msg.c_str());
      return 1;
    }
    std::vector<ExprSrcShape> shapes;
    for (int i = 3; i < argc; ++i) {
      ExprSrcShape s;
      if (sscanf(argv[i], "%d.%d.%d", &s.enc, &s.type, &s.bits) != 3) return 2;
      shapes.push_back(s);
    }
    if (shapes.size() != d.cols.size()) {
      fprintf(stderr, "%zu source shapes for %zu columns\n", shapes.size(), d.cols.size());
      return 2;
    }
    printf("// %s\n%s", expr_kernel_key(d, shapes).c_str(), expr_kernel_source(d, shapes).c_str());
    return 0;
  }
  if (mode != "names" && mode != "host") {
    fprintf(stderr, "usage: expr_host_check names|host < specs, or kernel <spec> <enc.type.bits>...\n");
    return 2;
  }
  std::vector<ExprDef> defs;
  std::string line;
  while (std::getline(std::cin, line)) {
    if (line.empty()) continue;
    ExprDef d;
    std::string msg;
    const int v = parse_spec(line, &d, &msg);
    if (mode == "names") {
      if (v) printf("refused %d %s\n", v, msg.c_str());
      else printf("ok %s\n", d.name.c_str());
    }
    if (!v) defs.push_back(d);
  }
  if (mode == "names") return 0;
  printf("#include <cmath>\n#include <cstdio>\n#include <cstdlib>\n#include <cstring>\n#include <iostream>\n"
         "#include <sstream>\n#include <string>\n"
         "static inline double x_lit(unsigned long long b) { double d; memcpy(&d, &b, 8); return d; }\n"
         "static inline unsigned long long x_bits(double d) { unsigned long long b; memcpy(&b, &d, 8); return b; }\n"
         "#define XFN static inline\n#define XLIT(b) x_lit(b)\n#define XBITS(x) x_bits(x)\n%s",
         kExprPrelude);
  for (size_t i = 0; i < defs.size(); ++i) {
    printf("namespace e%zu {\n%s}\nstatic double f%zu(const double* c) { return e%zu::pinot_expr_value(", i,
           expr_value_function(defs[i]).c_str(), i, i);
    for (size_t k = 0; k < defs[i].cols.size(); ++k) printf("%sc[%zu]", k ? ", " : "", k);
    printf("); }\n");
  }
  printf("typedef double (*Fn)(const double*);\nstatic const Fn fns[] = {");
  for (size_t i = 0; i < defs.size(); ++i) printf("f%zu, ", i);
  printf("};\nstatic const int ncols[] = {");
  for (size_t i = 0; i < defs.size(); ++i) printf("%zu, ", defs[i].cols.size());
  printf("};\nint main() {\n  std::string line;\n  while (std::getline(std::cin, line)) {\n"
         "    std::istringstream ss(line);\n    size_t i;\n    if (!(ss >> i) || i >= sizeof(fns) / sizeof(fns[0])) return 2;\n"
         "    double c[8] = {0};\n    for (int k = 0; k < ncols[i]; ++k) {\n      std::string h;\n      if (!(ss >> h)) return 2;\n"
         "      c[k] = x_lit(strtoull(h.c_str(), nullptr, 16));\n    }\n    const double r = fns[i](c);\n"
         "    printf(\"%%016llx\\n\", r != r ? 0x7ff8000000000000ull : x_bits(r));\n  }\n  return 0;\n}\n");
  return 0;
}
