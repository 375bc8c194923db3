// expr.h — arithmetic expressions (pinot_amd_query_define_expression): validation and canonical form of a postfix
// tree, the name of its virtual column, and the generated source of its evaluator. Host C++ only (no HIP): the
// same text builds into libpinot_amd.so and into a stand-alone checker.
//
// Every node's value is a Java double. Canonical form: the tree in postfix with
//   * ADD / MULT: the non-literal arguments in order, then ONE literal -- 0.0 + (the literal arguments, in order) or
//     1.0 * (them) -- as the last argument (AdditionTransformFunction / MultiplicationTransformFunction hoist their
//     literals at init and start the per-doc fold from that sum / product);
//   * every other node as given.
// Two trees are the same expression iff their canonical forms are equal (operators, columns, literal bits; every
// NaN literal is one value).
#pragma once
#include <stdint.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace pamd {

constexpr int kMaxExprNodes = 32;
constexpr int kMaxExprSrc = 8;

// pinot_amd_xnode_kind
enum {
  X_COLUMN = 0, X_LITERAL, X_ADD, X_SUB, X_MULT, X_DIV, X_MOD, X_ABS, X_CEIL, X_FLOOR, X_SQRT, X_SIGN, X_LEAST,
  X_GREATEST, X_KINDS
};
// expr_canonicalize's verdicts (the caller maps them to PINOT_AMD_EINVAL / PINOT_AMD_EUNSUPPORTED)
enum { XV_OK = 0, XV_EINVAL = 1, XV_EUNSUPPORTED = 2 };

struct ExprNodeIn {  // one node of the caller's postfix (pinot_amd_xnode)
  int32_t kind, num_args;
  const char* column;
  double literal;
};
struct ExprNode {
  int kind = 0, nargs = 0;
  int src = -1;      // X_COLUMN: index into ExprDef::cols
  double lit = 0.0;  // X_LITERAL
};
struct ExprDef {
  std::vector<ExprNode> nodes;    // canonical postfix
  std::vector<std::string> cols;  // distinct source columns in first-use order
  std::string name;               // the virtual column's name
};

inline const char* expr_kind_name(int k) {
  static const char* const names[] = {"column", "literal", "add", "sub", "mult", "div", "mod", "abs", "ceil", "floor",
                                      "sqrt", "sign", "least", "greatest"};
  return k >= 0 && k < X_KINDS ? names[k] : "?";
}

inline uint64_t expr_lit_bits(double v) {
  uint64_t b;
  if (v != v) return 0x7ff8000000000000ull;
  memcpy(&b, &v, 8);
  return b;
}

namespace expr_detail {
struct Tree {
  int kind = 0;
  int src = -1;
  double lit = 0.0;
  std::vector<int> kids;
};
inline void emit(const std::vector<Tree>& t, int i, std::vector<ExprNode>* out) {
  const Tree& n = t[(size_t)i];
  if (n.kind == X_COLUMN || n.kind == X_LITERAL) {
    ExprNode e;
    e.kind = n.kind;
    e.src = n.src;
    e.lit = n.lit;
    out->push_back(e);
    return;
  }
  int nargs = 0;
  if (n.kind == X_ADD || n.kind == X_MULT) {
    double acc = n.kind == X_ADD ? 0.0 : 1.0;
    for (int k : n.kids)
      if (t[(size_t)k].kind == X_LITERAL) acc = n.kind == X_ADD ? acc + t[(size_t)k].lit : acc * t[(size_t)k].lit;
    for (int k : n.kids)
      if (t[(size_t)k].kind != X_LITERAL) {
        emit(t, k, out);
        ++nargs;
      }
    ExprNode l;
    l.kind = X_LITERAL;
    l.lit = acc;
    out->push_back(l);
    ++nargs;
  } else {
    for (int k : n.kids) {
      emit(t, k, out);
      ++nargs;
    }
  }
  ExprNode e;
  e.kind = n.kind;
  e.nargs = nargs;
  out->push_back(e);
}
}  // namespace expr_detail

// The canonical form of a postfix tree, or why it is refused (*msg).
inline int expr_canonicalize(const ExprNodeIn* in, int n, ExprDef* out, std::string* msg) {
  using expr_detail::Tree;
  char b[256];
  if (!in || n < 1) {
    *msg = "define_expression: no nodes";
    return XV_EINVAL;
  }
  if (n > kMaxExprNodes) {
    snprintf(b, sizeof(b), "define_expression: %d nodes (at most %d)", n, kMaxExprNodes);
    *msg = b;
    return XV_EINVAL;
  }
  std::vector<Tree> t;
  std::vector<int> stack;
  std::vector<std::string> cols;
  for (int i = 0; i < n; ++i) {
    const ExprNodeIn& x = in[i];
    Tree node;
    node.kind = x.kind;
    if (x.kind < 0 || x.kind >= X_KINDS) {
      snprintf(b, sizeof(b), "define_expression: node %d: function kind %d is not supported (add sub mult div mod abs ceil "
                             "floor sqrt sign least greatest only)", i, x.kind);
      *msg = b;
      return XV_EUNSUPPORTED;
    }
    if (x.kind == X_COLUMN) {
      if (!x.column || !*x.column) {
        snprintf(b, sizeof(b), "define_expression: node %d: a column node needs a name", i);
        *msg = b;
        return XV_EINVAL;
      }
      size_t s = 0;
      while (s < cols.size() && cols[s] != x.column) ++s;
      if (s == cols.size()) {
        if ((int)cols.size() >= kMaxExprSrc) {
          snprintf(b, sizeof(b), "define_expression: more than %d distinct columns", kMaxExprSrc);
          *msg = b;
          return XV_EINVAL;
        }
        cols.push_back(x.column);
      }
      node.src = (int)s;
    } else if (x.kind == X_LITERAL) {
      node.lit = x.literal;
    } else {
      const int k = x.num_args;
      const bool nary = x.kind == X_ADD || x.kind == X_MULT || x.kind == X_LEAST || x.kind == X_GREATEST;
      const bool binary = x.kind == X_SUB || x.kind == X_DIV || x.kind == X_MOD;
      if (nary ? k < 2 : binary ? k != 2 : k != 1) {
        snprintf(b, sizeof(b), "define_expression: node %d: %s takes %s, not %d", i, expr_kind_name(x.kind),
                 nary ? "two or more arguments" : binary ? "two arguments" : "one argument", k);
        *msg = b;
        return XV_EINVAL;
      }
      if ((int)stack.size() < k) {
        snprintf(b, sizeof(b), "define_expression: node %d: %s pops %d arguments, the postfix holds %zu", i,
                 expr_kind_name(x.kind), k, stack.size());
        *msg = b;
        return XV_EINVAL;
      }
      node.kids.assign(stack.end() - k, stack.end());
      stack.resize(stack.size() - (size_t)k);
      if (!nary && !binary && t[(size_t)node.kids[0]].kind == X_LITERAL) {
        snprintf(b, sizeof(b), "define_expression: node %d: %s of a literal", i, expr_kind_name(x.kind));
        *msg = b;
        return XV_EINVAL;
      }
    }
    stack.push_back((int)t.size());
    t.push_back(node);
  }
  if (stack.size() != 1) {
    snprintf(b, sizeof(b), "define_expression: the postfix leaves %zu values, not one", stack.size());
    *msg = b;
    return XV_EINVAL;
  }
  if (cols.empty()) {
    *msg = "define_expression: an expression without a column";
    return XV_EINVAL;
  }
  out->nodes.clear();
  expr_detail::emit(t, stack[0], &out->nodes);
  // sources renumbered in the canonical order of first use
  out->cols.clear();
  for (ExprNode& e : out->nodes) {
    if (e.kind != X_COLUMN) continue;
    const std::string& c = cols[(size_t)e.src];
    size_t s = 0;
    while (s < out->cols.size() && out->cols[s] != c) ++s;
    if (s == out->cols.size()) out->cols.push_back(c);
    e.src = (int)s;
  }
  if ((int)out->nodes.size() > 2 * kMaxExprNodes) {  // (the hoisted literals add at most one node per ADD / MULT)
    *msg = "define_expression: too many nodes";
    return XV_EINVAL;
  }
  // the name: "$x(" + the canonical postfix + ")" -- '$' keeps it apart from every real column
  std::string nm = "$x(";
  for (size_t i = 0; i < out->nodes.size(); ++i) {
    const ExprNode& e = out->nodes[i];
    if (i) nm += ' ';
    if (e.kind == X_COLUMN) {
      nm += "c" + std::to_string(out->cols[(size_t)e.src].size()) + ":" + out->cols[(size_t)e.src];
    } else if (e.kind == X_LITERAL) {
      snprintf(b, sizeof(b), "l%016llx", (unsigned long long)expr_lit_bits(e.lit));
      nm += b;
    } else {
      nm += std::string(expr_kind_name(e.kind)) + std::to_string(e.nargs);
    }
  }
  out->name = nm + ")";
  return XV_OK;
}

// the tree without its column names (sources by index): the evaluator kernel's identity beside the sources' shapes
inline std::string expr_shape(const ExprDef& d) {
  std::string s;
  char b[32];
  for (const ExprNode& e : d.nodes) {
    if (e.kind == X_COLUMN) snprintf(b, sizeof(b), "c%d ", e.src);
    else if (e.kind == X_LITERAL) snprintf(b, sizeof(b), "l%016llx ", (unsigned long long)expr_lit_bits(e.lit));
    else snprintf(b, sizeof(b), "%s%d ", expr_kind_name(e.kind), e.nargs);
    s += b;
  }
  return s;
}

// Helpers of the generated value function. The including text defines XFN (the function qualifiers), XLIT(bits)
// (a double from its bit pattern) and XBITS(x) (the pattern of a double). Contraction is off: a fused multiply-add
// rounds once where Java rounds twice.
static const char* const kExprPrelude = R"PINOTX(
#pragma clang fp contract(off)
XFN double x_min(double a, double b) {  // Math.min: NaN propagates, -0.0 < 0.0
  if (a != a) return a;
  if (a == 0.0 && b == 0.0 && XBITS(b) == 0x8000000000000000ull) return b;
  return a <= b ? a : b;
}
XFN double x_max(double a, double b) {  // Math.max
  if (a != a) return a;
  if (a == 0.0 && b == 0.0 && XBITS(a) == 0x8000000000000000ull) return b;
  return a >= b ? a : b;
}
XFN double x_sign(double a) { return a > 0.0 ? 1.0 : a < 0.0 ? -1.0 : a; }  // Math.signum: +-0 and NaN are themselves
)PINOTX";

// `XFN double pinot_expr_value(double c0, ...)`: straight-line code, one local per node, in the reference's order
// of evaluation
inline std::string expr_value_function(const ExprDef& d) {
  std::string s = "XFN double pinot_expr_value(";
  for (size_t i = 0; i < d.cols.size(); ++i) s += (i ? ", double c" : "double c") + std::to_string(i);
  s += ") {\n";
  std::vector<std::string> stack;
  char b[96];
  int tmp = 0;
  for (const ExprNode& e : d.nodes) {
    if (e.kind == X_COLUMN) {
      stack.push_back("c" + std::to_string(e.src));
      continue;
    }
    if (e.kind == X_LITERAL) {
      snprintf(b, sizeof(b), "XLIT(0x%016llxull)", (unsigned long long)expr_lit_bits(e.lit));
      stack.push_back(b);
      continue;
    }
    const std::vector<std::string> a(stack.end() - e.nargs, stack.end());
    stack.resize(stack.size() - (size_t)e.nargs);
    const std::string t = "t" + std::to_string(tmp++);
    switch (e.kind) {
      case X_ADD:
      case X_MULT: {  // from the hoisted literal (the last argument), then each argument in order
        const char* op = e.kind == X_ADD ? " + " : " * ";
        s += "  double " + t + " = " + a.back() + ";\n";
        for (size_t k = 0; k + 1 < a.size(); ++k) s += "  " + t + " = " + t + op + a[k] + ";\n";
        break;
      }
      case X_SUB: s += "  const double " + t + " = " + a[0] + " - " + a[1] + ";\n"; break;
      case X_DIV: s += "  const double " + t + " = " + a[0] + " / " + a[1] + ";\n"; break;
      case X_MOD: s += "  const double " + t + " = fmod(" + a[0] + ", " + a[1] + ");\n"; break;
      case X_ABS: s += "  const double " + t + " = fabs(" + a[0] + ");\n"; break;
      case X_CEIL: s += "  const double " + t + " = ceil(" + a[0] + ");\n"; break;
      case X_FLOOR: s += "  const double " + t + " = floor(" + a[0] + ");\n"; break;
      case X_SQRT: s += "  const double " + t + " = sqrt(" + a[0] + ");\n"; break;
      case X_SIGN: s += "  const double " + t + " = x_sign(" + a[0] + ");\n"; break;
      default: {  // X_LEAST / X_GREATEST: a left fold
        const char* f = e.kind == X_LEAST ? "x_min(" : "x_max(";
        s += "  double " + t + " = " + a[0] + ";\n";
        for (size_t k = 1; k < a.size(); ++k) s += "  " + t + " = " + f + t + ", " + a[k] + ");\n";
        break;
      }
    }
    stack.push_back(t);
  }
  s += "  return " + stack.back() + ";\n}\n";
  return s;
}

// One source column as the evaluator reads it in a segment
struct ExprSrcShape {
  int enc = 0;   // ENC_FIXED_BIT 0 | ENC_RAW 1 | ENC_SORTED 2
  int type = 0;  // T_INT 0 | T_LONG 1 | T_FLOAT 2 | T_DOUBLE 3
  int bits = 0;  // fixed-bit width, 1..31
};

// The evaluator kernel `pinot_expr_eval(f0, d0, card0, ..., out, num_docs, tiles)`: 256-thread blocks stride over
// 1024-doc tiles, each lane owns 4 consecutive docs -- a raw source is one or two 16-byte loads, a fixed-bit one a
// 5-dword window of the bit stream and 4 dictionary reads, a sorted one a binary search over the first-docId array
// and a linear advance -- and writes 4 big-endian doubles (two 16-byte stores; the docs of the last, partial lane
// one by one, so the staged padding stays zero). Reads past the last doc stay inside the sources' staging padding.
inline std::string expr_kernel_source(const ExprDef& d, const std::vector<ExprSrcShape>& src) {
  std::string s;
  s += "#define XFN static __device__ __forceinline__\n"
       "#define XLIT(b) __longlong_as_double((long long)(b))\n"
       "#define XBITS(x) ((unsigned long long)__double_as_longlong(x))\n";
  s += kExprPrelude;
  s += expr_value_function(d);
  s += R"PINOTX(
typedef unsigned x_u4 __attribute__((ext_vector_type(4)));
typedef unsigned x_u2 __attribute__((ext_vector_type(2)));
XFN unsigned x_bs(unsigned x) { return __builtin_bswap32(x); }
XFN unsigned x_sel(unsigned i, unsigned a, unsigned b, unsigned c, unsigned e) { return i == 0 ? a : i == 1 ? b : i == 2 ? c : e; }
template <int B>
XFN void x_fixed4(const unsigned* __restrict__ w, long long doc0, int card, int id[4]) {
  const long long bit0 = doc0 * B;
  const long long w0 = bit0 >> 5;
  const unsigned r = (unsigned)(bit0 & 31);
  const unsigned x0 = x_bs(w[w0]), x1 = x_bs(w[w0 + 1]), x2 = x_bs(w[w0 + 2]), x3 = x_bs(w[w0 + 3]), x4 = x_bs(w[w0 + 4]);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const unsigned p = r + (unsigned)(k * B);
    const unsigned i = p >> 5, sh = p & 31;
    const unsigned long long win = ((unsigned long long)x_sel(i, x0, x1, x2, x3) << 32) | x_sel(i, x1, x2, x3, x4);
    const int v = (int)((win << sh) >> (64 - B));
    id[k] = v < card ? v : card - 1;
  }
}
XFN void x_sorted4(const int* __restrict__ starts, long long doc0, int card, int id[4]) {
  int lo = 0, hi = card - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if ((long long)starts[mid] <= doc0) lo = mid; else hi = mid - 1;
  }
  id[0] = lo;
#pragma unroll
  for (int k = 1; k < 4; ++k) {
    while (lo + 1 < card && (long long)starts[lo + 1] <= doc0 + k) ++lo;
    id[k] = lo;
  }
}
)PINOTX";
  s += "extern \"C\" __global__ void __launch_bounds__(256) pinot_expr_eval(";
  for (size_t i = 0; i < src.size(); ++i) {
    const std::string n = std::to_string(i);
    s += "const unsigned* __restrict__ f" + n + ", const void* __restrict__ d" + n + ", int card" + n + ", ";
  }
  s += "unsigned char* __restrict__ out, long long num_docs, long long tiles) {\n"
       "  for (long long t = blockIdx.x; t < tiles; t += gridDim.x) {\n"
       "    const long long doc0 = t * 1024 + (long long)threadIdx.x * 4;\n"
       "    if (doc0 >= num_docs) continue;\n";
  static const char* const ctype[] = {"int", "long long", "float", "double"};
  for (size_t i = 0; i < src.size(); ++i) {
    const std::string n = std::to_string(i), c = "c" + n;
    const ExprSrcShape& sh = src[i];
    s += "    double " + c + "[4];\n    {\n";
    if (sh.enc == 1) {  // raw: big-endian values, 4 per lane
      if (sh.type == 0 || sh.type == 2) {
        s += "      const x_u4 r = *static_cast<const x_u4*>(__builtin_assume_aligned(f" + n + " + doc0, 16));\n";
        const char* comp[] = {"r.x", "r.y", "r.z", "r.w"};
        for (int k = 0; k < 4; ++k)
          s += "      " + c + "[" + std::to_string(k) + "] = (double)" +
               (sh.type == 0 ? "(int)x_bs(" + std::string(comp[k]) + ")" : "__uint_as_float(x_bs(" + std::string(comp[k]) + "))") +
               ";\n";
      } else {
        s += "      const x_u4 r = *static_cast<const x_u4*>(__builtin_assume_aligned(f" + n + " + doc0 * 2, 16));\n"
             "      const x_u4 q = *static_cast<const x_u4*>(__builtin_assume_aligned(f" + n + " + doc0 * 2 + 4, 16));\n";
        const char* hi[] = {"r.x", "r.z", "q.x", "q.z"};
        const char* lo[] = {"r.y", "r.w", "q.y", "q.w"};
        for (int k = 0; k < 4; ++k) {
          const std::string u = "(((unsigned long long)x_bs(" + std::string(hi[k]) + ") << 32) | x_bs(" + lo[k] + "))";
          s += "      " + c + "[" + std::to_string(k) + "] = " +
               (sh.type == 1 ? "(double)(long long)" + u : "__longlong_as_double((long long)" + u + ")") + ";\n";
        }
      }
    } else {
      s += "      int id[4];\n";
      if (sh.enc == 0) s += "      x_fixed4<" + std::to_string(sh.bits) + ">(f" + n + ", doc0, card" + n + ", id);\n";
      else s += "      x_sorted4(reinterpret_cast<const int*>(f" + n + "), doc0, card" + n + ", id);\n";
      s += "      const " + std::string(ctype[sh.type]) + "* __restrict__ dv = static_cast<const " + ctype[sh.type] + "*>(d" + n +
           ");\n";
      for (int k = 0; k < 4; ++k)
        s += "      " + c + "[" + std::to_string(k) + "] = (double)dv[id[" + std::to_string(k) + "]];\n";
    }
    s += "    }\n";
  }
  s += "    unsigned hi[4], lo[4];\n";
  for (int k = 0; k < 4; ++k) {
    s += "    {\n      const unsigned long long b = XBITS(pinot_expr_value(";
    for (size_t i = 0; i < src.size(); ++i) s += (i ? ", c" : "c") + std::to_string(i) + "[" + std::to_string(k) + "]";
    s += "));\n      hi[" + std::to_string(k) + "] = x_bs((unsigned)(b >> 32));\n      lo[" + std::to_string(k) +
         "] = x_bs((unsigned)b);\n    }\n";
  }
  s += "    unsigned char* o = out + doc0 * 8;\n"
       "    if (doc0 + 4 <= num_docs) {\n"
       "      *static_cast<x_u4*>(__builtin_assume_aligned(o, 16)) = x_u4{hi[0], lo[0], hi[1], lo[1]};\n"
       "      *static_cast<x_u4*>(__builtin_assume_aligned(o + 16, 16)) = x_u4{hi[2], lo[2], hi[3], lo[3]};\n"
       "    } else {\n";
  for (int k = 0; k < 3; ++k)
    s += "      if (doc0 + " + std::to_string(k) + " < num_docs) *reinterpret_cast<x_u2*>(o + " + std::to_string(8 * k) +
         ") = x_u2{hi[" + std::to_string(k) + "], lo[" + std::to_string(k) + "]};\n";
  s += "    }\n  }\n}\n";
  return s;
}

inline std::string expr_kernel_key(const ExprDef& d, const std::vector<ExprSrcShape>& src) {
  std::string k = "expr|" + expr_shape(d);
  for (const ExprSrcShape& s : src) k += "|" + std::to_string(s.enc) + "." + std::to_string(s.type) + "." + std::to_string(s.bits);
  return k;
}

}  // namespace pamd
