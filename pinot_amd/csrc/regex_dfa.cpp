// regex_dfa.cpp — pattern -> AST -> Thompson NFA over UTF-8 bytes -> DFA over byte classes (regex_dfa.h).
#include "regex_dfa.h"

#include <string.h>

#include <algorithm>
#include <map>
#include <memory>
#include <utility>

namespace pamd_regex {
namespace {

struct Err {
  int code;
  std::string msg;
};
[[noreturn]] void refuse(const std::string& what) { throw Err{kUnsupported, "unsupported pattern: " + what}; }
[[noreturn]] void invalid(const std::string& what) { throw Err{kInvalid, "invalid pattern: " + what}; }
[[noreturn]] void too_complex(const char* what, int cap) {
  throw Err{kUnsupported, std::string("pattern too complex: more than ") + std::to_string(cap) + " " + what};
}

// ---- code-point sets ----
typedef std::pair<uint32_t, uint32_t> Range;  // inclusive
typedef std::vector<Range> Set;
constexpr uint32_t kMaxCp = 0x10FFFF;

void normalize(Set& s) {
  std::sort(s.begin(), s.end());
  Set out;
  for (const Range& r : s) {
    if (!out.empty() && r.first <= out.back().second + 1)
      out.back().second = std::max(out.back().second, r.second);
    else
      out.push_back(r);
  }
  s.swap(out);
}
Set negated(Set s) {
  normalize(s);
  Set out;
  uint32_t next = 0;
  for (const Range& r : s) {
    if (r.first > next) out.push_back({next, r.first - 1});
    next = r.second + 1;
  }
  if (next <= kMaxCp) out.push_back({next, kMaxCp});
  return out;
}
void unite(Set& a, const Set& b) { a.insert(a.end(), b.begin(), b.end()); }

bool ascii_letter(uint32_t c) { return (c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z'); }
bool in(uint32_t lo, uint32_t c, uint32_t hi) { return lo <= c && c <= hi; }

// Pattern.SingleU for an ASCII pattern char: c matches x iff toLowerCase(toUpperCase(c)) == toLowerCase(toUpperCase(x)).
// Beyond the two ASCII cases, exactly four code points fold into ASCII under Unicode's simple case mappings: U+0130 and
// U+0131 to 'i', U+017F to 's', U+212A to 'k'.
Set ci_single(uint32_t x) {
  Set s;
  if (!ascii_letter(x)) {
    s.push_back({x, x});
    return s;
  }
  const uint32_t lo = x | 0x20, up = x & ~0x20u;
  s.push_back({lo, lo});
  s.push_back({up, up});
  if (lo == 'i') s.push_back({0x130, 0x131});
  if (lo == 's') s.push_back({0x17F, 0x17F});
  if (lo == 'k') s.push_back({0x212A, 0x212A});
  return s;
}
// Pattern.CIRangeU for an ASCII range: c matches iff c, toUpperCase(c) or toLowerCase(toUpperCase(c)) is in [lo, hi]
Set ci_range(uint32_t lo, uint32_t hi) {
  Set s;
  s.push_back({lo, hi});
  for (uint32_t c = 'a'; c <= 'z'; ++c) {
    const uint32_t up = c - 0x20;
    if (in(lo, c, hi) || in(lo, up, hi)) {
      s.push_back({c, c});
      s.push_back({up, up});
    }
  }
  if (in(lo, 'I', hi) || in(lo, 'i', hi)) s.push_back({0x131, 0x131});  // upper 'I', then lower 'i'
  if (in(lo, 'i', hi)) s.push_back({0x130, 0x130});                      // its own upper case; lower 'i'
  if (in(lo, 'S', hi) || in(lo, 's', hi)) s.push_back({0x17F, 0x17F});
  if (in(lo, 'k', hi)) s.push_back({0x212A, 0x212A});
  return s;
}

Set set_digit() { return Set{{'0', '9'}}; }
Set set_word() { return Set{{'a', 'z'}, {'A', 'Z'}, {'0', '9'}, {'_', '_'}}; }
Set set_space() { return Set{{' ', ' '}, {'\t', '\r'}}; }  // [ \t\n\x0B\f\r]
Set set_dot() { return negated(Set{{'\n', '\n'}, {'\r', '\r'}, {0x85, 0x85}, {0x2028, 0x2029}}); }

// ---- AST ----
enum { N_EMPTY, N_SET, N_CAT, N_ALT, N_REP, N_BOL, N_EOL };
struct Node {
  int kind = N_EMPTY;
  Set set;
  std::vector<std::unique_ptr<Node>> kids;
  int min = 0, max = 0;  // N_REP; max < 0: unbounded
};
typedef std::unique_ptr<Node> NodeP;
NodeP mk(int kind) {
  NodeP n(new Node());
  n->kind = kind;
  return n;
}

std::string cp_text(uint32_t c) {
  std::string s;
  if (c < 0x80) {
    s += (char)c;
  } else if (c < 0x800) {
    s += (char)(0xC0 | (c >> 6));
    s += (char)(0x80 | (c & 0x3F));
  } else if (c < 0x10000) {
    s += (char)(0xE0 | (c >> 12));
    s += (char)(0x80 | ((c >> 6) & 0x3F));
    s += (char)(0x80 | (c & 0x3F));
  } else {
    s += (char)(0xF0 | (c >> 18));
    s += (char)(0x80 | ((c >> 12) & 0x3F));
    s += (char)(0x80 | ((c >> 6) & 0x3F));
    s += (char)(0x80 | (c & 0x3F));
  }
  return s;
}

std::vector<uint32_t> decode_utf8(const std::string& s) {
  std::vector<uint32_t> out;
  size_t i = 0;
  const size_t n = s.size();
  while (i < n) {
    const uint8_t b = (uint8_t)s[i];
    uint32_t c;
    int len;
    if (b < 0x80) { c = b; len = 1; }
    else if (b >= 0xC2 && b <= 0xDF) { c = b & 0x1F; len = 2; }
    else if (b >= 0xE0 && b <= 0xEF) { c = b & 0x0F; len = 3; }
    else if (b >= 0xF0 && b <= 0xF4) { c = b & 0x07; len = 4; }
    else invalid("the pattern is not UTF-8");
    if (i + len > n) invalid("the pattern is not UTF-8");
    for (int k = 1; k < len; ++k) {
      const uint8_t t = (uint8_t)s[i + k];
      if ((t & 0xC0) != 0x80) invalid("the pattern is not UTF-8");
      c = (c << 6) | (t & 0x3F);
    }
    if ((len == 3 && c < 0x800) || (len == 4 && (c < 0x10000 || c > kMaxCp)) || (c >= 0xD800 && c <= 0xDFFF))
      invalid("the pattern is not UTF-8");
    out.push_back(c);
    i += len;
  }
  return out;
}

struct Parser {
  std::vector<uint32_t> p;
  size_t i = 0;
  bool ci = false;

  bool more() const { return i < p.size(); }
  uint32_t peek() const { return p[i]; }
  bool at(uint32_t c, size_t k = 0) const { return i + k < p.size() && p[i + k] == c; }

  NodeP set_node(Set s) {
    NodeP n = mk(N_SET);
    normalize(s);
    n->set = std::move(s);
    return n;
  }
  void ci_ascii_only(uint32_t c) {
    if (ci && c > 0x7F)
      refuse("case-insensitive pattern with the non-ASCII character '" + cp_text(c) +
             "' (needs Unicode's simple case mappings)");
  }
  Set literal(uint32_t c) {
    ci_ascii_only(c);
    return ci ? ci_single(c) : Set{{c, c}};
  }

  int hex_digit() {
    if (!more()) invalid("illegal hexadecimal escape sequence");
    const uint32_t c = p[i++];
    if (c >= '0' && c <= '9') return (int)(c - '0');
    if (c >= 'a' && c <= 'f') return (int)(c - 'a' + 10);
    if (c >= 'A' && c <= 'F') return (int)(c - 'A' + 10);
    invalid("illegal hexadecimal escape sequence");
  }

  // after the backslash. Returns true and *cp for a literal; false and *set for a predefined class. Anchors and
  // everything refused are thrown.
  bool escape(uint32_t* cp, Set* set, bool in_class) {
    if (!more()) invalid("a trailing backslash");
    const uint32_t c = p[i++];
    const bool alpha = ascii_letter(c), digit = c >= '0' && c <= '9';
    if (!alpha && !digit) {
      *cp = c;
      return true;
    }
    if (c == '0') refuse("octal escape \\0");
    if (digit) refuse(std::string("back-reference \\") + (char)c);
    switch (c) {
      case 't': *cp = '\t'; return true;
      case 'n': *cp = '\n'; return true;
      case 'r': *cp = '\r'; return true;
      case 'f': *cp = '\f'; return true;
      case 'x': {
        if (at('{')) refuse("\\x{...} escape");
        const int h = hex_digit(), l = hex_digit();
        *cp = (uint32_t)(h * 16 + l);
        return true;
      }
      case 'u': {
        uint32_t v = 0;
        for (int k = 0; k < 4; ++k) v = v * 16 + (uint32_t)hex_digit();
        if (v >= 0xD800 && v <= 0xDFFF) refuse("surrogate escape \\u");
        *cp = v;
        return true;
      }
      case 'd': *set = set_digit(); return false;
      case 'D': *set = negated(set_digit()); return false;
      case 'w': *set = set_word(); return false;
      case 'W': *set = negated(set_word()); return false;
      case 's': *set = set_space(); return false;
      case 'S': *set = negated(set_space()); return false;
      case 'b': case 'B': case 'A': case 'z': case 'Z': case 'G':
        refuse(std::string("boundary matcher \\") + (char)c);
      case 'p': case 'P': refuse(std::string("\\") + (char)c + "{...} class");
      case 'Q': case 'E': refuse("\\Q...\\E quoting");
      case 'k': refuse("named back-reference \\k");
      default: refuse(std::string("escape \\") + (char)c);
    }
  }

  NodeP char_class() {  // after '['
    bool neg = false;
    if (at('^')) {
      neg = true;
      ++i;
    }
    Set s;
    bool first = true;
    for (;; first = false) {
      if (!more()) invalid("unclosed character class");
      uint32_t c = p[i++];
      if (c == ']' && !first) break;
      if (c == '[') refuse("nested or POSIX character class");
      if (c == '&' && at('&')) refuse("character class intersection &&");
      uint32_t lo = c;
      if (c == '\\') {
        Set pre;
        if (!escape(&lo, &pre, true)) {
          unite(s, pre);
          continue;
        }
      }
      if (at('-') && i + 1 < p.size() && p[i + 1] != ']') {
        ++i;
        uint32_t hi = p[i++];
        if (hi == '[') refuse("nested or POSIX character class");
        if (hi == '\\') {
          Set pre;
          if (!escape(&hi, &pre, true)) invalid("illegal character range");
        }
        if (hi < lo) invalid("illegal character range");
        ci_ascii_only(lo);
        ci_ascii_only(hi);
        unite(s, ci ? ci_range(lo, hi) : Set{{lo, hi}});
        continue;
      }
      unite(s, literal(lo));
    }
    return set_node(neg ? negated(s) : s);
  }

  NodeP atom() {
    const uint32_t c = p[i++];
    switch (c) {
      case '(': {
        if (at('?')) {
          if (at(':', 1)) {
            i += 2;
          } else if (at('=', 1) || at('!', 1)) {
            refuse("look-ahead (?= / (?!");
          } else if (at('<', 1) && (at('=', 2) || at('!', 2))) {
            refuse("look-behind (?<= / (?<!");
          } else if (at('<', 1)) {
            refuse("named group (?<name>");
          } else if (at('>', 1)) {
            refuse("atomic group (?>");
          } else {
            refuse("inline flags (?...)");
          }
        }
        NodeP n = alt();
        if (!at(')')) invalid("unclosed group");
        ++i;
        return n;
      }
      case '[': return char_class();
      case '.': return set_node(set_dot());
      case '^': return mk(N_BOL);
      case '$': return mk(N_EOL);
      case '*': case '+': case '?': invalid(std::string("dangling meta character '") + (char)c + "'");
      case '{': invalid("illegal repetition");
      case '\\': {
        uint32_t cp = 0;
        Set pre;
        if (escape(&cp, &pre, false)) return set_node(literal(cp));
        return set_node(pre);
      }
      default: return set_node(literal(c));
    }
  }

  NodeP rep() {
    NodeP a = atom();
    if (!more()) return a;
    int mn, mx;
    const uint32_t c = peek();
    if (c == '*') { mn = 0; mx = -1; ++i; }
    else if (c == '+') { mn = 1; mx = -1; ++i; }
    else if (c == '?') { mn = 0; mx = 1; ++i; }
    else if (c == '{') {
      ++i;
      auto number = [&]() -> int {
        if (!more() || peek() < '0' || peek() > '9') invalid("illegal repetition");
        long v = 0;
        while (more() && peek() >= '0' && peek() <= '9') {
          v = v * 10 + (long)(p[i++] - '0');
          if (v > kMaxRepeat) too_complex("repetitions in a counted quantifier", kMaxRepeat);
        }
        return (int)v;
      };
      mn = number();
      mx = mn;
      if (at(',')) {
        ++i;
        mx = at('}') ? -1 : number();
      }
      if (!at('}')) invalid("unclosed counted closure");
      ++i;
      if (mx >= 0 && mx < mn) invalid("illegal repetition range");
    } else {
      return a;
    }
    if (at('?')) ++i;  // lazy: the same language, and only existence is asked
    else if (at('+')) refuse("possessive quantifier");
    if (at('*') || at('+') || at('?')) invalid(std::string("dangling meta character '") + (char)peek() + "'");
    if (at('{')) refuse("a quantifier applied to a quantifier");
    if (a->kind == N_BOL || a->kind == N_EOL) refuse("a quantifier applied to an anchor");
    NodeP r = mk(N_REP);
    r->min = mn;
    r->max = mx;
    r->kids.push_back(std::move(a));
    return r;
  }

  NodeP cat() {
    NodeP n = mk(N_CAT);
    while (more() && peek() != '|' && peek() != ')') n->kids.push_back(rep());
    return n;
  }
  NodeP alt() {
    NodeP first = cat();
    if (!at('|')) return first;
    NodeP n = mk(N_ALT);
    n->kids.push_back(std::move(first));
    while (at('|')) {
      ++i;
      n->kids.push_back(cat());
    }
    return n;
  }
};

// can the node match without consuming input wherever it stands? ('^' counts as no: it holds at position 0 only)
bool nullable(const Node& n) {
  switch (n.kind) {
    case N_EMPTY: case N_EOL: return true;
    case N_SET: case N_BOL: return false;
    case N_CAT:
      for (auto& k : n.kids)
        if (!nullable(*k)) return false;
      return true;
    case N_ALT:
      for (auto& k : n.kids)
        if (nullable(*k)) return true;
      return false;
    default: return n.min == 0 || nullable(*n.kids[0]);
  }
}
// '$' is compiled as "the rest of the input is at most one line terminator" followed by acceptance, which is exact only
// when everything that can follow it in the pattern can match empty (then X$Y matches iff X$ does). Anything else is
// refused: tail_ok says whether what follows the node is such a tail.
void check_dollar(const Node& n, bool tail_ok) {
  switch (n.kind) {
    case N_EOL:
      if (!tail_ok) refuse("'$' followed by an element that must consume input or by '^'");
      return;
    case N_CAT: {
      bool ok = tail_ok;
      for (size_t k = n.kids.size(); k-- > 0;) {
        check_dollar(*n.kids[k], ok);
        ok = ok && nullable(*n.kids[k]);
      }
      return;
    }
    case N_ALT:
      for (auto& k : n.kids) check_dollar(*k, tail_ok);
      return;
    case N_REP:
      check_dollar(*n.kids[0], (n.max == 1 || n.max == 0) ? tail_ok : tail_ok && nullable(*n.kids[0]));
      return;
    default: return;
  }
}

// ---- NFA ----
struct Edge {
  uint8_t lo, hi;
  bool nocr;  // taken only when the previous byte was not '\r' (Dollar: no match between \r and \n)
  int to;
};
struct NState {
  std::vector<int> eps, bol_eps;  // bol_eps: taken at input position 0 only
  std::vector<Edge> edges;
  bool end_ok = false;  // the end-of-input symbol leads to acceptance
};

void utf8_encode(uint32_t c, uint8_t* b, int* n) {
  const std::string s = cp_text(c);
  *n = (int)s.size();
  memcpy(b, s.data(), s.size());
}

struct Nfa {
  std::vector<NState> st;
  int eol = -1;  // the shared '$' entry state

  int add() {
    if ((int)st.size() >= kMaxNfaStates) too_complex("NFA states", kMaxNfaStates);
    st.emplace_back();
    return (int)st.size() - 1;
  }
  void eps(int a, int b) { st[a].eps.push_back(b); }
  void edge(int a, uint8_t lo, uint8_t hi, int b, bool nocr = false) { st[a].edges.push_back({lo, hi, nocr, b}); }

  // code points [lo, hi], all of one encoded length and free of surrogates, as byte-range sequences from -> to
  void utf8_same_len(uint32_t lo, uint32_t hi, int from, int to) {
    uint8_t a[4], b[4];
    int n, m;
    utf8_encode(lo, a, &n);
    utf8_encode(hi, b, &m);
    for (int k = 1; k < n; ++k) {
      const uint32_t mask = (1u << (6 * k)) - 1;
      if ((lo & ~mask) != (hi & ~mask)) {
        if ((lo & mask) != 0) {
          utf8_same_len(lo, lo | mask, from, to);
          utf8_same_len((lo | mask) + 1, hi, from, to);
          return;
        }
        if ((hi & mask) != mask) {
          utf8_same_len(lo, (hi & ~mask) - 1, from, to);
          utf8_same_len(hi & ~mask, hi, from, to);
          return;
        }
      }
    }
    int cur = from;
    for (int k = 0; k < n; ++k) {
      const int nxt = k + 1 == n ? to : add();
      edge(cur, a[k], b[k], nxt);
      cur = nxt;
    }
  }
  void set_edges(const Set& s, int from, int to) {
    static const uint32_t cut[5][2] = {{0, 0x7F}, {0x80, 0x7FF}, {0x800, 0xD7FF}, {0xE000, 0xFFFF}, {0x10000, kMaxCp}};
    for (const Range& r : s)
      for (auto& c : cut) {
        const uint32_t lo = std::max(r.first, c[0]), hi = std::min(r.second, c[1]);
        if (lo <= hi) utf8_same_len(lo, hi, from, to);
      }
  }

  int eol_state() {
    if (eol >= 0) return eol;
    const int e = add(), end = add(), cr = add(), c2 = add(), e2 = add(), e280 = add();
    st[e].end_ok = st[end].end_ok = st[cr].end_ok = true;
    edge(e, '\n', '\n', end, true);
    edge(e, '\r', '\r', cr);
    edge(cr, '\n', '\n', end);
    edge(e, 0xC2, 0xC2, c2);  // U+0085
    edge(c2, 0x85, 0x85, end);
    edge(e, 0xE2, 0xE2, e2);  // U+2028, U+2029
    edge(e2, 0x80, 0x80, e280);
    edge(e280, 0xA8, 0xA9, end);
    return eol = e;
  }

  // the fragment of `n` starting at state `from`; returns its end state
  int build(const Node& n, int from) {
    switch (n.kind) {
      case N_EMPTY: return from;
      case N_SET: {
        const int to = add();
        set_edges(n.set, from, to);
        return to;
      }
      case N_CAT: {
        int cur = from;
        for (auto& k : n.kids) cur = build(*k, cur);
        return cur;
      }
      case N_ALT: {
        const int to = add();
        for (auto& k : n.kids) {
          const int s = add();
          eps(from, s);
          eps(build(*k, s), to);
        }
        return to;
      }
      case N_REP: {
        const Node& body = *n.kids[0];
        int cur = from;
        for (int k = 0; k < n.min; ++k) cur = build(body, cur);
        const int out = add();
        if (n.max < 0) {
          const int loop = add(), b = add();
          eps(cur, loop);
          eps(loop, b);
          eps(build(body, b), loop);
          eps(loop, out);
        } else {
          for (int k = n.min; k < n.max; ++k) {
            eps(cur, out);
            const int s = add();
            eps(cur, s);
            cur = build(body, s);
          }
          eps(cur, out);
        }
        return out;
      }
      case N_BOL: {
        const int to = add();
        st[from].bol_eps.push_back(to);
        return to;
      }
      default: {  // N_EOL: what follows can match empty (check_dollar), so the '$' states accept by themselves
        eps(from, eol_state());
        return add();
      }
    }
  }
};

struct Closure {
  const Nfa& nfa;
  std::vector<int> stamp, stack;
  int gen = 0;
  explicit Closure(const Nfa& n) : nfa(n), stamp(n.st.size(), 0) {}
  // `seed` -> its epsilon closure, sorted
  void run(std::vector<int>& set, bool bol) {
    ++gen;
    stack.clear();
    std::vector<int> out;
    for (int s : set)
      if (stamp[s] != gen) {
        stamp[s] = gen;
        stack.push_back(s);
      }
    while (!stack.empty()) {
      const int s = stack.back();
      stack.pop_back();
      out.push_back(s);
      auto visit = [&](int t) {
        if (stamp[t] != gen) {
          stamp[t] = gen;
          stack.push_back(t);
        }
      };
      for (int t : nfa.st[s].eps) visit(t);
      if (bol)
        for (int t : nfa.st[s].bol_eps) visit(t);
    }
    std::sort(out.begin(), out.end());
    set.swap(out);
  }
};

void build_dfa(const Nfa& nfa, int nfa_start, int nfa_accept, Dfa* out) {
  // byte classes from the edges' boundaries
  bool cut[257] = {false};
  cut[0] = true;
  for (const NState& s : nfa.st)
    for (const Edge& e : s.edges) cut[e.lo] = cut[(int)e.hi + 1] = true;
  std::vector<uint8_t> cls(256), rep;
  int nbc = -1;
  for (int b = 0; b < 256; ++b) {
    if (cut[b]) {
      ++nbc;
      rep.push_back((uint8_t)b);
    }
    cls[b] = (uint8_t)nbc;
  }
  ++nbc;
  const int ncls = nbc + 1, endc = nbc;

  // subset construction; states 0 = dead, 1 = accept; a state is (NFA set, previous byte was '\r' and the set holds
  // the '$' entry state)
  typedef std::pair<std::vector<int>, int> Key;
  std::map<Key, int> ids;
  std::vector<Key> keys(2);
  std::vector<std::vector<int>> trans(2, std::vector<int>(ncls));
  for (int c = 0; c < ncls; ++c) {
    trans[0][c] = 0;
    trans[1][c] = 1;
  }
  Closure closure(nfa);
  auto intern = [&](std::vector<int>& set, bool after_cr) -> int {
    if (set.empty()) return 0;
    if (std::binary_search(set.begin(), set.end(), nfa_accept)) return 1;
    const int cr = after_cr && nfa.eol >= 0 && std::binary_search(set.begin(), set.end(), nfa.eol) ? 1 : 0;
    Key k(set, cr);
    auto it = ids.find(k);
    if (it != ids.end()) return it->second;
    if ((int)keys.size() >= kMaxDfaStates) too_complex("DFA states", kMaxDfaStates);
    const int id = (int)keys.size();
    ids.emplace(k, id);
    keys.push_back(std::move(k));
    trans.emplace_back(ncls, 0);
    return id;
  };
  std::vector<int> seed{nfa_start};
  closure.run(seed, true);
  const int start = intern(seed, false);
  std::vector<int> next;
  for (int id = 2; id < (int)keys.size(); ++id) {
    const std::vector<int> set = keys[id].first;  // (a copy: intern() grows keys)
    const int cr = keys[id].second;
    bool end_ok = false;
    for (int s : set) end_ok |= nfa.st[s].end_ok;
    trans[id][endc] = end_ok ? 1 : 0;
    for (int c = 0; c < nbc; ++c) {
      const uint8_t b = rep[c];
      next.clear();
      for (int s : set)
        for (const Edge& e : nfa.st[s].edges)
          if (e.lo <= b && b <= e.hi && !(e.nocr && cr)) next.push_back(e.to);
      closure.run(next, false);
      const int to = intern(next, b == '\r');
      trans[id][c] = to;
    }
  }
  const int n = (int)keys.size();

  // states that cannot reach acceptance are the dead state (an anchored pattern's lanes leave at the first mismatch)
  std::vector<std::vector<int>> rev(n);
  for (int s = 0; s < n; ++s)
    for (int c = 0; c < ncls; ++c) rev[trans[s][c]].push_back(s);
  std::vector<char> live(n, 0);
  std::vector<int> stack{1};
  live[1] = 1;
  while (!stack.empty()) {
    const int s = stack.back();
    stack.pop_back();
    for (int t : rev[s])
      if (!live[t]) {
        live[t] = 1;
        stack.push_back(t);
      }
  }
  std::vector<int> renum(n, 0);
  int ns = 2;
  renum[1] = 1;
  for (int s = 2; s < n; ++s)
    if (live[s]) renum[s] = ns++;
  // byte classes with equal columns merge
  std::vector<int> col_of(nbc, -1);
  std::vector<int> kept;  // representative old class of each new class
  for (int c = 0; c < nbc; ++c) {
    for (size_t k = 0; k < kept.size() && col_of[c] < 0; ++k) {
      bool same = true;
      for (int s = 0; s < n && same; ++s)
        if (live[s] || s == 0) same = renum[trans[s][c]] == renum[trans[s][kept[k]]];
      if (same) col_of[c] = (int)k;
    }
    if (col_of[c] < 0) {
      col_of[c] = (int)kept.size();
      kept.push_back(c);
    }
  }
  const int nc = (int)kept.size() + 1;
  if ((long)ns * nc > kMaxTableEntries) too_complex("transition table entries (states x byte classes)", kMaxTableEntries);
  out->num_classes = nc;
  out->num_states = ns;
  for (int b = 0; b < 256; ++b) out->class_of[b] = (uint8_t)col_of[cls[b]];
  out->table.assign((size_t)ns * nc, 0);
  for (int s = 0; s < n; ++s) {
    if (s != 0 && !live[s]) continue;
    uint16_t* row = &out->table[(size_t)renum[s] * nc];
    for (size_t k = 0; k < kept.size(); ++k) row[k] = (uint16_t)(renum[trans[s][kept[k]]] * nc);
    row[nc - 1] = (uint16_t)(renum[trans[s][endc]] * nc);
  }
  out->start = (uint16_t)(renum[start] * nc);
}

}  // namespace

int compile(const std::string& pattern, bool case_insensitive, Dfa* out, std::string* err) {
  try {
    Parser ps;
    ps.p = decode_utf8(pattern);
    ps.ci = case_insensitive;
    NodeP root = ps.alt();
    if (ps.more()) invalid("unmatched closing ')'");
    check_dollar(*root, true);
    Nfa nfa;
    const int search = nfa.add();  // the unanchored search: any byte, then try the pattern again
    nfa.edge(search, 0, 255, search);
    const int first = nfa.add();
    nfa.eps(search, first);
    const int last = nfa.build(*root, first);
    const int accept = nfa.add();
    nfa.eps(last, accept);
    build_dfa(nfa, search, accept, out);
    return kOk;
  } catch (const Err& e) {
    if (err) *err = e.msg;
    return e.code;
  }
}

bool match(const Dfa& d, const char* s, size_t n) {
  const uint16_t* t = d.table.data();
  const uint32_t acc = d.accept();
  uint32_t row = d.start;
  for (size_t i = 0; i < n && row > acc; ++i) row = t[row + d.class_of[(uint8_t)s[i]]];
  if (row > acc) row = t[row + (uint32_t)d.end_class()];
  return row == acc;
}

std::string like_to_regexp(const std::string& like) {
  size_t start = 0, end = like.size();
  std::string prefix = "^", suffix = "$";
  if (like.empty()) return "^$";
  if (like.size() == 1) {
    if (like[0] == '%') return "";
  } else {
    if (like[0] == '%') {
      start = like.find_first_not_of('%');
      if (start == std::string::npos) return "";
      prefix = "";
    }
    if (like.back() == '%') {
      const size_t last = like.find_last_not_of('%');
      if (last == std::string::npos) return "";
      end = last + 1;
      suffix = "";
    }
  }
  static const char kMeta[] = "^$.{}[]()*+?|<>-&/";
  std::string out = prefix;
  bool prev_backslash = false;
  for (size_t i = start; i < end; ++i) {
    const char c = like[i];
    if (c == '_') {
      out += prev_backslash ? "_" : ".";
    } else if (c == '%') {
      out += prev_backslash ? "%" : ".*";
    } else {
      if ((c != '\0' && strchr(kMeta, c)) || prev_backslash) out += '\\';
      out += c;
    }
    prev_backslash = c == '\\';
  }
  if (prev_backslash) out += '\\';
  return out + suffix;
}

}  // namespace pamd_regex
