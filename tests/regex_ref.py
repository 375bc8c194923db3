"""LIKE / REGEXP_LIKE restated on Python's `re`, sharing nothing with the library's pattern compiler.

The engine restated is java.util.regex as Pinot drives it (JavaUtilPattern): flags 0 or CASE_INSENSITIVE |
UNICODE_CASE, Matcher.find(). A pattern of the supported subset is translated token by token into a Python pattern that
is compiled with re.ASCII and WITHOUT re.IGNORECASE:

* `.` becomes the explicit class of everything but the five line terminators (no DOTALL);
* `$` becomes a look-ahead restating Pattern.Dollar without MULTILINE: the end of input, or one final line terminator
  (`\\n` only when no `\\r` precedes it, `\\r`, `\\r\\n`, U+0085, U+2028, U+2029);
* `^` becomes `\\A`;
* in case-insensitive mode every literal and every class range is expanded by brute force over Java's rules
  (Pattern.SingleU: lower(upper(c)) == lower(upper(x)); Pattern.CIRangeU: c, upper(c) or lower(upper(c)) in the range)
  with Character.toUpperCase / toLowerCase restated for ASCII and the four code points that fold into it, so `\\w`
  keeps not matching U+017F.

Whole queries: a template marks pattern leaves with braces, ``WHERE {url LIKE '%x%'} AND n > 3``; `rewrite` drops the
braces for the library and turns leaf k into ``f_k = 1`` over an INT column this module evaluates per doc, for the
unchanged CPU oracle."""
import re

import numpy as np

from pinot_amd import segment as S

META = "^$.{}[]()*+?|<>-&/"


def like_to_regexp(like: str) -> str:
    """RegexpPatternConverterUtils.likeToRegexpLike."""
    if like == "":
        return "^$"
    if like == "%":
        return ""
    body, prefix, suffix = like, "^", "$"
    if len(like) > 1:
        if like.startswith("%"):
            body = body.lstrip("%")
            if body == "":
                return ""
            prefix = ""
        if like.endswith("%"):
            body = body.rstrip("%")
            suffix = ""
    out = ""
    esc = False
    for ch in body:
        if ch in "_%":
            out += ch if esc else {"_": ".", "%": ".*"}[ch]
        else:
            out += ("\\" if (ch in META or esc) else "") + ch
        esc = ch == "\\"
    return prefix + out + ("\\" if esc else "") + suffix


class Refused(ValueError):
    """A construct outside the supported subset."""


# Character.toUpperCase / toLowerCase over ASCII and the four code points whose simple case mappings reach ASCII
_UP = {0x131: ord("I"), 0x17F: ord("S")}
_LOW = {0x130: ord("i"), 0x212A: ord("k")}
_CANDIDATES = list(range(128)) + [0x130, 0x131, 0x17F, 0x212A]


def _upper(c):
    return _UP.get(c, c - 32 if 97 <= c <= 122 else c)


def _lower(c):
    return _LOW.get(c, c + 32 if 65 <= c <= 90 else c)


def _fold(c):
    return _lower(_upper(c))


def _ci_single(x):
    return [c for c in _CANDIDATES if _fold(c) == _fold(x)]


def _ci_range(lo, hi):
    return [c for c in _CANDIDATES if lo <= c <= hi or lo <= _upper(c) <= hi or lo <= _lower(_upper(c)) <= hi]


def _cls(cps):
    return "".join("\\U%08x" % c for c in cps)


_DOT = "[^\\n\\r\\x85\\u2028\\u2029]"
_DOLLAR = "(?=(?:\\r\\n|[\\r\\x85\\u2028\\u2029]|(?<!\\r)\\n)?\\Z)"
_PREDEF = "dDwWsS"


def _escape(p, i, ci):
    """The escape whose backslash is at p[i - 1]: (kind, payload, next index); kind 'lit' (a code point) or 'pre'."""
    if i >= len(p):
        raise Refused("trailing backslash")
    ch = p[i]
    if not (ch.isascii() and ch.isalnum()):
        return "lit", ord(ch), i + 1
    if ch in _PREDEF:
        return "pre", "\\" + ch, i + 1
    if ch in "tnrf":
        return "lit", ord({"t": "\t", "n": "\n", "r": "\r", "f": "\f"}[ch]), i + 1
    if ch == "x" and re.fullmatch("[0-9a-fA-F]{2}", p[i + 1:i + 3]):
        return "lit", int(p[i + 1:i + 3], 16), i + 3
    if ch == "u" and re.fullmatch("[0-9a-fA-F]{4}", p[i + 1:i + 5]):
        return "lit", int(p[i + 1:i + 5], 16), i + 5
    raise Refused("escape \\" + ch)


def translate(p: str, ci: bool) -> str:
    out, i = [], 0

    def lit(cp):
        if ci and cp > 127:
            raise Refused("non-ASCII character in a case-insensitive pattern")
        if ci:
            return "[" + _cls(_ci_single(cp)) + "]"
        return "\\U%08x" % cp

    while i < len(p):
        ch = p[i]
        i += 1
        if ch == ".":
            out.append(_DOT)
        elif ch == "$":
            out.append(_DOLLAR)
        elif ch == "^":
            out.append("\\A")
        elif ch == "\\":
            kind, v, i = _escape(p, i, ci)
            out.append(v if kind == "pre" else lit(v))
        elif ch == "(":
            if p[i:i + 1] == "?":
                if p[i:i + 2] != "?:":
                    raise Refused("group construct (?" + p[i + 1:i + 2])
                i += 2
            out.append("(?:")
        elif ch in ")|*+?":
            if ch == "+" and out and out[-1] in ("*", "+", "?", "}"):
                raise Refused("possessive quantifier")
            out.append(ch)
        elif ch == "{":
            m = re.match(r"(\d+)(,(\d*))?\}", p[i:])
            if not m:
                raise Refused("illegal repetition")
            out.append("{" + m.group(0)[:-1])
            out.append("}")
            i += m.end()
        elif ch == "[":
            neg = p[i:i + 1] == "^"
            i += 1 if neg else 0
            items, first = [], True
            while True:
                if i >= len(p):
                    raise Refused("unclosed class")
                c = p[i]
                i += 1
                if c == "]" and not first:
                    break
                first = False
                if c == "[" or (c == "&" and p[i:i + 1] == "&"):
                    raise Refused("nested class / intersection")
                lo = ord(c)
                if c == "\\":
                    kind, v, i = _escape(p, i, ci)
                    if kind == "pre":
                        items.append(v)
                        continue
                    lo = v
                if p[i:i + 1] == "-" and i + 1 < len(p) and p[i + 1] != "]":
                    h = p[i + 1]
                    i += 2
                    hi = ord(h)
                    if h == "[":
                        raise Refused("nested class")
                    if h == "\\":
                        kind, hi, i = _escape(p, i, ci)
                        if kind == "pre":
                            raise Refused("illegal range")
                    if hi < lo:
                        raise Refused("illegal range")
                    if ci and hi > 127:
                        raise Refused("non-ASCII character in a case-insensitive pattern")
                    items.append(_cls(_ci_range(lo, hi)) if ci else "\\U%08x-\\U%08x" % (lo, hi))
                else:
                    if ci and lo > 127:
                        raise Refused("non-ASCII character in a case-insensitive pattern")
                    items.append(_cls(_ci_single(lo)) if ci else "\\U%08x" % lo)
            out.append("[" + ("^" if neg else "") + "".join(items) + "]")
        else:
            out.append(lit(ord(ch)))
    return "".join(out)


def compile_ref(pattern: str, ci: bool = False):
    return re.compile(translate(pattern, ci), re.ASCII)


def matches(pattern: str, subject: str, ci: bool = False) -> bool:
    """Matcher.find() of the pattern over the subject."""
    return compile_ref(pattern, ci).search(subject) is not None


# ----------------------------------------------------------------------------------------- whole queries
_LEAF = re.compile(r"\{([^{}]*)\}")
_LIKE = re.compile(r"^\s*(\w+)\s+(NOT\s+)?LIKE\s+'((?:[^']|'')*)'\s*$", re.I)
_RLIKE = re.compile(r"^\s*(NOT\s+)?REGEXP_LIKE\(\s*(\w+)\s*,\s*'((?:[^']|'')*)'\s*(?:,\s*'(\w?)'\s*)?\)\s*$", re.I)


def leaf_of(text: str):
    """(column, compiled reference pattern, negate) of one braced leaf."""
    m = _LIKE.match(text)
    if m:
        return m.group(1), compile_ref(like_to_regexp(m.group(3).replace("''", "'")), True), bool(m.group(2))
    m = _RLIKE.match(text)
    if not m:
        raise ValueError(f"not a pattern leaf: {text!r}")
    return m.group(2), compile_ref(m.group(3).replace("''", "'"), (m.group(4) or "").lower() == "i"), bool(m.group(1))


def rewrite(template: str):
    """(the library's query, the oracle's query, the leaves)."""
    leaves = [leaf_of(m.group(1)) for m in _LEAF.finditer(template)]
    k = iter(range(len(leaves)))
    return _LEAF.sub(lambda m: m.group(1), template), _LEAF.sub(lambda m: f"f_{next(k)} = 1", template), leaves


def leaf_bits(values, leaf) -> np.ndarray:
    """Per doc 0 / 1: `values` holds a str per doc, or a list of str per doc of a multi-value column (ANY match; under
    NOT the negation of that)."""
    _, rx, neg = leaf
    memo = {}

    def hit(v):
        r = memo.get(v)
        if r is None:
            r = memo[v] = rx.search(v) is not None
        return r
    out = np.zeros(len(values), dtype=np.int32)
    for d, v in enumerate(values):
        h = any(hit(x) for x in v) if isinstance(v, (list, tuple)) else hit(v)
        out[d] = 1 if h != neg else 0
    return out


def oracle_segment(name, sv_columns, string_values, leaves):
    """A SegmentBuffers for the oracle: sv_columns {name: (values, type, kwargs)} as they are, plus f_k per leaf
    evaluated over string_values {column: per-doc str or list of str}."""
    cols = dict(sv_columns)
    for k, leaf in enumerate(leaves):
        cols[f"f_{k}"] = (leaf_bits(string_values[leaf[0]], leaf), S.INT, {"detect_sorted": False})
    return S.build_segment(name, cols)
