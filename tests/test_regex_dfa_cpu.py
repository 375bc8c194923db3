"""The pattern compiler and its host runner (pinot_amd/csrc/regex_dfa.cpp) against tests/regex_ref.py.

regex_dfa.cpp and the stand-alone driver tests/regex_dfa_main.cpp are built with the host compiler under
-fsanitize=address,undefined and run as a program of their own: patterns and subjects on stdin, verdicts on stdout.
Every pattern is answered exactly as the reference engine would answer it, or refused by name; never wrong."""
import json
import os
import random
import shutil
import subprocess

import pytest

import regex_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OK, INVALID, UNSUPPORTED = 0, 1, 2
MAX_STATES = 4096  # regex_dfa.h kMaxDfaStates


def _hex(s: str) -> str:
    b = s.encode("utf-8")
    return b.hex() if b else "-"


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("regex_dfa") / "regex_dfa_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "pinot_amd", "csrc", "regex_dfa.cpp"), os.path.join(HERE, "regex_dfa_main.cpp"),
                    "-o", exe], check=True)

    def run(cases):
        """cases: [(pattern, ci, [subjects])] -> [(code, message | (states, classes), [bool | None])]"""
        lines = []
        for pat, ci, subjects in cases:
            lines.append(f"P {1 if ci else 0} {_hex(pat)}")
            lines.extend("S " + _hex(s) for s in subjects)
        p = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert p.returncode == 0, p.stderr[-4000:]
        assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]
        out, rows = [], iter(p.stdout.splitlines())
        for pat, ci, subjects in cases:
            head = next(rows).split(" ", 2)
            if head[0] == "OK":
                code, info = OK, (int(head[1]), int(head[2]))
            else:
                code, info = int(head[1]), head[2]
            verdicts = [{"1": True, "0": False, "X": None}[next(rows)] for _ in subjects]
            out.append((code, info, verdicts))
        return out

    def like(patterns):
        p = subprocess.run([exe], input="".join(f"L {_hex(x)}\n" for x in patterns), capture_output=True, text=True)
        assert p.returncode == 0, p.stderr[-4000:]
        return [bytes.fromhex(h).decode() if h != "-" else "" for h in p.stdout.splitlines()]
    run.like = like
    return run


def check_exact(driver, cases):
    """Every case compiles and every verdict equals the reference's."""
    got = driver(cases)
    bad = []
    for (pat, ci, subjects), (code, info, verdicts) in zip(cases, got):
        if code != OK:
            bad.append((pat, ci, "refused: " + str(info)))
            continue
        for s, v in zip(subjects, verdicts):
            exp = R.matches(pat, s, ci)
            if v != exp:
                bad.append((pat, ci, s, "got", v, "expected", exp))
    assert not bad, bad[:20]


TEXTS = ["", "a", "abc", "ABC", "xabcx", "ab", "abcabc", "a.c", "a\nb", "a\rb", "abc\n", "abc\r\n", "abc\r", "abc\u2028",
         "abc\u2029", "abc\u0085", "abc\n\n", "\n", "\r\n", "é", "aé", "éa", "€", "a€b", "\U0001F600", "a\U0001F600b",
         "a b", "a_b", "a-b", "9", "a9", "  ", "\t", "a+b", "a\\b", "(a)", "[a]", "aaa", "aaaa", "aaaaa", "bbb", "abab",
         "İ", "ı", "ſ", "K", "I", "i", "S", "s", "K", "k", "xİx", "xıx", "xſx", "xKx", "Z", "z", "_", "~", "{"]

SUBSET = [
    "abc", "a.c", "a\\.c", "\\+", "\\\\", "a\\tb", "\\n", "\\r$", "\\f", "\\x41", "\\x61bc", "\\u00e9", "\\u20ac", "é", "€",
    "\U0001F600", ".", "..", "...", "a.b", "^.$", "^..$", "^...$", "^....$", ".*", "a.*b", "a.+b", "a.?b",
    "[abc]", "[^abc]", "[a-c]", "[^a-c]", "[a-cx-z]", "[\\d]", "[\\D]", "[^\\d]", "[\\w-]", "[a\\-z]", "[]a]", "[^]a]", "[a-]",
    "[-a]", "[\\n\\r]", "[^\\n]", "[é]", "[^é]", "[à-ÿ]", "[^à-ÿ]", "[€-₿]", "[\\u00e0-\\u00ff]", "[\\x41-\\x43]", "[.]",
    "[$]", "[a^]", "[&]", "[a&b]", "[^\\s\\d]", "[^\\W]", "[\\S\\s]",
    "\\d", "\\D", "\\w", "\\W", "\\s", "\\S", "\\d+", "\\w+$", "^\\s*$", "\\D\\d",
    "(abc)", "(?:abc)", "(a|b)c", "a|b", "a|", "|a", "()", "(a|)", "(a(b(c)))", "(?:a|b)*c", "a||b",
    "a*", "a+", "a?", "a{2}", "a{2,}", "a{2,3}", "a{0}", "a{0,1}", "(ab){2}", "(ab){1,2}c", "(a|b){3}", "[ab]{2,}c",
    "a*?", "a+?", "a??", "a{2}?", "a{2,}?", "a{2,3}?", "a.*?c", "(ab)+?c",
    "^abc", "abc$", "^abc$", "^$", "^", "$", "a^b", "(^a|b)", "a*^b", "(^|x)a", "^^a", "$$", "^$$", "a$|b", "(a$|b$)", "(a|b)$",
    "(abc$)?", "abc$()", "\\.$", "a?$", "[^a]$", "\\s$", "^\\n$", "\\n$", "\\r\\n$", ".$", "^.*$", "\\r?$", "\\r*$",
    "}", "]", "a}", "a]", " ", "#", "a b", "~", "<a>", "a-b", "a&b", "a/b", "\\<a\\>", "\\-", "\\&", "\\/", "\\_", "\\%",
]

REFUSED = {
    "\\1": UNSUPPORTED, "(a)\\1": UNSUPPORTED, "\\k<n>": UNSUPPORTED, "\\0": UNSUPPORTED, "(?=a)": UNSUPPORTED,
    "(?!a)": UNSUPPORTED, "(?<=a)b": UNSUPPORTED, "(?<!a)b": UNSUPPORTED, "\\bfoo": UNSUPPORTED, "foo\\B": UNSUPPORTED,
    "\\Aa": UNSUPPORTED, "a\\z": UNSUPPORTED, "a\\Z": UNSUPPORTED, "\\Ga": UNSUPPORTED, "a*+": UNSUPPORTED,
    "a++": UNSUPPORTED, "a?+": UNSUPPORTED, "a{2}+": UNSUPPORTED, "(?>a)": UNSUPPORTED, "(?i)a": UNSUPPORTED,
    "(?i:a)": UNSUPPORTED, "(?s).": UNSUPPORTED, "\\p{L}": UNSUPPORTED, "\\P{L}": UNSUPPORTED, "\\p{Alpha}": UNSUPPORTED,
    "[[:alpha:]]": UNSUPPORTED, "[a&&b]": UNSUPPORTED, "[a[b]]": UNSUPPORTED, "[a-c&&[b]]": UNSUPPORTED,
    "\\Qa.b\\E": UNSUPPORTED, "\\e": UNSUPPORTED, "\\a": UNSUPPORTED, "\\cA": UNSUPPORTED, "\\h": UNSUPPORTED,
    "\\v": UNSUPPORTED, "\\R": UNSUPPORTED, "\\X": UNSUPPORTED, "\\x{41}": UNSUPPORTED, "[\\b]": UNSUPPORTED,
    "(?<n>a)": UNSUPPORTED, "a$b": UNSUPPORTED, "$a": UNSUPPORTED, "(a$)+b": UNSUPPORTED, "^*": UNSUPPORTED,
    "$+": UNSUPPORTED, "\\ud83d": UNSUPPORTED,
    "*a": INVALID, "+": INVALID, "?": INVALID, "a**": INVALID, "(a": INVALID, "a)": INVALID, "[a": INVALID, "[": INVALID,
    "[]": INVALID, "[^]": INVALID, "a{": INVALID, "a{x}": INVALID, "a{3,2}": INVALID, "{": INVALID, "[z-a]": INVALID,
    "a\\": INVALID, "\\xg1": INVALID, "\\u12": INVALID, "[a-\\d]": INVALID,
}
REFUSED_NAMES = {"\\1": "back-reference", "(?=a)": "look-ahead", "(?<=a)b": "look-behind", "\\bfoo": "\\b",
                 "a*+": "possessive", "(?>a)": "atomic", "(?i)a": "inline flags", "\\p{L}": "\\p", "[a&&b]": "&&",
                 "[a[b]]": "nested", "\\Qa.b\\E": "\\Q", "\\e": "\\e", "a$b": "'$'"}


def test_subset_is_exact(driver):
    check_exact(driver, [(p, False, TEXTS) for p in SUBSET])


def test_subset_case_insensitive_is_exact(driver):
    ascii_only = [p for p in SUBSET if p.isascii() and "\\u00e" not in p and "\\u20ac" not in p]
    check_exact(driver, [(p, True, TEXTS) for p in ascii_only])


def test_refused_constructs_are_refused_by_name(driver):
    pats = list(REFUSED)
    got = driver([(p, False, []) for p in pats])
    wrong = [(p, code, info) for p, (code, info, _) in zip(pats, got) if code != REFUSED[p]]
    assert not wrong, wrong
    for p, (code, info, _) in zip(pats, got):
        if p in REFUSED_NAMES:
            assert REFUSED_NAMES[p] in info, (p, info)


def test_like_golden_pairs(driver):
    pairs = json.load(open(os.path.join(HERE, "golden", "like_patterns.json")))["pairs"]
    extra = ["", "%", "%%", "_", "a", "a%b", "a\\", "\\%", "%\\%", "a\\%", "50%", "a.b", "a|b", "(x)", "[x]", "x{2}", "a^$b",
             "<>-&/", "%é%", "_é_", "a%%b", "\\\\", "\\a"]
    got = driver.like([a for a, _ in pairs] + extra)
    assert got[:len(pairs)] == [b for _, b in pairs]
    assert got[len(pairs):] == [R.like_to_regexp(x) for x in extra]
    from pinot_amd.query import like_to_regexp
    assert [like_to_regexp(a) for a, _ in pairs] == [b for _, b in pairs]
    assert [like_to_regexp(x) for x in extra] == [R.like_to_regexp(x) for x in extra]
    # a LIKE is its converted pattern with 'i'; everything but the non-ASCII ones compiles
    likes = [a for a, _ in pairs] + [x for x in extra if x.isascii()]
    check_exact(driver, [(R.like_to_regexp(x), True, TEXTS + ["C+x", "c+", "xx++", "a_b\\", "a%b\\cde", "2_2", "zz"])
                         for x in likes])
    code, info, _ = driver([(R.like_to_regexp("%é%"), True, [])])[0]
    assert code == UNSUPPORTED and "non-ASCII" in info
    check_exact(driver, [("é", False, TEXTS)])


def test_dollar(driver):
    subjects = ["abc", "abc\n", "abc\r\n", "abc\r", "abc\u2028", "abc\n\n", "abc\u2029", "abc\u0085", "abc\n\r", "abc\r\r\n",
                "abc\r\n\n", "ab", "abcd", "", "\n", "\r\n", "\r", "abc\u2028x", "abc\r\nabc"]
    pats = ["abc$", "^abc$", "c$", "$", "^$", "\\r$", "c\\r$", "c\\r?$", "[^a]$", "\\s$", ".$", "abc\\n$", "(abc|x)$", "c$|d",
            R.like_to_regexp("abc"), R.like_to_regexp("%c"), R.like_to_regexp("abc_")]
    check_exact(driver, [(p, False, subjects) for p in pats])
    # LIKE 'abc' matches "abc\n" (Dollar without MULTILINE), and a '\r' consumed just before '$' does not let it match
    # between the '\r' and the '\n'
    (_, _, v), (_, _, w) = driver([("^abc$", True, ["abc\n", "abc\n\n", "ABC\r\n"]), ("\\r$", False, ["\r\n", "\r", "\r\r\n"])])
    assert v == [True, False, True] and w == [False, True, True]


def test_caret_mid_string(driver):
    check_exact(driver, [(p, False, ["ab", "b", "a\nb", "\nb", "xb", "bb", ""]) for p in ["a^b", "^b", "(^|a)b", "a*^b", "\\n^b"]])


def test_dot_and_underscore_over_code_points(driver):
    cps = ["a", "é", "€", "\U0001F600", "\n", "\r", "\u0085", "\u2028", "\u2029", "\x7f", "\u0080", "߿", "ࠀ", "￿",
           "\U00010000", "\U0010ffff", "퟿", ""]
    subjects = cps + [a + b for a in cps[:6] for b in cps[:6]] + ["a\nb", "a" + "\n" * 2 + "b", "aéb", "a€b"]
    pats = ["^.$", "^..$", ".", "a.b", "^a.*b$", R.like_to_regexp("_"), R.like_to_regexp("__"), R.like_to_regexp("a_b"),
            R.like_to_regexp("a%b")]
    check_exact(driver, [(p, False, subjects) for p in pats])
    (_, _, v), = driver([(R.like_to_regexp("a%b"), True, ["a\nb", "axb", "ab"])])
    assert v == [False, True, True]


def test_negated_classes_over_multibyte_input(driver):
    subjects = ["é", "€", "\U0001F600", "a", "aé", "éa", "ë", "ê", "è", "Ā", "\n", "é\n", ""]
    pats = ["[^a]", "^[^a]$", "[^é]", "^[^é]$", "^[^é]+$", "[^\\x00-\\x7f]", "^[^\\u0080-\\uffff]$", "\\W", "^\\W$", "^\\D\\S$",
            "[^\\w]", "^[^a-zé€]$"]
    check_exact(driver, [(p, False, subjects) for p in pats])


def test_case_fold_partners(driver):
    subjects = ["i", "I", "İ", "ı", "s", "S", "ſ", "k", "K", "K", "a", "z", "é", "_", "1", ""]
    pats = ["i", "I", "s", "S", "k", "K", "[a-z]", "[A-Z]", "[^k]", "[^K]", "[k]", "[I]", "[i]", "[i-i]", "[I-I]", "[h-j]",
            "[H-J]", "\\w", "\\W", "^[^s]$", "^[^a-z]$", "[j-l]", "[R-T]", "^\\w$", "is", "^k?$"]
    check_exact(driver, [(p, True, subjects) for p in pats])
    check_exact(driver, [(p, False, subjects) for p in pats])
    (_, _, v), (_, _, w) = driver([("k", True, ["K", "K", "k", "j"]), ("\\w", True, ["ſ", "s"])])
    assert v == [True, True, True, False] and w == [False, True]
    for p in ["é", "[é]", "[a-é]", "\\u00e9", "\\xe9"]:
        code, info, _ = driver([(p, True, [])])[0]
        assert code == UNSUPPORTED and "non-ASCII" in info, (p, code, info)


def test_empty_pattern_and_subject(driver):
    check_exact(driver, [(p, ci, ["", "a", "\n", "\r\n"]) for p in ["", "^$", "()", "a*", "^", "$"] for ci in (False, True)])
    assert driver.like([""]) == ["^$"]
    (_, _, v), = driver([("^$", True, ["", "\n", "a", "\n\n"])])  # LIKE ''
    assert v == [True, True, False, False]


def test_state_cap(driver):
    (code, (s10, _), _), = driver([("a{10}", False, [])])
    assert code == OK
    n = MAX_STATES - (s10 - 10)  # states grow by one per repetition
    at, past = driver([("a{%d}" % n, False, ["a" * n, "a" * (n - 1), "b" + "a" * n]), ("a{%d}" % (n + 1), False, [])])
    assert at[0] == OK and at[1][0] == MAX_STATES and at[2] == [True, False, True]
    assert past[0] == UNSUPPORTED and "pattern too complex" in past[1] and str(MAX_STATES) in past[1]
    code, info, _ = driver([("(a|b|c|d|e|f|g|h){30}x[a-m]{40}", False, [])])[0]
    assert code == UNSUPPORTED and "pattern too complex" in info
    code, info, _ = driver([("((a{200}){200}){200}", False, [])])[0]
    assert code == UNSUPPORTED and "pattern too complex" in info


def _random_pattern(rng, depth=0):
    atoms = ["a", "b", "é", "\\n", ".", "[ab]", "[^a]", "[^é]", "[aé]", "\\w", "\\W", "\\s", "[a-b]"]

    def atom():
        r = rng.random()
        if r < 0.15 and depth < 2:
            return "(" + _random_pattern(rng, depth + 1) + ")"
        if r < 0.2 and depth < 2:
            return "(?:" + _random_pattern(rng, depth + 1) + ")"
        return rng.choice(atoms)

    def piece():
        a = atom()
        r = rng.random()
        if r < 0.35:
            a += rng.choice(["*", "+", "?", "{2}", "{1,2}", "{2,}", "{0,2}"])
            if rng.random() < 0.2:
                a += "?"
        return a

    def branch():
        s = "".join(piece() for _ in range(rng.randint(0, 4)))
        if rng.random() < 0.2:
            s = "^" + s
        # ('$' inside a group mostly ends up in front of a consuming element, which is refused: keep those rare)
        if rng.random() < (0.25 if depth == 0 else 0.03):
            s += "$"
        return s
    return "|".join(branch() for _ in range(1 if rng.random() < 0.7 else rng.randint(2, 3)))


def test_random_patterns(driver):
    rng = random.Random(20240614)
    alphabet = ["a", "b", "é", "\n"]
    cases = []
    for k in range(3000):
        pat = _random_pattern(rng)
        subjects = ["".join(rng.choice(alphabet) for _ in range(rng.randint(0, 12))) for _ in range(8)]
        if k % 3 == 0:
            subjects += ["", "a\n", "b\r\n", "é\n\n"]
        cases.append((pat, False, subjects))
    got = driver(cases)
    wrong, refused = [], 0
    for (pat, ci, subjects), (code, info, verdicts) in zip(cases, got):
        if code != OK:
            assert code == UNSUPPORTED, (pat, code, info)  # the grammar writes valid patterns only
            refused += 1
            continue
        rx = R.compile_ref(pat, ci)
        for s, v in zip(subjects, verdicts):
            if v != (rx.search(s) is not None):
                wrong.append((pat, s, v))
    assert not wrong, wrong[:20]
    assert refused < len(cases) // 10, refused  # ('$' before a consuming element is the one refusal the grammar can hit)
