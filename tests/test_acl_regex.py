"""CPU tier of the ACL's geosite regex entries (include/hyobfs_acl.h, "THE REGEX
SUBSET"; hysteria_amd/csrc/acl_regex.h): the library's compiler and DFA walk
(hyobfs_acl_regex_check / _match, the function the kernel runs) against Python's
re on every regex of the reference's geosite database (tests/golden/
geosite_regex.json) and on an exhaustive small-case set, the traps and refusals
one by one, the kernel itself through a stand-alone AddressSanitizer build
(tests/emu/acl_regex_main.cpp + acl.hip against hip_emu.h, a child process), and
the Python surface's opt-in."""
import fcntl
import itertools
import os
import subprocess

import pytest

import acl_cases as ac
import acl_ref
import acl_regex_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
CLANG = "/opt/rocm/llvm/bin/clang++"


@pytest.fixture(scope="module")
def fx():
    return rc.fixture()


@pytest.fixture(scope="module")
def around(fx):
    """Per distinct fixture pattern: (pattern bytes, generated names), made once."""
    return [(v.encode(), rc.names_around(s.encode())) for v, s in sorted(fx["samples"].items())]


# ------------------------------------------------------------------ (i) fixture coverage
def test_fixture_shape(fx):
    assert len(fx["entries"]) == 407 and len(fx["samples"]) == 142
    assert {e[1] for e in fx["entries"]} == set(fx["samples"])
    assert len(rc.list_regexes("cn")) == 37 and len(rc.list_regexes("geolocation-!cn")) == 106
    assert fx["pinned"] == {"list": "apple", "name": "cdn4.apple-mapkit.com", "want": True}


def test_every_fixture_pattern_compiles(around):
    """None of the reference's 142 patterns may be refused; the largest DFA has 126
    states (^[a-z]([a-z0-9-]{0,61}[a-z0-9])?$) and no pattern more than 24 byte classes."""
    from hysteria_amd import acl
    most = [0, 0]
    for p, _ in around:
        st, states, classes = acl.regex_check(p)
        assert st == 0 and states <= acl.REGEX_MAX_STATES, (p, st, states)
        most = [max(most[0], states), max(most[1], classes)]
    assert most == [126, 24] and acl.regex_check(rc.BIG)[1] == 126


def test_generated_names_hit_and_miss(around):
    """For each pattern the oracle finds a matching and a non-matching generated name."""
    for p, names in around:
        hits = sum(rc.oracle(p, n) for n in names)
        assert 0 < hits < len(names), (p, hits, len(names))
        assert rc.oracle(p, names[0]), p   # the sample itself


# ------------------------------------------------------------------ (ii) fixture agreement
def test_fixture_patterns_agree_with_the_oracle(around):
    from hysteria_amd import acl
    n = 0
    for p, names in around:
        for name in names:
            assert acl.regex_match(p, name) == rc.oracle(p, name), (p, name)
            n += 1
    assert n > 15000   # about 140 names a pattern


def test_pinned_case(fx):
    """Test_geositeMatcher_Match, "regexp": cdn4.apple-mapkit.com matches geosite:apple."""
    from hysteria_amd import acl
    pin = fx["pinned"]
    assert any(acl.regex_match(v, pin["name"]) for v in rc.list_regexes(pin["list"])) is pin["want"]


# ------------------------------------------------------------------ (iii) exhaustive small cases
def test_small_patterns_on_every_short_name():
    """Seeded small in-subset patterns (alphabet a b . -, classes, | * + ? {m,n},
    ^ $, depth <= 3), each against every name of length <= 6 over {a, b, .} and
    against names with \\n, \\v and the other space bytes (traps a, b)."""
    from hysteria_amd import acl
    names = [bytes(t) for n in range(7) for t in itertools.product(b"ab.", repeat=n)]
    assert len(names) == 1093
    names += [b"\n", b"\x0b", b"a\n", b"\na", b"a\x0b", b"ab\n", b"a\nb", b" ", b"\t", b"\f", b"\r", b"a b", b"-", b"a-b",
              b"_", b"a\n\n", b"\n\n"]
    patterns = rc.small_patterns()
    kinds = [0, 0]
    for p in patterns:
        st, states, _ = acl.regex_check(p)
        assert st == 0, p
        for name in names:
            want = rc.oracle(p, name)
            assert acl.regex_match(p, name) == want, (p, name, want)
            kinds[want] += 1
    assert len(patterns) == 400 and min(kinds) > 50000, kinds


# ------------------------------------------------------------------ (iv) traps and refusals
def test_traps():
    from hysteria_amd import acl
    m = acl.regex_match
    # a: Go's \s has no \v
    assert [m(b"\\s", c) for c in (b"\t", b"\n", b"\x0b", b"\f", b"\r", b" ", b"a")] == [1, 1, 0, 1, 1, 1, 0]
    assert m(b"^\\S$", b"\x0b") and m(b"[\\s]", b" ") and not m(b"[\\s]", b"\x0b") and m(b"[^\\s]", b"\x0b")
    # b: '$' does not match before a trailing newline
    assert m(b"a$", b"a") and not m(b"a$", b"a\n") and not m(b"^$", b"\n") and m(b"a\n$", b"a\n")
    assert not m(b"a.$", b"a\n")           # '.' is every byte but \n
    # c: both anchors at position 0 of the empty name
    for p in (b"$^", b"^$", b"^^$$", b"($)(^)", b"$^$"):
        assert m(p, b"") and not m(p, b"a") and not m(p, b"\n"), p
    assert m(b"$", b"abc") and m(b"^", b"abc") and m(b"(^|x)$", b"x") and not m(b"(^|x)$", b"y")
    # d: '^' after a consumed byte never holds
    for name in (b"ab", b"a", b"b", b"", b"a\nb"):
        assert not m(b"a^b", name)
    assert not m(b"a$b", b"ab") and not m(b".^", b"a") and m(b"(^|\\.)a$", b".a") and not m(b"(^|\\.)a$", b"ba")


def test_semantics():
    """Unanchored on both sides, the pattern as it is (not lower-cased), the empty
    pattern and the empty name, empty branches, lazy marks, counted repeats."""
    from hysteria_amd import acl
    m = acl.regex_match
    assert m(b"b", b"abc") and not m(b"^b", b"abc") and not m(b"b$", b"abc") and m(b"^abc$", b"abc")
    assert not m(b"ABC", b"abc") and m(b"ABC", b"ABC")      # the name as given; the kernel lower-cases its names
    for name in (b"", b"a", b"\n", b"\xff\x80"):
        assert m(b"", name) and m(b"a|", name) and m(b"()", name) and m(b"(?:)", name) and m(b"x*", name)
    assert not m(b"a", b"") and m(b"^$", b"") and m(b".*", b"") and not m(b".+", b"")
    assert m(b"a+?b", b"aab") and m(b"a{2}?", b"aa") and not m(b"^a{2,3}?$", b"aaaa") and m(b"^a{2,}$", b"a" * 40)
    assert m(b"^a{1000}$", b"a" * 1000) and not m(b"^a{1000}$", b"a" * 999)
    assert m(b"^[^a]$", b"\xe9") and m(b"^.$", b"\x80") and m(b"^\\W\\D\\S$", b"\xc3\xa9\xff")   # bytes as they are
    assert m(b"^\\w+$", b"aZ09_") and not m(b"^\\w+$", b"a-b") and m(b"^[\\d\\-x]+$", b"1-x") and m(b"^[a\\]]+$", b"]a")
    assert m(b"^[a-]+$", b"a-") and m(b"^[-a]+$", b"-a") and m(b"^[\\.-9]+$", b"./0") and not m(b"^[\\.-9]+$", b"-")
    assert m(b"\\^\\$\\.\\|\\(\\)\\[\\]\\{\\}\\*\\+\\?\\\\", b"^$.|()[]{}*+?\\") and m(b"\\_\\-", b"_-")
    assert m(b"^(?:a|b(?:c|d))+$", b"abcbd") and m(b"^(a|(b|(c|(d))))$", b"d")
    assert acl.regex_check(b"^[a-z]{1,4}$") == (0, 6, 2)   # the start, four letters deep, and the dead end


REFUSED = [b"(?i)x", b"(?P<n>a)", b"(?s:a)", b"(?=a)", b"\\bfoo", b"a\\B", b"\\Aa", b"a\\z", b"\\pL", b"\\Qa\\E", b"\\x41",
           b"\\1", b"\\n", b"a\\", b"[[:alpha:]]", b"[a[b]", b"[]a]", b"[^]a]", b"[z-a]", b"[a-\\d]", b"[a", b"a{,3}",
           b"a{", b"a{x}", b"{1}", b"a{1,2", b"a{2,1}", b"a{1001}", b"a{1,1001}", b"a}", b"a]", b"a**", b"a+*", b"a?{2}",
           b"a*??", b"a{2}{3}", b"^*", b"$+", b"^{2}", b"*a", b"(*a)", b"a|*", b"(a", b"a)", b"caf\xc3\xa9", b"a\x80",
           b"a.{12}b$", b"(a{1000}){1000}", b"(" * 65 + b"a" + b")" * 65]


def test_refusals():
    """Every refusal of the header, one pattern each (and a few neighbours):
    HYOBFS_ACL_ERR_REGEX from regex_check and regex_match alike; a pattern longer
    than 255 bytes stays ERR_PATTERN; the neighbours just inside are taken."""
    from hysteria_amd import acl
    for p in REFUSED:
        assert acl.regex_check(p) == (acl.ERR_REGEX, 0, 0), p
        with pytest.raises(ValueError, match="-63"):
            acl.regex_match(p, b"a")
    assert acl.regex_check(b"a" * 256)[0] == acl.ERR_PATTERN and acl.regex_check(b"(?i)" + b"a" * 252)[0] == acl.ERR_PATTERN
    assert acl.regex_check(b"a" * 255)[0] == 0
    for p in (b"a{0,3}", b"a{1000}", b"a{0,1000}", b"a.{10}b$", b"(" * 64 + b"a" + b")" * 64, b"(?:a)", b"[a\\d]", b"a*?",
              b"(^)*", b"(a*)*", b"\\\n"):
        assert acl.regex_check(p)[0] == 0, p
    lib = acl._alib()
    assert lib.hyobfs_acl_regex_check(None, 1, None, None) == -2 and lib.hyobfs_acl_regex_check(None, 0, None, None) == 0
    assert lib.hyobfs_acl_regex_match(b"a", 1, None, 1) == -2 and lib.hyobfs_acl_regex_match(None, 0, None, 0) == 1
    assert acl.regex_check(b"a.{12}b$")[0] == acl.ERR_REGEX   # 2^13 states and more


def test_library_flags_and_bad_entry():
    """hyobfs_acl_ruleset_new_flags refuses before the device is looked at: without
    the flag every regex entry, with it the first one outside the subset, naming
    rule and entry; unknown flag bits are invalid; flags 0 is ruleset_new."""
    import ctypes

    from hysteria_amd import acl
    rules = [ac.R("all", 1), ac.R("domain_set", 2, entries=[("full", b"a.test"), ("regex", b"^ok$"), ("root", b"b.test"),
                                                            ("regex", b"\\bno"), ("regex", b"(?i)no")])]
    arr, keep = ac.c_rules(rules)
    for flags, entry in ((0, 1), (acl.FLAG_REGEX, 3)):
        with pytest.raises(acl.RuleRefused) as e:
            acl.ruleset_new(arr, 2, 0, flags)
        assert (e.value.status, e.value.rule, e.value.entry) == (acl.ERR_REGEX, 1, entry)
    lib = acl._alib()
    h = ctypes.c_void_p()
    assert lib.hyobfs_acl_ruleset_new_flags(arr, 2, 0, 2, ctypes.byref(h)) == -2
    assert lib.hyobfs_acl_ruleset_new_flags(arr, 2, 0, 3, ctypes.byref(h)) == -2
    assert (lib.hyobfs_acl_ruleset_bad_rule(), lib.hyobfs_acl_ruleset_bad_entry()) == (-1, -1)
    arr, keep = ac.c_rules([ac.R("domain_set", 2, entries=[("regex", b"a" * 256)])])
    with pytest.raises(acl.RuleRefused) as e:
        acl.ruleset_new(arr, 1, 0, acl.FLAG_REGEX)
    assert (e.value.status, e.value.rule, e.value.entry) == (acl.ERR_PATTERN, 0, 0)
    arr, keep = ac.c_rules([ac.R("exact", 1, pattern=b"x" * 256)])
    with pytest.raises(acl.RuleRefused) as e:
        acl.ruleset_new(arr, 1, 0, acl.FLAG_REGEX)
    assert (e.value.status, e.value.rule, e.value.entry) == (acl.ERR_PATTERN, 0, -1)


# ------------------------------------------------------------------ (v) the kernel under AddressSanitizer
@pytest.fixture(scope="module")
def acl_regex_main():
    """tests/emu/build/acl_regex_main: acl.hip + the driver, compiled for the host
    with AddressSanitizer (a program with its own main: nothing is preloaded).
    Rebuilt when a source is newer."""
    if not os.path.exists(CLANG):
        pytest.skip("no host clang for the emulated build")
    csrc = os.path.join(ROOT, "hysteria_amd", "csrc")
    srcs = [os.path.join(EMU, "acl_regex_main.cpp"), os.path.join(csrc, "acl.hip")]
    deps = srcs + [os.path.join(EMU, "hip_emu.h"), os.path.join(csrc, "kernels.h"), os.path.join(csrc, "acl_regex.h"),
                   os.path.join(ROOT, "include", "hyobfs_acl.h"), os.path.join(ROOT, "include", "hyobfs_sniff.h")]
    os.makedirs(os.path.join(EMU, "build"), exist_ok=True)
    exe = os.path.join(EMU, "build", "acl_regex_main")
    with open(os.path.join(EMU, "build", ".acl_regex_main.lock"), "w") as lk:
        fcntl.flock(lk, fcntl.LOCK_EX)
        if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(d) for d in deps):
            tmp = exe + ".tmp"
            subprocess.run([CLANG, "-std=c++20", "-O1", "-g", "-DHYOBFS_EMULATE", "-I" + EMU, "-I" + csrc, "-x", "c++",
                            "-fsanitize=address", "-fno-omit-frame-pointer", "-pthread",
                            "-Wno-unused-command-line-argument", *srcs, "-o", tmp], check=True, capture_output=True)
            os.replace(tmp, exe)
    return exe


def _run(exe, tmp_path, data, flags=1):
    path = tmp_path / "cases.bin"
    path.write_bytes(data)
    r = subprocess.run([exe, str(path), str(flags)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == "done"
    return lines[:-1]


def _check_groups(groups, lines, sniffed):
    at = 0
    for k, g in enumerate(groups):
        assert lines[at].split() == ["group", "0", "-1", "-1", str(len(g[1]))], (g[0], lines[at])
        exp = rc.expected(g, sniffed, k)
        got = [tuple(int(x) for x in ln.split()) for ln in lines[at + 1:at + 1 + len(exp)]]
        for i, (a, b) in enumerate(zip(got, exp)):
            assert a == b, (g[0], i, g[2][i], a, b)
        assert len(got) == len(exp)
        at += 1 + len(exp)
    assert at == len(lines)


def test_case_groups_cover_their_edges():
    """What the groups are there for, by the oracle alone."""
    exp = {g[0]: rc.expected(g) for g in rc.groups()}
    assert [e[1] for e in exp["rx_straddle"]][:10] == [0] * 8 + [-1, 1]
    assert [e[1] for e in exp["rx_130"]] == [0] * 9 + [1, 0, -1, 1]
    assert [e[2] for e in exp["rx_order"]] == [1000, 1002, 1003, 1003, 0]
    assert [e[1] for e in exp["rx_gating"]] == [-1, 1, 1, -1, 2, 0, 0, 0, 0, 0, -1]
    assert [e[1] for e in exp["rx_lengths"]][:3] == [1, 2, 2] and [e[1] for e in exp["rx_lengths"]][-3:] == [0, -1, -1]
    assert [e[1] for e in exp["rx_normalise"]] == [0, -1, 0, 3, 3, -1, 0]
    assert [e[0] for e in exp["rx_host"]] == [acl_ref.HOST] * 3 + [0, 0, acl_ref.HOST, acl_ref.HOST, 0]
    assert [e[1] for e in exp["rx_big"]] == [0, 0, -1, -1, 0, -1, 0, 0, -1, -1, -1, -1, -1, 0, 0, -1]
    assert [e[1] for e in exp["rx_pinned"]] == [0, -1, -1]
    cn = [e[1] for e in exp["rx_cn"]]
    assert cn.count(0) >= 37 + 2 and cn.count(1) >= 37
    assert len(exp["rx_items_1029"]) == 1029 and len({e for e in exp["rx_items_1029"]}) == 3


def test_emulated_kernel_both_entry_points(acl_regex_main, tmp_path):
    """Every group through hyobfs_acl_match_batch and hyobfs_acl_match_sniffed_batch
    under AddressSanitizer: the bytes between names poisoned, `res` exactly n
    records long, the rule sets made by hyobfs_acl_ruleset_new_flags."""
    groups = rc.groups()
    for mode in (0, 1):
        _check_groups(groups, _run(acl_regex_main, tmp_path, ac.case_file(groups, mode)), bool(mode))


def test_emulated_creation_refusals(acl_regex_main, tmp_path):
    """The driver's view of the refusals: without the flag the first regex entry,
    with it the first entry outside the subset, each with rule and entry."""
    rules = [ac.R("exact", 1, pattern=b"fine.test"),
             ac.R("domain_set", 2, entries=[("regex", b"^ok$"), ("full", b"a.test"), ("regex", b"a{,3}")])]
    groups = [("refused", rules, [])]
    assert _run(acl_regex_main, tmp_path, ac.case_file(groups, 0), 0) == ["group -63 1 0 0"]
    assert _run(acl_regex_main, tmp_path, ac.case_file(groups, 0), 1) == ["group -63 1 2 0"]
    assert _run(acl_regex_main, tmp_path, ac.case_file(groups, 0), 4) == ["group -2 -1 -1 0"]


# ------------------------------------------------------------------ (vi) the Python surface
class Geo:
    """The geo loader over the fixture's lists."""

    def __init__(self, fx):
        self.fx = fx

    def geoip(self, code):
        return None

    def geosite(self, name):
        got = [("regex", v, a) for n, v, a in self.fx["entries"] if n == name]
        got += [tuple(e) for e in self.fx["extra"].get(name, [])]
        return got or None


def test_compile_rules_opt_in(fx):
    """compile_rules keeps regex entries only with device_regex=True, applies the
    attribute filter first, and turns a refused pattern into a CompilationError
    with the rule's line and the library's status; without the switch, the old error."""
    from hysteria_amd import acl
    text = acl.parse_text_rules("a(geosite:apple)\n# c\nb(geosite:google@ads, tcp/443)\nc(geosite:google@cn)")
    outs = {"a": 1, "b": 2, "c": 3}
    with pytest.raises(acl.CompilationError) as e:
        acl.compile_rules(text, outs, Geo(fx))
    assert e.value.line_num == 1 and "cannot be matched on the device" in e.value.message
    rs = acl.compile_rules(text, outs, Geo(fx), device_regex=True)
    assert [len([x for x in r.entries if x[0] == "regex"]) for r in rs.rules] == [6, 1, 0]
    assert rs.flags() == acl.FLAG_REGEX and acl.compile_rules(text[2:], outs, Geo(fx)).flags() == 0
    arr, keep = rs.c_rules()
    assert arr[0].n_entries == len(rs.rules[0].entries) == 26
    # the host matcher, for the names the device leaves
    pin = fx["pinned"]
    assert rs.match_host(pin["name"]) == 0 and rs.match_host(pin["name"].upper() + ".") == 0
    assert rs.match_host("adservice.google.com", proto=1, port=443) == 1
    assert rs.match_host("adservice.google.com", proto=2, port=443) == -1
    assert rs.match_host("xadservice.google.com", proto=1, port=443) == -1

    class Bad(Geo):
        def geosite(self, name):
            return [("root", "fine.test", []), ("regex", "\\bword", []), ("regex", "(?i)skipped", ["x"])]
    with pytest.raises(acl.CompilationError) as e:
        acl.compile_rules(acl.parse_text_rules("\n\na(geosite:any)"), outs, Bad(fx), device_regex=True)
    assert e.value.line_num == 3 and "(-63)" in e.value.message and "bword" in e.value.message
    # the attribute filter comes first: with @x only the entry that is refused remains
    with pytest.raises(acl.CompilationError) as e:
        acl.compile_rules(acl.parse_text_rules("a(geosite:any@x)"), outs, Bad(fx), device_regex=True)
    assert "skipped" in e.value.message


def test_host_matcher_translation():
    """RuleSet.match_host evaluates regex entries with Go's meaning: the traps, and
    on every fixture pattern's names the same verdicts as the library's walk."""
    from hysteria_amd import acl

    def host(pattern, name):
        return acl.RuleSet([acl.Rule(acl.KIND_DOMAIN_SET, entries=[("regex", pattern)])]).match_host(name) == 0
    assert host("\\s", "a b") and not host("\\s", "a\x0bb") and host("\\S", "\x0b") and host("[^\\s]", "\x0b")
    assert not host("[\\s]", "\x0b") and host("[\\S]", "\x0b") and not host("[^\\S]", "\x0b") and host("[^\\Sa]", " ")
    assert host("a$", "a") and not host("a$", "a\n") and host("^$", "") and host("$^", "") and not host("$^", "a")
    assert not host("a^b", "ab") and host("^[^\\.]+$", "café") and host("^\\W$", "é") and host("[\\]a]", "]")
    assert host("^[a-c-]+$", "a-c") and host("^[\\d-]+$", "1-2") and not host("^A", "a") and host("^a", "A")
    fx = rc.fixture()
    for v, s in sorted(fx["samples"].items()):
        for name in rc.names_around(s.encode())[::7]:
            if name != name.lower().rstrip(b"."):
                continue
            assert host(v, name.decode()) == bool(acl.regex_match(v, name)), (v, name)


def test_structs_and_constants(tmp_path):
    """The new constants and entry points against the header, by a probe compiled with gcc."""
    from hysteria_amd import _lib, acl
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include "hyobfs_acl.h"\n'
                   '#ifdef SIGS\n'
                   'int (*f)(const hyobfs_acl_rule*, uint32_t, int, uint32_t, hyobfs_acl_ruleset**) = '
                   'hyobfs_acl_ruleset_new_flags;\n'
                   'int (*g)(const uint8_t*, uint32_t, uint32_t*, uint32_t*) = hyobfs_acl_regex_check;\n'
                   'int (*h)(const uint8_t*, uint32_t, const uint8_t*, uint32_t) = hyobfs_acl_regex_match;\n'
                   'int64_t (*k)(void) = hyobfs_acl_ruleset_bad_entry;\n'
                   '#else\nint main(void){\n'
                   'printf("%u %d %d\\n", HYOBFS_ACL_FLAG_REGEX, HYOBFS_ACL_REGEX_MAX_STATES, HYOBFS_ABI_VERSION);\n'
                   'return 0;}\n#endif\n')
    exe = tmp_path / "probe"
    gcc = ["gcc", "-std=c11", "-Werror", "-I", os.path.join(ROOT, "include"), str(src)]
    subprocess.run(gcc + ["-DSIGS", "-c", "-o", str(tmp_path / "sigs.o")], check=True)   # the declared signatures
    subprocess.run(gcc + ["-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert [int(x) for x in out] == [acl.FLAG_REGEX, acl.REGEX_MAX_STATES, _lib.ABI_VERSION]
    for name in ("hyobfs_acl_ruleset_new_flags", "hyobfs_acl_ruleset_bad_entry", "hyobfs_acl_regex_check",
                 "hyobfs_acl_regex_match"):
        assert name in _lib._ACL_SIG and name in _lib.header_functions()
