"""CPU tier of the ACL matcher (include/hyobfs_acl.h): the Python restatement
(tests/acl_ref.py) against the reference's own tables (tests/golden/
acl_vectors.json), the product's parser, compiler and host matcher
(hysteria_amd/acl.py) against the same tables and against the restatement, and
the kernel itself through a stand-alone AddressSanitizer build (tests/emu/
acl_main.cpp + acl.hip against hip_emu.h, run as a child process)."""
import collections
import ctypes
import fcntl
import ipaddress
import itertools
import json
import os
import subprocess

import pytest

import acl_cases as ac
import acl_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
CLANG = "/opt/rocm/llvm/bin/clang++"


@pytest.fixture(scope="module")
def vectors():
    with open(os.path.join(ROOT, "tests", "golden", "acl_vectors.json"), encoding="utf-8") as f:
        return json.load(f)


def _ip16(text):
    """net.ParseIP / net.IPv4: always the 16-byte form."""
    if text is None:
        return None
    b = ipaddress.ip_address(text).packed
    return acl_ref.V4_IN_V6 + b if len(b) == 4 else b


class Geo:
    """The geo loader over the vectors' hand-written lists."""

    def __init__(self, v):
        self.v = v

    def geoip(self, code):
        g = self.v["geoip"].get(code)
        return None if g is None else ([(ipaddress.ip_address(a).packed, p) for a, p in g["cidrs"]], g["inverse"])

    def geosite(self, name):
        g = self.v["geosite"].get(name)
        return None if g is None else [tuple(e) for e in g]


def _text_rules(rows):
    from hysteria_amd.acl import TextRule
    return [TextRule(r["outbound"], r["address"], r["proto_port"], r["hijack_address"], i + 1) for i, r in enumerate(rows)]


def _ref_rules(ruleset):
    """A compiled RuleSet as the restatement's rule dicts."""
    out = []
    for r in ruleset.rules:
        d = ac.R(ac.KINDS[r.kind], r.outbound, r.proto, (r.start_port, r.end_port),
                 acl_ref.NO_HIJACK if r.hijack is None else ruleset.hijacks.index(r.hijack))
        d.update(pattern=r.pattern.encode(), ip=r.ip, prefix=r.prefix, inverse=r.inverse,
                 entries=[(e[0], e[1].encode()) if r.kind == 6 else e for e in r.entries])
        out.append(d)
    return out


# ------------------------------------------------------------------ the restatement and the host matcher
def test_restatement_ip_and_cidr_tables(vectors):
    """Test_ipMatcher_Match and Test_cidrMatcher_Match (matchers_test.go:8-141), in
    the 16-byte forms the reference's table builds and in the ABI's 4-byte forms."""
    from hysteria_amd import acl
    for row in vectors["ip_matcher"]:
        for form in (_ip16, lambda t: None if t is None else ipaddress.ip_address(t).packed):
            rule = ac.R("ip", 1, ip=form(row["ip"]))
            host = (b"", form(row["ipv4"]), _ip16(row["ipv6"]))
            assert acl_ref.ip_matcher(rule, host) == row["want"], row["name"]
        rs = acl.RuleSet([acl.Rule(acl.KIND_IP, ip=ipaddress.ip_address(row["ip"]).packed)])
        assert (rs.match_host("", row["ipv4"], row["ipv6"]) == 0) == row["want"], row["name"]
    for row in vectors["cidr_matcher"]:
        net = acl.parse_cidr(row["cidr"])
        rule = ac.R("cidr", 1, ip=net[0], prefix=net[1])
        assert acl_ref.cidr_matcher(rule, (b"", _ip16(row["ipv4"]), _ip16(row["ipv6"]))) == row["want"], row["name"]
        rs = acl.RuleSet([acl.Rule(acl.KIND_CIDR, ip=net[0], prefix=net[1])])
        assert (rs.match_host("", row["ipv4"], row["ipv6"]) == 0) == row["want"], row["name"]


def test_restatement_and_host_matcher_domain_table(vectors):
    """Test_domainMatcher_Match (matchers_test.go:143-351), the IDN rows included,
    through the restatement and through the product's host matcher."""
    from hysteria_amd import acl
    kinds = {0: acl.KIND_DOMAIN_EXACT, 1: acl.KIND_DOMAIN_WILDCARD, 2: acl.KIND_DOMAIN_SUFFIX}
    idn = 0
    for row in vectors["domain_matcher"]:
        mode = vectors["domain_modes"][str(row["mode"])]
        rule = ac.R(mode, 1, pattern=row["pattern"].encode())
        assert acl_ref.domain_matcher(rule, (row["host"].encode(), None, None)) == row["want"], row["name"]
        rs = acl.RuleSet([acl.Rule(kinds[row["mode"]], pattern=row["pattern"])])
        assert (rs.match_host(row["host"]) == 0) == row["want"], row["name"]
        assert (rs.match_host(row["host"].encode()) == 0) == row["want"], row["name"]
        idn += "IDN" in row["name"]
        if "IDN" in row["name"]:   # the device leaves every one of these names to the host
            assert acl_ref.left_to_host(row["host"].encode()), row["name"]
    assert idn == 8


def test_compile_table(vectors):
    """TestCompile (compile_test.go:25-363): the product's compiler, then the
    restatement's Match and the product's host matcher over the compiled rules."""
    from hysteria_amd import acl
    v = vectors["compile"]
    rs = acl.compile_rules(_text_rules(v["rules"]), v["outbounds"], Geo(v))
    assert [r.kind for r in rs.rules] == [1, 2, 0, 1, 2, 4, 3, 7, 6, 6, 5, 0, 3]
    assert rs.rules[12].pattern == "dotpattern.test"
    assert [e[1] for e in rs.rules[9].entries] == ["gstatic-cn.com", "www.google.cn", "googleapis-cn"]   # @cn only
    rules = _ref_rules(rs)
    for t in v["tests"]:
        host = (t["name"].encode(), _ip16(t["ipv4"]), _ip16(t["ipv6"]))
        r = acl_ref.match(rules, host, t["proto"], t["port"])
        want = (t["want_outbound"], t["want_ip"])
        assert rs.decision(r) == want, t
        assert rs.decision(rs.match_host(t["name"], t["ipv4"], t["ipv6"], t["proto"], t["port"])) == want, t
    with pytest.raises(acl.CompilationError) as e:
        acl.compile_rules(_text_rules(v["invalid_rules"]), v["invalid_outbounds"], Geo(v))
    assert e.value.line_num == 1 and "*/3-1" in str(e.value)


def test_host_matcher_equals_restatement_on_every_case():
    """RuleSet.match_host (the one CPU path) against acl_ref.match on every case
    group, the names the device would leave to the host included."""
    from hysteria_amd import acl
    n = 0
    for label, rules, items in ac.all_groups():
        rs = acl.RuleSet(ac.product_rules(rules))
        for it in items[:256]:
            assert rs.match_host(it[0], it[1], it[2], it[3], it[4]) == acl_ref.match(rules, it[:3], it[3], it[4]), \
                (label, it)
            n += 1
    assert n > 1200


# ------------------------------------------------------------------ parser and compiler
def test_parse_text_rules(vectors):
    """TestParseTextRules (parse_test.go:8-70)."""
    from hysteria_amd import acl
    for case in vectors["parse"]:
        if case["want_err"]:
            with pytest.raises(acl.InvalidSyntaxError) as e:
                acl.parse_text_rules(case["text"])
            assert e.value.line_num == 1
        else:
            got = [r._asdict() for r in acl.parse_text_rules(case["text"])]
            assert got == case["want"], case["name"]
    with pytest.raises(acl.InvalidSyntaxError) as e:
        acl.parse_text_rules("direct(all)\n\n# c\nwhat is this\n")
    assert (e.value.line_num, e.value.line) == (4, "what is this") and "line 4" in str(e.value)
    with pytest.raises(acl.InvalidSyntaxError):
        acl.parse_text_rules("direct(all)\nx")   # no newline at the end: '$' is the end of the text
    for case in vectors["parse_geosite_name"]:
        assert acl.parse_geosite_name(case["s"]) == (case["want"], case["want_attrs"]), case["name"]


def test_parse_proto_port():
    """parseProtoPort (compile.go:175-233)."""
    from hysteria_amd.acl import parse_proto_port as pp
    assert pp("") == pp("*") == pp("*/*") == (0, 0, 0)
    assert pp("TCP") == (1, 0, 0) and pp("udp") == (2, 0, 0) and pp("udp/*") == (2, 0, 0)
    assert pp("tcp/80") == (1, 80, 80) and pp("*/8888") == (0, 8888, 8888) and pp("tcp/6881-6889") == (1, 6881, 6889)
    assert pp("udp/ 10-20 ") == (2, 10, 20)     # the range form is trimmed
    for bad in ("icmp", "icmp/1", "*/3-1", "tcp/65536", "tcp/", "tcp/-1", "tcp/ 80", "tcp/1-", "tcp/a", "/80", "tcp/1-2-3",
                "tcp/+80"):
        assert pp(bad) is None, bad


def test_compile_errors(vectors):
    """Compile's refusals (compile.go:135-152, :235-316), each with its line."""
    from hysteria_amd import acl
    geo = Geo(vectors["compile"])

    def err(text, outbounds=("a",), geo=geo):
        with pytest.raises(acl.CompilationError) as e:
            acl.compile_rules(acl.parse_text_rules(text), {o: 1 for o in outbounds}, geo)
        return e.value.line_num, e.value.message

    assert err("a(all)\nb(all)") == (2, "outbound b not found")
    assert err("\n\na(1.1.2.0/24, */3-1)") == (3, "invalid protocol/port: */3-1")
    assert err("a(suffix:)") == (1, "empty domain suffix")
    assert err("a(suffix:.)") == (1, "empty domain suffix")
    assert err("a(1.2.3.4/33)") == (1, "invalid CIDR address: 1.2.3.4/33")
    assert err("a(1.2.3/24)")[1] == "invalid CIDR address: 1.2.3/24"
    assert err("a(::1/129)")[1] == "invalid CIDR address: ::1/129"
    assert err("a(1.2.3.4/)")[1] == "invalid CIDR address: 1.2.3.4/"
    assert err("a(all,*,not-an-ip)") == (1, "invalid hijack address (must be an IP address): not-an-ip")
    assert err("a(geoip:)")[1] == "empty GeoIP country code"
    assert err("a(geoip:kp)")[1] == "GeoIP country code kp not found"
    assert err("a(geosite:@cn)")[1] == "empty GeoSite name"
    assert err("a(geosite:nothing)")[1] == "GeoSite name nothing not found"
    assert "regex" in err("a(all)\na(geosite:google@ads)")[1]          # a device limit, with the rule's line
    assert err("a(geoip:jp)", geo=None)[0] == 1 and err("a(geosite:4chan)", geo=None)[0] == 1
    assert "longer than 255" in err("a(%s)" % ("x" * 256))[1]
    # the outbound's name is looked up in lower case; the address decides the matcher in the reference's order
    rs = acl.compile_rules(acl.parse_text_rules("A(ALL)\na(*)\na(1.2.3.4)\na(::FFFF:1.2.3.4/120)\na(x*.Y)\na(x.y.)"), {"a": 7})
    assert [r.kind for r in rs.rules] == [0, 0, 1, 2, 4, 3] and rs.rules[4].pattern == "x*.y"
    assert (rs.rules[3].ip, rs.rules[3].prefix) == (ipaddress.ip_address("::ffff:1.2.3.0").packed, 120)


# ------------------------------------------------------------------ the case sets
def test_random_set_is_balanced():
    """Of the 2048 random items every rule kind decides at least 5 %, no rule at
    least 10 %, and at most 5 % are left to the host, by the restatement alone."""
    group = ac.random_group()
    assert len(group[1]) == 96 and len(group[2]) == 2048
    kinds = collections.Counter()
    for st, rule, _, _ in ac.expected(group):
        kinds["host" if st == acl_ref.HOST else "none" if rule < 0 else group[1][rule]["kind"]] += 1
    for k in ac.KINDS:
        assert kinds[k] >= 0.05 * 2048, kinds
    assert kinds["none"] >= 0.10 * 2048 and 0 < kinds["host"] <= 0.05 * 2048, kinds


def test_case_families_cover_their_edges():
    """Spot checks that pin what the families are there for."""
    exp = {g[0]: ac.expected(g) for g in ac.all_groups(0)}
    mp = [e[2] for e in exp["match_position"]]
    assert mp[:2] == [1063, 1064] and mp[4:8] == [2010, 2005, 2070, 1129] and mp[8:11] == [0, 2100, 2040]
    assert [e[0] for e in exp["name_lengths_all"]] == [acl_ref.HOST, acl_ref.HOST, 0, 0, 0]
    assert all(e[0] == acl_ref.HOST for e in exp["host_decided"][:8] + exp["host_decided"][12:15])
    assert all(e[0] == 0 for e in exp["host_decided"][8:12] + exp["host_decided"][15:17])
    assert [e[1] for e in exp["suffix"][:4]] == [0, 0, 0, -1]
    k = ac.WILDCARD_PATTERNS.index(b"*a*a*a*a*a*b")
    assert [e[1] for e in exp["wildcard_%d" % k]][14:16] == [-1, 0]           # 255 a's; 254 a's and a b
    assert [e[1] for e in exp["cidr_ip_8"]][:4] == [0, -1, 0, -1]             # the v4-mapped network, prefix < 96
    assert [e[1] for e in exp["cidr_ip_10"]][:3] == [-1, -1, -1]
    assert exp["cidr_set_size_0_inverse"][0][1] == 1 and exp["cidr_set_size_0"][0][1] == -1
    assert exp["cidr_set_unmasked"] != exp["cidr_set_size_2"]
    assert {e[1] for e in exp["cidr_set_size_1000"]} == {-1, 1}


def test_iterative_wildcard_equals_the_recursive_one():
    """The kernel's form of deepMatchRune (acl.hip wildcard(): remember the last '*',
    on a mismatch let it take one more byte), restated here, against the
    reference's recursion on every name over {a, b} and every pattern over
    {a, b, *} up to length 6."""
    def iterative(name, pattern):
        s = q = mark = 0
        star = -1
        while s < len(name):
            pc = pattern[q] if q < len(pattern) else None
            if pc == "*":
                star = q
                q += 1
                mark = s
            elif pc == name[s]:
                s += 1
                q += 1
            elif star >= 0:
                q = star + 1
                mark += 1
                s = mark
            else:
                return False
        while q < len(pattern) and pattern[q] == "*":
            q += 1
        return q == len(pattern)

    names = ["".join(t) for n in range(7) for t in itertools.product("ab", repeat=n)]
    n = 0
    for m in range(7):
        for t in itertools.product("ab*", repeat=m):
            p = "".join(t)
            for name in names:
                assert iterative(name, p) == acl_ref.deep_match_rune(name, p), (name, p)
                n += 1
    assert n == 127 * 1093


# ------------------------------------------------------------------ the kernel on the CPU
@pytest.fixture(scope="module")
def acl_main():
    """tests/emu/build/acl_main: acl.hip + the driver, compiled for the host with
    AddressSanitizer (a program with its own main: nothing is preloaded).
    Rebuilt when a source is newer."""
    if not os.path.exists(CLANG):
        pytest.skip("no host clang for the emulated build")
    csrc = os.path.join(ROOT, "hysteria_amd", "csrc")
    srcs = [os.path.join(EMU, "acl_main.cpp"), os.path.join(csrc, "acl.hip")]
    deps = srcs + [os.path.join(EMU, "hip_emu.h"), os.path.join(csrc, "kernels.h"),
                   os.path.join(ROOT, "include", "hyobfs_acl.h"), os.path.join(ROOT, "include", "hyobfs_sniff.h")]
    os.makedirs(os.path.join(EMU, "build"), exist_ok=True)
    exe = os.path.join(EMU, "build", "acl_main")
    with open(os.path.join(EMU, "build", ".acl_main.lock"), "w") as lk:
        fcntl.flock(lk, fcntl.LOCK_EX)
        if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(d) for d in deps):
            tmp = exe + ".tmp"
            subprocess.run([CLANG, "-std=c++20", "-O1", "-g", "-DHYOBFS_EMULATE", "-I" + EMU, "-I" + csrc, "-x", "c++",
                            "-fsanitize=address", "-fno-omit-frame-pointer", "-pthread",
                            "-Wno-unused-command-line-argument", *srcs, "-o", tmp], check=True, capture_output=True)
            os.replace(tmp, exe)
    return exe


def _run(exe, tmp_path, data):
    path = tmp_path / "cases.bin"
    path.write_bytes(data)
    r = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == "done"
    return lines[:-1]


def _check_groups(groups, lines, sniffed):
    at = 0
    for k, g in enumerate(groups):
        assert lines[at].split() == ["group", "0", "-1", str(len(g[1]))], (g[0], lines[at])
        exp = ac.expected(g, sniffed, k)
        got = [tuple(int(x) for x in ln.split()) for ln in lines[at + 1:at + 1 + len(exp)]]
        for i, (a, b) in enumerate(zip(got, exp)):
            assert a == b, (g[0], i, g[2][i], a, b)
        assert len(got) == len(exp)
        at += 1 + len(exp)
    assert at == len(lines)


def test_emulated_match_batch(acl_main, tmp_path):
    """Every case family through hyobfs_acl_match_batch under AddressSanitizer, the
    gaps between names poisoned and `res` exactly n records long."""
    groups = ac.all_groups(random_items=160)   # the whole random set runs in the GPU tier
    assert {g[0].rstrip("_0123456789") for g in groups} >= {"rule_count", "match_position", "proto_port", "name_lengths",
                                                           "normalisation", "host_decided", "suffix", "wildcard",
                                                           "domain_sets", "cidr_ip", "cidr_set_size", "random"}
    _check_groups(groups, _run(acl_main, tmp_path, ac.case_file(groups, 0)), False)


def test_emulated_match_sniffed_batch(acl_main, tmp_path):
    """Every family (its edge groups) through hyobfs_acl_match_sniffed_batch: names in rows of
    name_stride bytes with the rest of each row poisoned; every 7th item a failed
    sniff and every empty name NO_NAME, their rows poisoned whole."""
    groups = ac.family_samples()
    exp = [e for k, g in enumerate(groups) for e in ac.expected(g, True, k)]
    kinds = collections.Counter(e[0] for e in exp)
    assert kinds[acl_ref.NO_NAME] > 60 and kinds[acl_ref.HOST] > 20 and kinds[0] > 300, kinds
    _check_groups(groups, _run(acl_main, tmp_path, ac.case_file(groups, 1)), True)


def test_emulated_null_addresses(acl_main, tmp_path):
    """ip_flags, ipv4 and ipv6 null: no item has an address."""
    groups = []
    for label, rules, items in ac.normalisation_groups() + ac.cidr_set_groups()[:2] + ac.cidr_ip_groups()[:1]:
        groups.append((label, rules, [(it[0], None, None, it[3], it[4]) for it in items]))
    for mode in (0, 1):
        _check_groups(groups, _run(acl_main, tmp_path, ac.case_file(groups, mode, null_ips=True)), bool(mode))


def test_emulated_creation_refusals(acl_main, tmp_path):
    """hyobfs_acl_ruleset_new refuses, with the rule's index: a regex entry, an
    over-long pattern or set value, a null pattern, null entries with a count, a
    bad family or prefix, an unknown kind or protocol."""
    ok = ac.R("exact", 1, pattern=b"fine.test")
    bad = [
        (ac.R("domain_set", 1, entries=[("full", b"a.test"), ("regex", b"^a.*$")]), -63),
        (ac.R("exact", 1, pattern=b"x" * 256), -64),
        (ac.R("domain_set", 1, entries=[("plain", b"y" * 256)]), -64),
        (ac.R("suffix", 1, null_pattern=True), -2),
        (ac.R("domain_set", 1, entries=[("full", b"a.test")], entries_null=True), -2),
        (ac.R("cidr_set", 1, entries=[(ac.ip("1.2.3.0"), 24)], entries_null=True, inverse=False), -2),
        (ac.R("cidr", 1, ip=ac.ip("1.2.3.0"), prefix=33), -2),
        (ac.R("cidr", 1, ip=ac.ip("::"), prefix=129), -2),
        (ac.R("ip", 1, ip=ac.ip("1.2.3.4"), family=5), -2),
        (ac.R("cidr_set", 1, entries=[(ac.ip("1.2.3.0"), 40)], inverse=False), -2),
        (ac.R("exact", 1, pattern=b"a", proto=3), -2),
    ]
    groups = [("refused_%d" % k, [dict(ok)] * (k % 3) + [r], []) for k, (r, _) in enumerate(bad)]
    groups.append(("fine", [dict(ok), ac.R("exact", 2, pattern=b"x" * 255)], [ac.item(b"x" * 255)]))
    lines = _run(acl_main, tmp_path, ac.case_file(groups, 0))
    for k, (_, st) in enumerate(bad):
        assert lines[k].split() == ["group", str(st), str(k % 3), "0"], (k, lines[k])
    assert lines[len(bad):] == ["group 0 -1 2", "0 1 2 %d" % acl_ref.NO_HIJACK]


# ------------------------------------------------------------------ the Python surface without a GPU
def test_library_refuses_rules_before_the_device_check():
    """The product library validates every rule before it looks at the device, so
    a refusal is the same on a machine without a GPU; an unknown kind too."""
    from hysteria_amd import acl
    for rule, st in ((ac.R("domain_set", 1, entries=[("regex", b".*")]), acl.ERR_REGEX),
                     (ac.R("wildcard", 1, pattern=b"*" * 256), acl.ERR_PATTERN)):
        arr, keep = ac.c_rules([ac.R("all", 1), rule])
        with pytest.raises(acl.RuleRefused) as e:
            acl.ruleset_new(arr, 2, 0)
        assert (e.value.status, e.value.rule) == (st, 1)
    arr, keep = ac.c_rules([ac.R("suffix", 1, pattern=b"x")])
    arr[0].pattern = None
    with pytest.raises(acl.RuleRefused) as e:
        acl.ruleset_new(arr, 1, 0)
    assert (e.value.status, e.value.rule) == (-2, 0)
    arr[0].kind = 8
    with pytest.raises(acl.RuleRefused):
        acl.ruleset_new(arr, 1, 0)
    lib = acl._alib()
    h = ctypes.c_void_p()
    assert lib.hyobfs_acl_ruleset_new(None, 1, 0, ctypes.byref(h)) == -2
    assert lib.hyobfs_acl_ruleset_new(None, 0, 0, None) == -2
    assert lib.hyobfs_acl_ruleset_bad_rule() == -1


def test_library_has_the_acl_entry_points():
    from hysteria_amd import acl
    lib = acl._alib()
    assert lib.hyobfs_acl_ruleset_rules(None) == 0
    lib.hyobfs_acl_ruleset_free(None)
    # n == 0 is OK before any pointer is looked at; a null required pointer is INVALID
    assert lib.hyobfs_acl_match_batch(None, None, None, None, None, None, None, None, None, 0, None, None) == 0
    assert lib.hyobfs_acl_match_sniffed_batch(None, None, 0, None, None, None, None, None, None, 0, None, None) == 0
    assert lib.hyobfs_acl_match_batch(None, None, None, None, None, None, None, None, None, 1, None, None) == -2
    assert lib.hyobfs_acl_match_sniffed_batch(None, None, 0, None, None, None, None, None, None, 1, None, None) == -2


def test_structs_match_header(tmp_path):
    """The ctypes and numpy mirrors of hyobfs_acl.h's structs, its status codes
    and kinds, against a probe compiled with gcc."""
    from hysteria_amd import acl
    structs = (("hyobfs_acl_rule", acl.HyobfsAclRule), ("hyobfs_acl_domain", acl.HyobfsAclDomain),
               ("hyobfs_acl_cidr", acl.HyobfsAclCidr))
    body, want = [], []
    for ct, cls in structs:
        for f, _ in cls._fields_:
            body.append(f'printf("%zu\\n", offsetof({ct}, {f}));')
            want.append(getattr(cls, f).offset)
        body.append(f'printf("%zu\\n", sizeof({ct}));')
        want.append(ctypes.sizeof(cls))
    for f in acl.ACL_RESULT_DTYPE.names:
        body.append(f'printf("%zu\\n", offsetof(hyobfs_acl_result, {f}));')
        want.append(acl.ACL_RESULT_DTYPE.fields[f][1])
    body.append('printf("%zu\\n", sizeof(hyobfs_acl_result));')
    want.append(acl.ACL_RESULT_DTYPE.itemsize)
    consts = ["HYOBFS_ACL_ERR_NO_NAME", "HYOBFS_ACL_ERR_HOST", "HYOBFS_ACL_ERR_REGEX", "HYOBFS_ACL_ERR_PATTERN",
              "HYOBFS_ACL_MAX_NAME", "HYOBFS_ACL_ALL", "HYOBFS_ACL_IP", "HYOBFS_ACL_CIDR", "HYOBFS_ACL_DOMAIN_EXACT",
              "HYOBFS_ACL_DOMAIN_WILDCARD", "HYOBFS_ACL_DOMAIN_SUFFIX", "HYOBFS_ACL_DOMAIN_SET", "HYOBFS_ACL_CIDR_SET",
              "HYOBFS_ACL_DOMAIN_PLAIN", "HYOBFS_ACL_DOMAIN_REGEX", "HYOBFS_ACL_DOMAIN_ROOT", "HYOBFS_ACL_DOMAIN_FULL",
              "HYOBFS_ABI_VERSION"]
    body += [f'printf("%d\\n", (int){c});' for c in consts]
    want += [acl.ERR_NO_NAME, acl.ERR_HOST, acl.ERR_REGEX, acl.ERR_PATTERN, acl.MAX_NAME, *range(8), *range(4), 4]
    assert (acl.ERR_NO_NAME, acl.ERR_HOST, acl.MAX_NAME) == (acl_ref.NO_NAME, acl_ref.HOST, acl_ref.MAX_NAME)
    assert [ac.KINDS.index(k) for k in ac.KINDS] == list(range(8)) and ac.DOMAIN_TYPES == acl._DOMAIN_TYPES
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hyobfs_acl.h"\nint main(void){\n' + "\n".join(body)
                   + "\nreturn 0;}\n")
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    vals = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert vals == want


def test_package_exports():
    import hysteria_amd
    for name in ("acl", "RuleSet", "TextRule", "parse_text_rules", "compile_rules", "CompilationError",
                 "InvalidSyntaxError", "ACL_RESULT_DTYPE", "quic_sniff_and_match"):
        assert name in hysteria_amd.__all__ and hasattr(hysteria_amd, name)
