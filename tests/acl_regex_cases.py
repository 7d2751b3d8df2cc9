"""Cases for the geosite regex entries of the ACL matcher (include/hyobfs_acl.h,
"THE REGEX SUBSET"), shared by the CPU tier (tests/test_acl_regex.py) and the GPU
tier (tests/test_gpu_acl_regex.py).  TEST INFRASTRUCTURE ONLY.

The oracle is Python's ``re`` over bytes after the translation that Go's meaning
demands; tests/acl_ref.py is extended here (not edited) by a regex branch of
``geosite_matcher``.  Case groups are tests/acl_cases.py's (label, rules, items).
"""
import functools
import json
import os
import random
import re

import acl_cases as ac
import acl_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R, item, number = ac.R, ac.item, ac.number


@functools.lru_cache(maxsize=None)
def fixture():
    with open(os.path.join(ROOT, "tests", "golden", "geosite_regex.json"), encoding="utf-8") as f:
        return json.load(f)


def list_regexes(name, attrs=()):
    """The regex values of one fixture list that pass the attribute filter, in order."""
    return [v for n, v, a in fixture()["entries"] if n == name and all(x in a for x in attrs)]


# ------------------------------------------------------------------ the oracle
def to_py(pattern: bytes) -> bytes:
    """Go's pattern for Python's re: '^' -> \\A, '$' -> \\Z (Python's '$' also matches
    before a trailing newline: trap b), \\s and \\S spelled out (Go's \\s has no \\v:
    trap a).  \\S inside a class cannot be spelled and is not generated."""
    out, i, inclass = b"", 0, False
    while i < len(pattern):
        c = pattern[i:i + 1]
        if c == b"\\":
            e = pattern[i + 1:i + 2]
            i += 2
            if e == b"s":
                out += b"\\t\\n\\f\\r " if inclass else b"[\\t\\n\\f\\r ]"
            elif e == b"S":
                assert not inclass
                out += b"[^\\t\\n\\f\\r ]"
            else:
                out += b"\\" + e
            continue
        if inclass:
            inclass = c != b"]"
            out += c
        elif c == b"[":
            inclass = True
            out += c
            if pattern[i + 1:i + 2] == b"^":
                out += b"^"
                i += 1
        else:
            out += {b"^": b"\\A", b"$": b"\\Z"}.get(c, c)
        i += 1
    return out


@functools.lru_cache(maxsize=None)
def _compiled(pattern: bytes):
    return re.compile(to_py(pattern))


def oracle(pattern: bytes, name: bytes) -> bool:
    """regexp.MatchString(pattern, name), by Python's re."""
    return _compiled(pattern).search(name) is not None


# ------------------------------------------------------------------ acl_ref with a regex branch
def geosite_matcher(rule, host):
    """acl_ref.geosite_matcher, and a "regex" entry by the oracle."""
    rest = [e for e in rule["entries"] if e[0] != "regex"]
    if acl_ref.geosite_matcher(dict(rule, entries=rest), host):
        return True
    return any(oracle(v, host[0]) for t, v in rule["entries"] if t == "regex")


def match(rules, host, proto, port):
    host = (acl_ref.normalise(host[0]), host[1], host[2])
    for i, rule in enumerate(rules):
        if rule["proto"] != 0 and rule["proto"] != proto:
            continue
        if rule["start_port"] != 0 and (port < rule["start_port"] or port > rule["end_port"]):
            continue
        if (geosite_matcher if rule["kind"] == "domain_set" else acl_ref.MATCHERS[rule["kind"]])(rule, host):
            return i
    return -1


def expected_one(rules, it, sniff_status=None):
    """acl_ref.expected with the regex branch."""
    name, v4, v6, proto, port = it
    if sniff_status is not None and (sniff_status != 0 or len(name) == 0):
        return (acl_ref.NO_NAME, -1, 0, acl_ref.NO_HIJACK)
    if acl_ref.left_to_host(name):
        return (acl_ref.HOST, -1, 0, acl_ref.NO_HIJACK)
    r = match(rules, (name, v4, v6), proto, port)
    if r < 0:
        return (0, -1, 0, acl_ref.NO_HIJACK)
    return (0, r, rules[r]["outbound"], rules[r]["hijack"])


def expected(group, sniffed=False, k=0):
    _, rules, items = group
    st = ac.sniff_statuses(items, k) if sniffed else [None] * len(items)
    return [expected_one(rules, it, s) for it, s in zip(items, st)]


# ------------------------------------------------------------------ names around a matching sample
def names_around(sample: bytes):
    """The sample; every single-byte deletion, insertion and replacement of it; and
    the sample with a label, a '.' or a byte put before and after it.  The anchors
    (^|\\.) and $ are where a DFA goes wrong."""
    out = [sample]
    for i in range(len(sample) + 1):
        for c in (b"a", b".", b"0"):
            out.append(sample[:i] + c + sample[i:])
    for i in range(len(sample)):
        out.append(sample[:i] + sample[i + 1:])
        for c in (b"z", b".", b"9", b"-"):
            if sample[i:i + 1] != c:
                out.append(sample[:i] + c + sample[i + 1:])
    for pre in (b"www.", b".", b"w"):
        out.append(pre + sample)
    for post in (b".com", b".", b"m"):
        out.append(sample + post)
    out += [b"", b".", b"x" + sample + b"x"]
    return list(dict.fromkeys(out))


# ------------------------------------------------------------------ small in-subset patterns
def small_patterns(count=400, seed=11):
    """Seeded small patterns of the subset: alphabet a b . -, classes, | * + ?
    {m,n}, ^ $, AST depth <= 3."""
    rnd = random.Random(seed)
    atoms = [b"a", b"b", b"\\.", b"-", b".", b"[ab]", b"[^a]", b"[a.-]", b"[^\\.]", b"\\s", b"\\S", b"\\w", b"\\D", b"^",
             b"$"]
    reps = [b"*", b"+", b"?", b"{2}", b"{1,2}", b"{0,1}", b"{2,}", b"*?", b"+?"]

    def gen(depth):
        k = rnd.random()
        if depth == 0 or k < 0.35:
            return rnd.choice(atoms)
        if k < 0.6:
            return b"".join(gen(depth - 1) for _ in range(rnd.randrange(1, 4)))
        if k < 0.8:
            x = gen(depth - 1)
            if x in (b"^", b"$") or x == b"":
                return x
            if len(x) > 1 and not (x.startswith(b"[") and x.endswith(b"]") and x.count(b"[") == 1) \
                    and not (len(x) == 2 and x.startswith(b"\\")):
                x = rnd.choice((b"(", b"(?:")) + x + b")"
            return x + rnd.choice(reps)
        return b"(" + b"|".join(gen(depth - 1) for _ in range(rnd.randrange(1, 4))) + (b"|" if k > 0.97 else b"") + b")"

    out = []
    while len(out) < count:
        p = gen(3)
        if p not in out:
            out.append(p)
    return out


# ------------------------------------------------------------------ case groups for the kernel
BIG = b"^[a-z]([a-z0-9-]{0,61}[a-z0-9])?$"   # the fixture's largest DFA: 126 states


def _rx(*values, **kw):
    return R("domain_set", entries=[("regex", v) for v in values], **kw)


def groups():
    fx = fixture()
    out = []
    # item counts: a wave without an item, and more than one workgroup
    rules = number([_rx(b"(^|\\.)mimi[0-9]{3}\\.com$", b"^cdn(-cn)?[1-4]?\\.apple-mapkit\\.com$"), _rx(b"\\.test$")])
    pool = [b"mimi123.com", b"x.mimi123.com", b"xmimi123.com", b"cdn4.apple-mapkit.com", b"cdn5.apple-mapkit.com",
            b"a.test", b"a.tes", b"mimi12.com", b"cdn-cn.apple-mapkit.com", b"", b"mimi1234.com"]
    for n in (1, 3, 4, 5, 1029):
        out.append(("rx_items_%d" % n, rules, [item(pool[(7 * i) % len(pool)]) for i in range(n)]))
    # regex entries that straddle entry index 63 / 64 (they stand after the set's other entries)
    ents = [("root", b"r%d.pad.test" % k) for k in range(30)]
    ents = ents[:15] + [("regex", b"^s%d\\.edge\\.test$" % k) for k in range(8)] + ents[15:] \
        + [("full", b"f%d.pad.test" % k) for k in range(30)]
    rules = number([R("domain_set", entries=ents), R("exact", pattern=b"s9.edge.test")])
    out.append(("rx_straddle", rules, [item(b"s%d.edge.test" % k) for k in range(10)]
                + [item(b"r29.pad.test"), item(b"x.f29.pad.test"), item(b"f29.pad.test"), item(b"xs3.edge.test")]))
    # 130 regex entries: three steps
    rules = number([_rx(*[b"^e%d\\.rx[0-9]?\\.test$" % k for k in range(130)]), R("suffix", pattern=b"rx.test")])
    out.append(("rx_130", rules, [item(b"e%d.rx.test" % k) for k in (0, 1, 62, 63, 64, 65, 127, 128, 129, 130)]
                + [item(b"e64.rx7.test"), item(b"e64.rx77.test"), item(b"xe64.rx.test")]))
    # a regex rule before and after an exact rule that matches the same name: the first wins
    rules = number([_rx(b"^first\\."), R("exact", pattern=b"first.test"), R("exact", pattern=b"second.test"),
                    _rx(b"(first|second)\\.test$")])
    out.append(("rx_order", rules, [item(b"first.test"), item(b"second.test"), item(b"a.second.test"),
                                    item(b"afirst.test"), item(b"third.test")]))
    # protocol and port gating on a regex rule
    rules = number([_rx(b"gate", proto=2), _rx(b"gate", ports=(80, 90)), _rx(b"^gate$", proto=1, ports=(443, 443))])
    out.append(("rx_gating", rules, [item(b"gate", proto=p, port=q) for p in (1, 2) for q in (79, 80, 90, 91, 443)]
                + [item(b"xgatex", proto=1, port=443)]))
    # one whole fixture list: cn's regexes mixed with 200 of its root entries
    cn = list_regexes("cn")
    assert len(cn) == 37
    roots = [e[1].encode() for e in fx["extra"]["cn"]]
    ents = []
    for k, v in enumerate(roots):
        ents.append(("root", v))
        if k % 5 == 0 and k // 5 < len(cn):
            ents.append(("regex", cn[k // 5].encode()))
    rules = number([R("domain_set", entries=ents), R("all")])
    names = []
    for v in cn:
        s = fx["samples"][v].encode()
        names += [s, b"x" + s, s + b"x", s[1:]]
    names += [roots[0], b"www." + roots[199], b"x" + roots[7]]
    out.append(("rx_cn", rules, [item(x) for x in names]))
    # names of 0, 1, 63, 64, 65 and 255 bytes; the long ones walk ".+x$" to their end
    rules = number([_rx(b".+x$"), _rx(b"^$"), _rx(b"^.$")])
    names = [b"", b"x", b"a"]
    for n in (2, 63, 64, 65, 255):
        names += [b"a" * (n - 1) + b"x", b"a" * n, b"a" * (n - 2) + b"xa"]
    out.append(("rx_lengths", rules, [item(x) for x in names]))
    # normalisation in front of the pattern: trailing dots, upper-case input, an upper-case pattern
    rules = number([_rx(b"\\.com$"), _rx(b"^Upper"), _rx(b"^[A-Z]+$"), _rx(b"^upper\\.org$")])
    out.append(("rx_normalise", rules, [item(b"a.com..."), item(b"a.com.x"), item(b"A.COM."), item(b"UPPER.ORG"),
                                        item(b"Upper.org"), item(b"..."), item(b"CDN4.Apple-Mapkit.COM")]))
    # names left to the host, whatever the rules; empty names are NO_NAME in the sniffed form
    rules = number([_rx(b""), R("all")])
    out.append(("rx_host", rules, [item(b"xn--abc.com"), item(b"caf\xc3\xa9.fr"), item(b"a" * 256), item(b""),
                                   item(b"ok.test"), item(b"a\x80"), item(b"A.XN--b"), item(b"x")]))
    # the 126-state pattern
    rules = number([_rx(BIG)])
    names = [b"a", b"a" * 63, b"a" * 64, b"a-", b"ab-c", b"1a", b"a1", b"a" + b"-" * 61 + b"b", b"a" + b"-" * 62 + b"b",
             b"a.b", b"", b"-", b"a" * 62 + b"-", b"z" * 62 + b"9", b"A", b"a" * 255]
    out.append(("rx_big", rules, [item(x) for x in names]))
    # the reference's pinned case: Test_geositeMatcher_Match, "regexp"
    pin = fx["pinned"]
    rules = number([_rx(*[v.encode() for v in list_regexes(pin["list"])])])
    out.append(("rx_pinned", rules, [item(pin["name"].encode()), item(b"cdn5.apple-mapkit.com"),
                                     item(b"x" + pin["name"].encode())]))
    return out
