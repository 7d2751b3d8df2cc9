"""The outbound ACL -- ``extras/outbounds/acl`` on MI355X: text rules are parsed and
compiled on the host, matched for whole batches of hosts on the GPU.

==================================================  ==================================================
reference (Go)                                      here
==================================================  ==================================================
``TextRule`` (parse.go:28-34)                       ``TextRule``
``ParseTextRules`` / ``InvalidSyntaxError``         ``parse_text_rules(text)`` / ``InvalidSyntaxError``
(parse.go:9-72)
``Compile`` / ``CompilationError``                  ``compile_rules(text_rules, outbounds, geo)`` /
(compile.go:111-161)                                ``CompilationError``
``parseProtoPort`` (compile.go:175-233)             ``parse_proto_port``
``compileHostMatcher`` (compile.go:235-316)         ``compile_host_matcher``
``parseGeoSiteName`` (compile.go:318-326)           ``parse_geosite_name``
``GeoLoader`` (compile.go:120-123)                  ``geo``: ``geoip(code)``, ``geosite(name)``
``compiledRule`` (compile.go:53-60)                 ``Rule`` -> ``hyobfs_acl_rule``
``compiledRuleSetImpl.Match`` (compile.go:88-109)   ``RuleSet.match_batch`` / ``match_sniffed_batch``
                                                    (GPU), ``RuleSet.match_many`` (lists in and out)
``Sniffer.UDP``, then ``Match``                     ``quic_sniff_and_match`` (GPU, one stream)
the matchers (matchers.go, matchers_v2geo.go)       ``include/hyobfs_acl.h`` states them;
                                                    ``RuleSet.match_host`` for the names the device
                                                    leaves to the host
==================================================  ==================================================

Matching runs in ``libhyobfs.so`` (``include/hyobfs_acl.h`` states the rules and
the one divergence).  A geosite entry of type regex goes to the device only on
request (``compile_rules(..., device_regex=True)``) and only if the library takes
its pattern (``regex_check``; the header's "THE REGEX SUBSET"); without the
switch such an entry is a CompilationError, as before.  The full and root values
of a large geosite list are looked up in a hash table on the device instead of
walked one by one, again on request (``compile_rules(..., device_index=True)``;
the header's "THE INDEX"); no result changes.  The device leaves three kinds of names to the host (a byte
>= 0x80, ``xn--`` anywhere, more than 255 bytes), because ``domainMatcher`` runs
``idna.ToUnicode`` on the name; ``match_many`` finishes exactly those items with
``RuleSet.match_host``, which decodes ``xn--`` labels with the standard
library's punycode codec and keeps the undecoded name on any error.  That is the
one CPU path, and only for those names.  It evaluates a regex entry with ``re``
under ``re.ASCII`` on the decoded name, after the translation that Go's
semantics demand (``_regex_to_py``).  STATED DIVERGENCE: a name that is not valid
UTF-8 is decoded with U+FFFD in place of each invalid sequence as Python
delimits it; Go walks such bytes as one U+FFFD rune per byte.

Out of scope: reading geoip / geosite ``.dat`` files (``geo`` hands the lists
over), the outbounds themselves, the resolver, and the LRU cache of
compile.go:79 (it only remembers results).
"""
from __future__ import annotations

import collections
import ctypes
import ipaddress
import re

import numpy as np

from . import _lib, quic, sniff
from ._dev import _pack, _ptr, _records, _stream, _to

MAX_NAME = 255
NO_HIJACK = 0xFFFFFFFF
FLAG_REGEX = 1              # HYOBFS_ACL_FLAG_REGEX
FLAG_INDEX = 2              # HYOBFS_ACL_FLAG_INDEX (hyobfs_acl_options.flags only)
INDEX_MIN_DEFAULT = 65      # HYOBFS_ACL_INDEX_MIN_DEFAULT
REGEX_MAX_STATES = 4096     # HYOBFS_ACL_REGEX_MAX_STATES
PROTO_BOTH, PROTO_TCP, PROTO_UDP = 0, 1, 2

ERR_NO_NAME, ERR_HOST, ERR_REGEX, ERR_PATTERN = range(-61, -65, -1)
ERRORS = {
    ERR_NO_NAME: "no sniffed name",
    ERR_HOST: "name left to the host",
    ERR_REGEX: "a regex entry cannot be matched on the device",   # not asked for, or outside the subset
    ERR_PATTERN: "pattern longer than 255 bytes",
}

(KIND_ALL, KIND_IP, KIND_CIDR, KIND_DOMAIN_EXACT, KIND_DOMAIN_WILDCARD, KIND_DOMAIN_SUFFIX, KIND_DOMAIN_SET,
 KIND_CIDR_SET) = range(8)
DOMAIN_PLAIN, DOMAIN_REGEX, DOMAIN_ROOT, DOMAIN_FULL = range(4)   # geositeDomainType
_DOMAIN_TYPES = {"plain": DOMAIN_PLAIN, "regex": DOMAIN_REGEX, "root": DOMAIN_ROOT, "full": DOMAIN_FULL}

# struct hyobfs_acl_result as a numpy record
ACL_RESULT_DTYPE = np.dtype([("status", "<i4"), ("rule", "<i4"), ("outbound", "<u4"), ("hijack", "<u4")])
assert ACL_RESULT_DTYPE.itemsize == 16


class HyobfsAclDomain(ctypes.Structure):
    """struct hyobfs_acl_domain."""
    _fields_ = [("type", ctypes.c_uint32), ("len", ctypes.c_uint32), ("value", ctypes.c_void_p)]


class HyobfsAclCidr(ctypes.Structure):
    """struct hyobfs_acl_cidr."""
    _fields_ = [("addr", ctypes.c_uint8 * 16), ("family", ctypes.c_uint8), ("prefix", ctypes.c_uint8),
                ("pad_", ctypes.c_uint8 * 2)]


class HyobfsAclRule(ctypes.Structure):
    """struct hyobfs_acl_rule."""
    _fields_ = [("kind", ctypes.c_uint32), ("proto", ctypes.c_uint32), ("start_port", ctypes.c_uint16),
                ("end_port", ctypes.c_uint16), ("outbound", ctypes.c_uint32), ("hijack", ctypes.c_uint32),
                ("pattern_len", ctypes.c_uint32), ("pattern", ctypes.c_void_p), ("addr", ctypes.c_uint8 * 16),
                ("family", ctypes.c_uint8), ("prefix", ctypes.c_uint8), ("inverse", ctypes.c_uint8),
                ("pad_", ctypes.c_uint8), ("n_entries", ctypes.c_uint32), ("entries", ctypes.c_void_p)]


class HyobfsAclOptions(ctypes.Structure):
    """struct hyobfs_acl_options."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("index_min", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32)]


class HyobfsAclIndexInfo(ctypes.Structure):
    """struct hyobfs_acl_index_info."""
    _fields_ = [("values", ctypes.c_uint32), ("slots", ctypes.c_uint32), ("max_probe", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32)]


IndexInfo = collections.namedtuple("IndexInfo", "values slots max_probe")


def _alib(lib=None):
    """The library with include/hyobfs_acl.h declared (_lib.load() has done it for
    every build that holds these entry points; one without them fails here)."""
    return _lib.declare(lib if lib is not None else _lib.load(), "acl", _lib._ACL_SIG)


# ------------------------------------------------------------------ device calls
class RuleRefused(ValueError):
    """hyobfs_acl_ruleset_new refused rule ``rule`` with ``status``; ``entry``: the
    DOMAIN_SET entry it was about, or -1."""

    def __init__(self, status: int, rule: int, entry: int = -1):
        self.status, self.rule, self.entry = status, rule, entry
        where = f"rule {rule}" + (f", entry {entry}" if entry >= 0 else "")
        super().__init__(f"{where}: {ERRORS.get(status, 'invalid rule')} ({status})")


def ruleset_new(c_rules, n_rules: int, device: int = 0, flags: int = 0, index_min=None):
    """hyobfs_acl_ruleset_new (``flags`` == 0) or hyobfs_acl_ruleset_new_flags over a
    HyobfsAclRule array: the handle.  With ``index_min`` given (0: the library's
    default), hyobfs_acl_ruleset_new_opts with these flags (FLAG_INDEX is valid
    there only) and that threshold.  A refused rule raises RuleRefused (before
    the device is looked at)."""
    lib = _alib()
    h = ctypes.c_void_p()
    if index_min is not None:
        opts = HyobfsAclOptions(ctypes.sizeof(HyobfsAclOptions), flags, index_min, 0)
        st = lib.hyobfs_acl_ruleset_new_opts(c_rules, n_rules, device, ctypes.byref(opts), ctypes.byref(h))
    elif flags:
        st = lib.hyobfs_acl_ruleset_new_flags(c_rules, n_rules, device, flags, ctypes.byref(h))
    else:
        st = lib.hyobfs_acl_ruleset_new(c_rules, n_rules, device, ctypes.byref(h))
    bad = int(lib.hyobfs_acl_ruleset_bad_rule())
    if st != _lib.HYOBFS_OK and bad >= 0:
        raise RuleRefused(st, bad, int(lib.hyobfs_acl_ruleset_bad_entry()))
    _lib.check(st, "acl_ruleset_new")
    assert lib.hyobfs_acl_ruleset_rules(h) == n_rules
    return h


def ruleset_free(handle) -> None:
    _alib().hyobfs_acl_ruleset_free(handle)


def ruleset_entries(handle) -> int:
    """hyobfs_acl_ruleset_entries: the entries of the table the kernel walks."""
    return int(_alib().hyobfs_acl_ruleset_entries(handle))


def ruleset_index_info(handle, rule: int) -> IndexInfo:
    """hyobfs_acl_ruleset_index_info: (values, slots, max_probe) of one rule's index;
    slots == 0 when the rule has none."""
    info = HyobfsAclIndexInfo()
    _lib.check(_alib().hyobfs_acl_ruleset_index_info(handle, rule, ctypes.byref(info)), "acl_ruleset_index_info")
    return IndexInfo(int(info.values), int(info.slots), int(info.max_probe))


def _pattern_bytes(p) -> bytes:
    return p.encode("utf-8", "surrogateescape") if isinstance(p, str) else bytes(p)


def regex_check(pattern):
    """hyobfs_acl_regex_check (host only): (status, DFA states, byte classes) of a
    geosite regex value; status 0 when the device takes it, else ERR_REGEX or
    ERR_PATTERN with zeros."""
    p = _pattern_bytes(pattern)
    states, classes = ctypes.c_uint32(0), ctypes.c_uint32(0)
    st = _alib().hyobfs_acl_regex_check(p, len(p), ctypes.byref(states), ctypes.byref(classes))
    return int(st), int(states.value), int(classes.value)


def regex_match(pattern, name) -> bool:
    """hyobfs_acl_regex_match (host only): the kernel's DFA walk of ``pattern`` over
    the bytes of ``name`` as given.  A refused pattern raises ValueError."""
    p, n = _pattern_bytes(pattern), _pattern_bytes(name)
    st = _alib().hyobfs_acl_regex_match(p, len(p), n, len(n))
    if st < 0:
        raise ValueError(f"regex {pattern!r}: {ERRORS.get(st, 'invalid')} ({st})")
    return bool(st)


def match_batch(handle, names, name_off, name_len, ipv4, ipv6, ip_flags, proto, port, n: int, res, stream=None) -> None:
    """hyobfs_acl_match_batch: name i is names[name_off[i], +name_len[i]); ``res``
    gets ACL_RESULT_DTYPE records.  Arguments are device tensors or pointers
    (``ipv4`` / ``ipv6`` / ``ip_flags`` may all be None: no addresses)."""
    st = _alib().hyobfs_acl_match_batch(handle, _ptr(names), _ptr(name_off), _ptr(name_len), _ptr(ipv4), _ptr(ipv6),
                                        _ptr(ip_flags), _ptr(proto), _ptr(port), n, _ptr(res), _stream(stream, res))
    _lib.check(st, "acl_match_batch")


def match_sniffed_batch(handle, names, name_stride: int, sres, ipv4, ipv6, ip_flags, proto, port, n: int, res,
                        stream=None) -> None:
    """hyobfs_acl_match_sniffed_batch: name i is names[i * name_stride,
    +sres[i].name_len), as the sniff calls leave ``names`` and ``sres``."""
    st = _alib().hyobfs_acl_match_sniffed_batch(handle, _ptr(names), name_stride, _ptr(sres), _ptr(ipv4), _ptr(ipv6),
                                                _ptr(ip_flags), _ptr(proto), _ptr(port), n, _ptr(res),
                                                _stream(stream, res))
    _lib.check(st, "acl_match_sniffed_batch")


# ------------------------------------------------------------------ parse.go
TextRule = collections.namedtuple("TextRule", "outbound address proto_port hijack_address line_num")

_LINE = re.compile(r"^(\w+)\s*\(([^,]+)(?:,([^,]+))?(?:,([^,]+))?\)\Z", re.ASCII)   # linePattern, parse.go:9


class InvalidSyntaxError(ValueError):
    def __init__(self, line: str, line_num: int):
        self.line, self.line_num = line, line_num
        super().__init__(f"invalid syntax at line {line_num}: {line}")


def parse_text_rules(text: str) -> list[TextRule]:
    """ParseTextRules (parse.go:50-72): '#' starts a comment, empty lines are
    skipped, line numbers count from 1."""
    rules = []
    for num, line in enumerate(text.split("\n"), 1):
        i = line.find("#")
        if i >= 0:
            line = line[:i]
        line = line.strip()
        if not line:
            continue
        m = _LINE.match(line)
        if m is None:
            raise InvalidSyntaxError(line, num)
        rules.append(TextRule(m.group(1), m.group(2).strip(), (m.group(3) or "").strip(), (m.group(4) or "").strip(),
                              num))
    return rules


# ------------------------------------------------------------------ compile.go
class CompilationError(ValueError):
    def __init__(self, line_num: int, message: str):
        self.line_num, self.message = line_num, message
        super().__init__(f"error at line {line_num}: {message}")


def _parse_uint16(s: str):
    """strconv.ParseUint(s, 10, 16): digits only; None on error."""
    if not re.fullmatch(r"[0-9]+", s) or int(s) > 0xFFFF:
        return None
    return int(s)


def parse_proto_port(proto_port: str):
    """parseProtoPort (compile.go:175-233): (proto, start_port, end_port), or None."""
    pp = proto_port.lower()
    if pp in ("", "*", "*/*"):
        return PROTO_BOTH, 0, 0
    parts = pp.split("/", 1)
    protos = {"tcp": PROTO_TCP, "udp": PROTO_UDP}
    if len(parts) == 1:
        return (protos[parts[0]], 0, 0) if parts[0] in protos else None
    protos["*"] = PROTO_BOTH
    if parts[0] not in protos:
        return None
    start = end = 0
    if parts[1] != "*":
        ports = parts[1].strip().split("-", 1)
        if len(ports) == 1:
            start = end = _parse_uint16(parts[1])   # the untrimmed text, as the reference parses it
            if start is None:
                return None
        else:
            start, end = _parse_uint16(ports[0]), _parse_uint16(ports[1])
            if start is None or end is None or start > end:
                return None
    return protos[parts[0]], start, end


def parse_ip(s: str):
    """net.ParseIP: the address bytes (4 for dotted IPv4, else 16), or None."""
    if "%" in s:
        return None
    try:
        return ipaddress.ip_address(s).packed
    except ValueError:
        return None


def parse_cidr(s: str):
    """net.ParseCIDR's IPNet: (masked address bytes, prefix), or None.  The address
    is 4 bytes for dotted IPv4 and 16 otherwise, as IPNet.IP is."""
    i = s.find("/")
    if i < 0:
        return None
    ip, mask = parse_ip(s[:i]), s[i + 1:]
    if ip is None or not re.fullmatch(r"[0-9]+", mask) or len(mask) > 6 or int(mask) > 8 * len(ip):
        return None
    bits, ones = 8 * len(ip), int(mask)
    m = ((1 << bits) - (1 << (bits - ones))).to_bytes(len(ip), "big")
    return bytes(a & b for a, b in zip(ip, m)), ones


def parse_geosite_name(s: str):
    """parseGeoSiteName (compile.go:318-326): (name, [attributes])."""
    parts = s.split("@")
    return parts[0].strip(), [a.strip() for a in parts[1:]]


class Rule:
    """compiledRule (compile.go:53-60) with its host matcher's fields."""
    __slots__ = ("kind", "proto", "start_port", "end_port", "outbound", "hijack", "pattern", "ip", "prefix",
                 "entries", "inverse", "line_num")

    def __init__(self, kind, pattern="", ip=b"", prefix=0, entries=(), inverse=False):
        self.kind, self.pattern, self.ip, self.prefix = kind, pattern, ip, prefix
        self.entries, self.inverse = list(entries), inverse
        self.proto = self.start_port = self.end_port = self.outbound = self.line_num = 0
        self.hijack = None


def compile_host_matcher(addr: str, geo=None, device_regex: bool = False) -> Rule:
    """compileHostMatcher (compile.go:235-316), its tests in the reference's
    order.  Raises ValueError with the reference's message.  ``device_regex``: a
    geosite regex entry is kept if the library takes its pattern."""
    addr = addr.lower().rstrip(".")
    if addr in ("*", "all"):
        return Rule(KIND_ALL)
    if addr.startswith("geoip:"):
        country = addr[6:]
        if not country:
            raise ValueError("empty GeoIP country code")
        if geo is None:
            raise ValueError("geoip rules need a geo loader")
        got = geo.geoip(country)
        if got is None:
            raise ValueError(f"GeoIP country code {country} not found")
        inverse = False
        if isinstance(got, tuple) and len(got) == 2 and isinstance(got[1], bool):
            got, inverse = got
        entries = []
        for ip, prefix in got:
            ip = bytes(ip)
            if len(ip) not in (4, 16):
                raise ValueError("invalid IP length")
            if not 0 <= prefix <= 8 * len(ip):
                raise ValueError("invalid prefix")
            entries.append((ip, int(prefix)))
        return Rule(KIND_CIDR_SET, entries=entries, inverse=inverse)
    if addr.startswith("geosite:"):
        name, attrs = parse_geosite_name(addr[8:])
        if not name:
            raise ValueError("empty GeoSite name")
        if geo is None:
            raise ValueError("geosite rules need a geo loader")
        got = geo.geosite(name)
        if got is None:
            raise ValueError(f"GeoSite name {name} not found")
        entries = []
        for typ, value, have in got:
            if typ not in _DOMAIN_TYPES:
                raise ValueError("unsupported domain type")
            # matchDomain's attribute test (matchers_v2geo.go:122-132): all of the rule's
            have = set(have or ())
            if attrs and not all(a in have for a in attrs):
                continue
            if typ == "regex":
                if not device_regex:
                    raise ValueError(f"GeoSite name {name}: regex entry {value!r} cannot be matched on the device")
                st = regex_check(value)[0]
                if st != _lib.HYOBFS_OK:
                    raise ValueError(f"GeoSite name {name}: regex entry {value!r}: "
                                     f"{ERRORS.get(st, 'invalid pattern')} ({st})")
            entries.append((typ, value))
        return Rule(KIND_DOMAIN_SET, entries=entries)
    if addr.startswith("suffix:"):
        if not addr[7:]:
            raise ValueError("empty domain suffix")
        return Rule(KIND_DOMAIN_SUFFIX, pattern=addr[7:])
    if "/" in addr:
        net = parse_cidr(addr)
        if net is None:
            raise ValueError(f"invalid CIDR address: {addr}")
        return Rule(KIND_CIDR, ip=net[0], prefix=net[1])
    ip = parse_ip(addr)
    if ip is not None:
        return Rule(KIND_IP, ip=ip)
    if "*" in addr:
        return Rule(KIND_DOMAIN_WILDCARD, pattern=addr)
    return Rule(KIND_DOMAIN_EXACT, pattern=addr)


def compile_rules(text_rules, outbounds: dict, geo=None, device_regex: bool = False, device_index: bool = False,
                  index_min: int = 0) -> "RuleSet":
    """Compile (compile.go:130-161).  ``outbounds`` maps lower-case names to
    integers; ``geo`` (optional) has ``geoip(code)`` returning a list of (address
    bytes, prefix) -- or (that list, inverse) -- and ``geosite(name)`` returning a
    list of (type, value, attributes) with type "plain", "regex", "root" or
    "full"; both return None for an unknown name.  A regex entry that passes the
    rule's attribute filter is a CompilationError, unless ``device_regex`` is set:
    then it is kept and matched on the device, and only a pattern that
    ``regex_check`` refuses is a CompilationError, with the library's status.
    ``device_index``: the device looks the full and root values of a geosite list
    with at least ``index_min`` of them (0: the library's default, 65) up in a hash
    table instead of walking them; no result changes."""
    rules = []
    for tr in text_rules:
        if tr.outbound.lower() not in outbounds:
            raise CompilationError(tr.line_num, f"outbound {tr.outbound} not found")
        try:
            rule = compile_host_matcher(tr.address, geo, device_regex)
        except ValueError as e:
            raise CompilationError(tr.line_num, str(e)) from None
        for what, p in (("pattern", rule.pattern), *(("value", e[1]) for e in rule.entries
                                                       if rule.kind == KIND_DOMAIN_SET)):
            if len(p.encode("utf-8", "surrogateescape") if isinstance(p, str) else p) > MAX_NAME:
                raise CompilationError(tr.line_num, f"{what} longer than {MAX_NAME} bytes")
        pp = parse_proto_port(tr.proto_port)
        if pp is None:
            raise CompilationError(tr.line_num, f"invalid protocol/port: {tr.proto_port}")
        rule.proto, rule.start_port, rule.end_port = pp
        if tr.hijack_address:
            ip = parse_ip(tr.hijack_address)
            if ip is None:
                raise CompilationError(tr.line_num,
                                       f"invalid hijack address (must be an IP address): {tr.hijack_address}")
            rule.hijack = str(ipaddress.ip_address(ip))
        rule.outbound = int(outbounds[tr.outbound.lower()])
        rule.line_num = tr.line_num
        rules.append(rule)
    return RuleSet(rules, device_index, index_min)


# ------------------------------------------------------------------ the host matcher (names the device leaves)
_V4_IN_V6 = bytes(10) + b"\xff\xff"


def _to4(ip):
    if ip is not None and len(ip) == 16 and ip[:12] == _V4_IN_V6:
        return ip[12:]
    return ip if ip is not None and len(ip) == 4 else None


def _to16(ip):
    return _V4_IN_V6 + ip if len(ip) == 4 else ip


def _contains(net_ip, prefix, ip):
    """IPNet.Contains for a mask of ``prefix`` ones as long as ``net_ip``."""
    if ip is None:
        return False
    nn, bits = _to4(net_ip), prefix
    if nn is None:
        nn = net_ip
    elif len(net_ip) == 16:
        bits = max(prefix - 96, 0)   # the last four bytes of the 16-byte mask
    x = _to4(ip)
    x = ip if x is None else x
    if len(x) != len(nn):
        return False
    shift = 8 * len(nn) - bits
    return int.from_bytes(nn, "big") >> shift == int.from_bytes(x, "big") >> shift


def _to_unicode(name: str) -> str:
    """idna.ToUnicode as the reference uses it: "xn--" labels decoded, the name
    unchanged on any error."""
    if "xn--" not in name:
        return name
    try:
        return ".".join(lab[4:].encode("ascii").decode("punycode") if lab.startswith("xn--") else lab
                        for lab in name.split("."))
    except (UnicodeError, ValueError):
        return name


def _wildcard(name: str, pattern: str) -> bool:
    """deepMatchRune (matchers.go:58-73), the kernel's iterative form over characters."""
    s = q = mark = 0
    star = -1
    while s < len(name):
        pc = pattern[q] if q < len(pattern) else None
        if pc == "*":
            star, mark = q, s
            q += 1
        elif pc == name[s]:
            s += 1
            q += 1
        elif star >= 0:
            mark += 1
            s, q = mark, star + 1
        else:
            return False
    return all(c == "*" for c in pattern[q:])


_GO_SPACE = frozenset(b"\t\n\f\r ")   # Go's \s: no \v (Python's has it)
_PERL = {"d": frozenset(range(0x30, 0x3A)), "s": _GO_SPACE,
         "w": frozenset(b"0123456789_abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ")}


def _py_class(ascii_set, beyond: bool) -> str:
    """A character class of exactly these ASCII code points, and every code point
    beyond ASCII if ``beyond``."""
    inside = sorted(set(range(128)) - ascii_set) if beyond else sorted(ascii_set)
    if not inside:
        return "[\\x00-\\U0010ffff]" if beyond else "(?!)"
    return "[%s%s]" % ("^" if beyond else "", "".join("\\x%02x" % c for c in inside))


def _regex_to_py(pattern: str) -> str:
    """A geosite regex (Go syntax, the header's subset) as a Python pattern for
    ``re.ASCII`` with Go's meaning: ``^`` -> ``\\A``, ``$`` -> ``\\Z`` (Python's ``$`` also
    matches before a trailing newline), ``\\s`` / ``\\S`` and every class spelled out
    (Go's ``\\s`` has no ``\\v``)."""
    out, i, n = [], 0, len(pattern)
    while i < n:
        c = pattern[i]
        i += 1
        if c == "\\" and i < n:
            e = pattern[i]
            i += 1
            if e in "sS":
                out.append(_py_class(set(_GO_SPACE), False) if e == "s" else _py_class(set(range(128)) - _GO_SPACE, True))
            else:
                out.append("\\" + e)
        elif c == "^":
            out.append("\\A")
        elif c == "$":
            out.append("\\Z")
        elif c == "[":
            neg = i < n and pattern[i] == "^"
            i += neg
            members, beyond = set(), False

            def member():
                """One class member at i: (ASCII set, reaches beyond ASCII, is a single byte)."""
                nonlocal i
                ch = pattern[i]
                i += 1
                if ch != "\\":
                    return {ord(ch)}, False, True
                e = pattern[i]
                i += 1
                if e.lower() in _PERL and e.isalpha():
                    s = set(_PERL[e.lower()])
                    return (s, False, False) if e.islower() else (set(range(128)) - s, True, False)
                return {ord(e)}, False, True
            while i < n and pattern[i] != "]":
                s, b, single = member()
                if single and i + 1 < n and pattern[i] == "-" and pattern[i + 1] != "]":
                    i += 1
                    hi = member()[0]
                    s = set(range(min(s), max(hi) + 1))
                members |= s
                beyond |= b
            i += 1   # the ']'
            if neg:
                members, beyond = set(range(128)) - members, not beyond
            out.append(_py_class(members, beyond))
        else:
            out.append(c)
    return "".join(out)


def _as_ip(x, size):
    """None, bytes of ``size``, an ipaddress object or its text -> bytes or None."""
    if x is None:
        return None
    if isinstance(x, str):
        x = ipaddress.ip_address(x)
    if not isinstance(x, (bytes, bytearray)):
        x = x.packed
    x = bytes(x)
    if len(x) == 4 and size == 16:
        x = _V4_IN_V6 + x
    if len(x) != size:
        raise ValueError(f"an address of {size} bytes is needed, got {len(x)}")
    return x


# ------------------------------------------------------------------ the rule set
class RuleSet:
    """A compiled rule set.  The device copy (hyobfs_acl_ruleset) is made on first
    use per device and freed by close() / the garbage collector.  ``device_index``:
    it is made by hyobfs_acl_ruleset_new_opts with HYOBFS_ACL_FLAG_INDEX and
    ``index_min`` (the header's "THE INDEX"; matching gives the same results)."""

    def __init__(self, rules, device_index: bool = False, index_min: int = 0):
        if index_min and not device_index:
            raise ValueError("index_min needs device_index")
        self.device_index, self.index_min = bool(device_index), int(index_min)
        self.rules = list(rules)
        self.hijacks = sorted({r.hijack for r in self.rules if r.hijack is not None})
        self._sets = {}
        self._regexes = {}   # pattern -> compiled, for match_host

    def __len__(self):
        return len(self.rules)

    # -- host side
    def _rule_matches_host(self, r: Rule, name: str, v4, v6) -> bool:
        if r.kind == KIND_ALL:
            return True
        if r.kind == KIND_IP:
            x = _to16(r.ip)
            return (v4 is not None and _to16(v4) == x) or (v6 is not None and _to16(v6) == x)
        if r.kind == KIND_CIDR:
            return _contains(r.ip, r.prefix, v4) or _contains(r.ip, r.prefix, v6)
        if r.kind in (KIND_DOMAIN_EXACT, KIND_DOMAIN_WILDCARD, KIND_DOMAIN_SUFFIX):
            uni = _to_unicode(name)
            if r.kind == KIND_DOMAIN_EXACT:
                return uni == r.pattern
            if r.kind == KIND_DOMAIN_WILDCARD:
                return _wildcard(uni, r.pattern)
            return uni == r.pattern or uni.endswith("." + r.pattern)
        if r.kind == KIND_DOMAIN_SET:
            for typ, value in r.entries:
                if (typ == "plain" and value in name) or (typ == "full" and name == value) or \
                        (typ == "root" and (name == value or name.endswith("." + value))) or \
                        (typ == "regex" and self._regex(value).search(name) is not None):
                    return True
            return False
        # KIND_CIDR_SET: geoipMatcher.Match with the reference's binary search
        n4 = sorted((e for e in r.entries if len(e[0]) == 4), key=lambda e: (e[0], e[1]))
        n6 = sorted((e for e in r.entries if len(e[0]) == 16), key=lambda e: (e[0], e[1]))
        for ip in (v4, v6):
            if ip is None:
                continue
            x = _to4(ip)
            lst, x = (n4, x) if x is not None else (n6, ip)
            left, right = 0, len(lst) - 1
            while left <= right:
                mid = (left + right) // 2
                if _contains(lst[mid][0], lst[mid][1], x):
                    return not r.inverse
                if lst[mid][0] < x:
                    left = mid + 1
                else:
                    right = mid - 1
        return bool(r.inverse)

    def _regex(self, value: str):
        if value not in self._regexes:
            self._regexes[value] = re.compile(_regex_to_py(value), re.ASCII)
        return self._regexes[value]

    def match_host(self, name, ipv4=None, ipv6=None, proto: int = 0, port: int = 0) -> int:
        """compiledRuleSetImpl.Match (compile.go:88-109) on the CPU: the index of the
        first matching rule, or -1.  For the names the device leaves to the host."""
        if isinstance(name, (bytes, bytearray)):
            name = bytes(name).decode("utf-8", "replace")
        name = name.lower().rstrip(".")
        v4, v6 = _as_ip(ipv4, 4), _as_ip(ipv6, 16)
        for i, r in enumerate(self.rules):
            if r.proto != PROTO_BOTH and r.proto != proto:
                continue
            if r.start_port != 0 and (port < r.start_port or port > r.end_port):
                continue
            if self._rule_matches_host(r, name, v4, v6):
                return i
        return -1

    def decision(self, rule: int):
        """(outbound, hijack address or None) of a rule index; (0, None) for -1:
        the reference's zero outbound, "use the default"."""
        if rule < 0:
            return 0, None
        return self.rules[rule].outbound, self.rules[rule].hijack

    # -- device side
    def c_rules(self):
        """(hyobfs_acl_rule array, the buffers it points into).  A regex entry is handed
        over as it is: hyobfs_acl_ruleset_new_flags with ``flags()`` takes it."""
        keep = []

        def buf(b):
            b = b.encode("utf-8", "surrogateescape") if isinstance(b, str) else bytes(b)
            keep.append(ctypes.create_string_buffer(b, len(b) + 1))
            return ctypes.cast(keep[-1], ctypes.c_void_p), len(b)

        arr = (HyobfsAclRule * max(len(self.rules), 1))()
        for c, r in zip(arr, self.rules):
            c.kind, c.proto, c.start_port, c.end_port, c.outbound = r.kind, r.proto, r.start_port, r.end_port, r.outbound
            c.hijack = NO_HIJACK if r.hijack is None else self.hijacks.index(r.hijack)
            if r.kind in (KIND_DOMAIN_EXACT, KIND_DOMAIN_WILDCARD, KIND_DOMAIN_SUFFIX):
                c.pattern, c.pattern_len = buf(r.pattern)
            elif r.kind in (KIND_IP, KIND_CIDR):
                c.addr[:len(r.ip)] = r.ip
                c.family, c.prefix = (4 if len(r.ip) == 4 else 6), r.prefix
            elif r.kind == KIND_DOMAIN_SET:
                ents = (HyobfsAclDomain * max(len(r.entries), 1))()
                for e, (typ, value) in zip(ents, r.entries):
                    e.type = _DOMAIN_TYPES[typ]
                    e.value, e.len = buf(value)
                keep.append(ents)
                c.entries, c.n_entries = ctypes.cast(ents, ctypes.c_void_p), len(r.entries)
            elif r.kind == KIND_CIDR_SET:
                ents = (HyobfsAclCidr * max(len(r.entries), 1))()
                for e, (ip, prefix) in zip(ents, r.entries):
                    e.addr[:len(ip)] = ip
                    e.family, e.prefix = (4 if len(ip) == 4 else 6), prefix
                keep.append(ents)
                c.entries, c.n_entries, c.inverse = ctypes.cast(ents, ctypes.c_void_p), len(r.entries), int(r.inverse)
        return arr, keep

    def flags(self) -> int:
        """HYOBFS_ACL_FLAG_REGEX if a rule holds a regex entry, and HYOBFS_ACL_FLAG_INDEX
        if the set was made with ``device_index``."""
        regex = any(r.kind == KIND_DOMAIN_SET and any(e[0] == "regex" for e in r.entries) for r in self.rules)
        return (FLAG_REGEX if regex else 0) | (FLAG_INDEX if self.device_index else 0)

    def device_set(self, device: int = 0):
        """The hyobfs_acl_ruleset handle on cuda:<device> (made once); regex entries
        go over with HYOBFS_ACL_FLAG_REGEX, and a set made with ``device_index``
        through hyobfs_acl_ruleset_new_opts."""
        if device not in self._sets:
            arr, keep = self.c_rules()
            try:
                self._sets[device] = ruleset_new(arr, len(self.rules), device, self.flags(),
                                                 self.index_min if self.device_index else None)
            except RuleRefused as e:
                line = self.rules[e.rule].line_num if 0 <= e.rule < len(self.rules) else 0
                raise CompilationError(line, str(e)) from None
        return self._sets[device]

    def close(self):
        sets, self._sets = self._sets, {}
        for h in sets.values():
            ruleset_free(h)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:   # interpreter shutdown
            pass

    @staticmethod
    def _device_of(device, *tensors):
        if device is not None:
            return device
        for t in tensors:
            if getattr(t, "is_cuda", False):
                return t.device.index or 0
        return 0

    def match_batch(self, names, name_off, name_len, ipv4, ipv6, ip_flags, proto, port, n: int, res, stream=None,
                    device=None) -> None:
        """hyobfs_acl_match_batch: name i is names[name_off[i], +name_len[i]); ``res``
        gets ACL_RESULT_DTYPE records.  Arguments are device tensors or pointers
        (``ipv4`` / ``ipv6`` / ``ip_flags`` may be None: no addresses)."""
        match_batch(self.device_set(self._device_of(device, res, names)), names, name_off, name_len, ipv4, ipv6,
                    ip_flags, proto, port, n, res, stream)

    def match_sniffed_batch(self, names, name_stride: int, sres, ipv4, ipv6, ip_flags, proto, port, n: int, res,
                            stream=None, device=None) -> None:
        """hyobfs_acl_match_sniffed_batch: name i is names[i * name_stride,
        +sres[i].name_len), as the sniff calls leave ``names`` and ``sres``."""
        match_sniffed_batch(self.device_set(self._device_of(device, res, names)), names, name_stride, sres, ipv4,
                            ipv6, ip_flags, proto, port, n, res, stream)

    @staticmethod
    def _address_arrays(hosts):
        n = len(hosts)
        v4, v6, fl = np.zeros((n, 4), np.uint8), np.zeros((n, 16), np.uint8), np.zeros(n, np.uint8)
        for i, (_, a, b) in enumerate(hosts):
            a, b = _as_ip(a, 4), _as_ip(b, 16)
            if a is not None:
                v4[i], fl[i] = np.frombuffer(a, np.uint8), 1
            if b is not None:
                v6[i] = np.frombuffer(b, np.uint8)
                fl[i] |= 2
        return v4.reshape(-1), v6.reshape(-1), fl

    def match_many(self, hosts, protos, ports, device: int = 0):
        """Match for a list of hosts (name, ipv4, ipv6) -- a name is str or bytes, an
        address None, bytes, text or an ipaddress object -- with one protocol and
        port each: [(outbound, hijack address or None)], (0, None) where no rule
        matches.  Runs on cuda:<device>; the names the device leaves to the host
        are finished by match_host."""
        import torch
        n = len(hosts)
        if not (n == len(protos) == len(ports)):
            raise ValueError("one protocol and one port per host")
        if n == 0:
            return []
        dev = torch.device("cuda", device)
        names = [h[0].encode("utf-8", "surrogateescape") if isinstance(h[0], str) else bytes(h[0]) for h in hosts]
        buf, off, lens = _pack(names)
        v4, v6, fl = self._address_arrays(hosts)
        d_res = torch.zeros(n * ACL_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        self.match_batch(_to(dev, buf), _to(dev, off), _to(dev, lens), _to(dev, v4), _to(dev, v6), _to(dev, fl),
                         _to(dev, np.asarray(protos, np.uint8)), _to(dev, np.asarray(ports, np.uint16).view(np.int16)),
                         n, d_res, device=device)
        out = []
        for i, r in enumerate(_records(d_res, ACL_RESULT_DTYPE)):
            if r["status"] == ERR_HOST:
                out.append(self.decision(self.match_host(names[i], hosts[i][1], hosts[i][2], int(protos[i]),
                                                         int(ports[i]))))
            else:
                _lib.check(int(r["status"]), "acl_match_batch item")
                out.append(self.decision(int(r["rule"])))
        return out


def quic_sniff_and_match(rules: RuleSet, datagrams, ports, hosts=None, device: int = 0, crypto_cap: int = 4096,
                         name_stride: int = MAX_NAME):
    """The fused path, worked: ``quic_sniff_batch`` and ``match_sniffed_batch`` on one
    stream over a list of QUIC client Initials; the names never leave the device.
    ``ports``: the request's port per datagram (the protocol is UDP); ``hosts``
    (optional): (ipv4, ipv6) of the request address per datagram.  Returns per
    datagram (outbound, hijack address or None), or None where the sniffer found
    no name: that request keeps its own address, which the caller matches itself
    (``match_many``).  Only the names the device leaves to the host are copied
    back, and finished by ``match_host``."""
    import torch
    n = len(datagrams)
    if n != len(ports) or (hosts is not None and n != len(hosts)):
        raise ValueError("one port (and one address pair) per datagram")
    if n == 0:
        return []
    dev = torch.device("cuda", device)
    hosts = [(None, None)] * n if hosts is None else hosts
    buf, off, lens = _pack(datagrams)
    v4, v6, fl = RuleSet._address_arrays([(None, a, b) for a, b in hosts])
    d_crypto = torch.zeros(n * crypto_cap, dtype=torch.uint8, device=dev)
    d_qres = torch.zeros(n * quic.RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    d_names = torch.zeros(n * name_stride, dtype=torch.uint8, device=dev)
    d_sres = torch.zeros(n * sniff.SNIFF_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    d_res = torch.zeros(n * ACL_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    ws = torch.empty(max(sniff.quic_sniff_workspace_size(n), 1), dtype=torch.uint8, device=dev)
    args = [_to(dev, x) for x in (buf, off, lens, np.arange(n, dtype=np.uint64) * np.uint64(crypto_cap),
                                  np.full(n, crypto_cap, np.uint32), v4, v6, fl, np.full(n, PROTO_UDP, np.uint8),
                                  np.asarray(ports, np.uint16).view(np.int16))]
    stream = torch.cuda.current_stream(dev)
    sniff.quic_sniff_batch(args[0], args[1], args[2], n, d_crypto, args[3], args[4], d_qres, d_names, name_stride,
                           d_sres, ws, stream=stream)
    rules.match_sniffed_batch(d_names, name_stride, d_sres, args[5], args[6], args[7], args[8], args[9], n, d_res,
                              stream=stream, device=device)
    out = []
    res = _records(d_res, ACL_RESULT_DTYPE)
    left = [i for i in range(n) if res[i]["status"] == ERR_HOST]
    if left:
        sres = _records(d_sres, sniff.SNIFF_RESULT_DTYPE)
        rows = d_names.view(n, name_stride)[torch.tensor(left, device=dev)].cpu().numpy()
        left = {i: rows[k, :int(sres[i]["name_len"])].tobytes() for k, i in enumerate(left)}
    for i, r in enumerate(res):
        if r["status"] == ERR_NO_NAME:
            out.append(None)
        elif r["status"] == ERR_HOST:
            out.append(rules.decision(rules.match_host(left[i], hosts[i][0], hosts[i][1], PROTO_UDP, int(ports[i]))))
        else:
            _lib.check(int(r["status"]), "acl_match_sniffed_batch item")
            out.append(rules.decision(int(r["rule"])))
    return out
