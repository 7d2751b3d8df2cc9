"""An independent Python restatement of the reference ACL's Match and of every
host matcher (apernet/hysteria extras/outbounds/acl), written from the Go.

TEST INFRASTRUCTURE ONLY: the product's kernel (hysteria_amd/csrc/acl.hip) and
its host matcher (hysteria_amd/acl.py) are compared with this file, and this
file is pinned to the reference's own test tables (tests/golden/acl_vectors.json).

A rule set is a list of dicts as tests/acl_cases.py writes them:
  {"kind": "all" | "ip" | "cidr" | "exact" | "wildcard" | "suffix" | "domain_set" | "cidr_set",
   "proto": 0 | 1 | 2, "start_port": int, "end_port": int, "outbound": int, "hijack": int,
   "pattern": bytes,                      exact / wildcard / suffix
   "ip": bytes (4 or 16),                 ip: the net.IP;  cidr: IPNet.IP
   "prefix": int,                         cidr: ones of a mask as long as "ip"
   "entries": [(type, value bytes)],      domain_set: type "plain" | "root" | "full"
   "entries": [(ip bytes, prefix)], "inverse": bool   cidr_set}
A host is (name bytes, ipv4 bytes | None, ipv6 bytes | None).

net.IP / net.IPNet are restated as Go's standard library defines them (To4,
Equal, networkNumberAndMask, Contains, CIDRMask); idna.ToUnicode is restated
with Python's punycode codec over the labels that begin with "xn--".
"""
import functools

NO_NAME, HOST = -61, -62   # include/hyobfs_acl.h
NO_HIJACK = 0xFFFFFFFF
MAX_NAME = 255

V4_IN_V6 = bytes(10) + b"\xff\xff"


# ------------------------------------------------------------------ Go's net.IP
def to4(ip):
    """net.IP.To4: the 4-byte form of a 4-byte or v4-mapped 16-byte address, else None."""
    if ip is None:
        return None
    if len(ip) == 4:
        return ip
    if len(ip) == 16 and ip[:12] == V4_IN_V6:
        return ip[12:]
    return None


def ip_equal(ip, x):
    """net.IP.Equal: an IPv4 address and its v4-mapped form are equal."""
    ip, x = ip or b"", x or b""
    if len(ip) == len(x):
        return ip == x and len(ip) in (4, 16)
    if len(ip) == 4 and len(x) == 16:
        return x[:12] == V4_IN_V6 and ip == x[12:]
    if len(ip) == 16 and len(x) == 4:
        return ip[:12] == V4_IN_V6 and ip[12:] == x
    return False


def cidr_mask(ones, bits):
    """net.CIDRMask."""
    if bits not in (32, 128) or ones < 0 or ones > bits:
        return None
    n = (1 << bits) - (1 << (bits - ones))
    return n.to_bytes(bits // 8, "big")


def network_number_and_mask(ip, mask):
    """net.networkNumberAndMask: the network address reduced with To4; of a
    16-byte mask over a 4-byte address only the last four bytes count."""
    r = to4(ip)
    if r is None:
        r = ip
        if len(r) != 16:
            return None, None
    if mask is None:
        return None, None
    if len(mask) == 4:
        if len(r) != 4:
            return None, None
    elif len(mask) == 16:
        if len(r) == 4:
            mask = mask[12:]
    else:
        return None, None
    return r, mask


def ipnet_contains(net_ip, mask, ip):
    """net.IPNet.Contains."""
    nn, m = network_number_and_mask(net_ip, mask)
    x = to4(ip)
    if x is not None:
        ip = x
    ip = ip or b""
    if nn is None or len(ip) != len(nn):
        return False
    return all(nn[i] & m[i] == ip[i] & m[i] for i in range(len(ip)))


# ------------------------------------------------------------------ matchers.go
def ip_matcher(rule, host):
    """ipMatcher.Match (matchers.go:24-26)."""
    return ip_equal(rule["ip"], host[1]) or ip_equal(rule["ip"], host[2])


def cidr_matcher(rule, host):
    """cidrMatcher.Match (matchers.go:32-34)."""
    mask = cidr_mask(rule["prefix"], 8 * len(rule["ip"]))
    return ipnet_contains(rule["ip"], mask, host[1]) or ipnet_contains(rule["ip"], mask, host[2])


def to_unicode(name: str) -> str:
    """idna.ToUnicode as domainMatcher.Match uses it (matchers.go:42-45): labels that
    begin with "xn--" are decoded; on any error the name stays as it was."""
    try:
        labels = name.split(".")
        for i, lab in enumerate(labels):
            if lab.startswith("xn--"):
                labels[i] = lab[4:].encode("ascii").decode("punycode")
        return ".".join(labels)
    except (UnicodeError, ValueError):
        return name


def deep_match_rune(s, pattern):
    """deepMatchRune (matchers.go:58-73), recursive as written there, over
    sequences of runes; memoised on the two remaining lengths."""
    @functools.lru_cache(maxsize=None)
    def go(i, j):
        while j < len(pattern):
            if pattern[j] == "*":
                return go(i, j + 1) or (i < len(s) and go(i + 1, j))
            if i >= len(s) or s[i] != pattern[j]:
                return False
            i += 1
            j += 1
        return i == len(s) and j == len(pattern)
    import sys
    old = sys.getrecursionlimit()
    sys.setrecursionlimit(max(old, 4 * (len(s) + len(pattern)) + 1000))
    try:
        return go(0, 0)
    finally:
        sys.setrecursionlimit(old)


def _text(b):
    return b.decode("utf-8", "replace") if isinstance(b, (bytes, bytearray)) else b


def domain_matcher(rule, host):
    """domainMatcher.Match (matchers.go:41-56)."""
    name = to_unicode(_text(host[0]))
    pattern = _text(rule["pattern"])
    if rule["kind"] == "exact":
        return name == pattern
    if rule["kind"] == "wildcard":
        return deep_match_rune(name, pattern)
    return name == pattern or name.endswith("." + pattern)


# ------------------------------------------------------------------ matchers_v2geo.go
def geoip_match_ip(n4, n6, ip):
    """geoipMatcher.matchIP (matchers_v2geo.go:24-46): n4 / n6 are sorted lists of
    (ip bytes as given, prefix)."""
    ip4 = to4(ip)
    if ip4 is not None:
        ip, n = ip4, n4
    else:
        n = n6
    left, right = 0, len(n) - 1
    while left <= right:
        mid = (left + right) // 2
        e_ip, e_prefix = n[mid]
        if ipnet_contains(e_ip, cidr_mask(e_prefix, 8 * len(e_ip)), ip):
            return True
        elif e_ip < ip:   # bytes.Compare(n[mid].IP, ip) < 0
            left = mid + 1
        else:
            right = mid - 1
    return False


def geoip_lists(entries):
    """newGeoIPMatcher (matchers_v2geo.go:62-94) with the ABI's stated sort:
    stable by address bytes, the shorter prefix first among equal addresses."""
    n4 = sorted((e for e in entries if len(e[0]) == 4), key=lambda e: (e[0], e[1]))
    n6 = sorted((e for e in entries if len(e[0]) == 16), key=lambda e: (e[0], e[1]))
    return n4, n6


def geoip_matcher(rule, host):
    """geoipMatcher.Match (matchers_v2geo.go:48-60)."""
    n4, n6 = geoip_lists(rule["entries"])
    if host[1] is not None and geoip_match_ip(n4, n6, host[1]):
        return not rule["inverse"]
    if host[2] is not None and geoip_match_ip(n4, n6, host[2]):
        return not rule["inverse"]
    return bool(rule["inverse"])


def geosite_matcher(rule, host):
    """geositeMatcher.Match / matchDomain (matchers_v2geo.go:121-161), after the
    attribute filter; on the name as it is (no ToUnicode)."""
    name = host[0]
    for typ, value in rule["entries"]:
        if typ == "plain" and value in name:
            return True
        if typ == "full" and name == value:
            return True
        if typ == "root" and (name == value or name.endswith(b"." + value)):
            return True
    return False


MATCHERS = {"all": lambda rule, host: True, "ip": ip_matcher, "cidr": cidr_matcher, "exact": domain_matcher,
            "wildcard": domain_matcher, "suffix": domain_matcher, "domain_set": geosite_matcher,
            "cidr_set": geoip_matcher}


# ------------------------------------------------------------------ compile.go
def normalise(name: bytes) -> bytes:
    """strings.TrimRight(strings.ToLower(name), ".") (compile.go:89) for the bytes
    the device lower-cases (ASCII); other bytes are the host's (see expected())."""
    return name.lower().rstrip(b".")


def rule_match(rule, host, proto, port):
    """compiledRule.Match (compile.go:62-70)."""
    if rule["proto"] != 0 and rule["proto"] != proto:
        return False
    if rule["start_port"] != 0 and (port < rule["start_port"] or port > rule["end_port"]):
        return False
    return MATCHERS[rule["kind"]](rule, host)


def match(rules, host, proto, port):
    """compiledRuleSetImpl.Match (compile.go:88-109) without the cache: the index
    of the first matching rule, or -1."""
    host = (normalise(host[0]), host[1], host[2])
    for i, rule in enumerate(rules):
        if rule_match(rule, host, proto, port):
            return i
    return -1


def left_to_host(name: bytes) -> bool:
    """The names the device leaves to the host (include/hyobfs_acl.h)."""
    return len(name) > MAX_NAME or any(b >= 0x80 for b in name) or b"xn--" in name.lower()


def expected(rules, item, sniff_status=None):
    """(status, rule, outbound, hijack) the device must report for one item
    (name, ipv4, ipv6, proto, port).  ``sniff_status``: the item goes through
    match_sniffed_batch with this hyobfs_sniff_result.status."""
    name, v4, v6, proto, port = item
    if sniff_status is not None and (sniff_status != 0 or len(name) == 0):
        return (NO_NAME, -1, 0, NO_HIJACK)
    if left_to_host(name):
        return (HOST, -1, 0, NO_HIJACK)
    r = match(rules, (name, v4, v6), proto, port)
    if r < 0:
        return (0, -1, 0, NO_HIJACK)
    return (0, r, rules[r]["outbound"], rules[r]["hijack"])
