"""Restatement of include/hyobfs_addr.h's rules H, P, I, T and F in Python, written
from the rules' text (and so from what Go's net.SplitHostPort, strconv.ParseUint,
net.ParseIP and IP.String do), not from hysteria_amd/csrc/addr_rules.h: it splits
texts into fields where the library walks bytes.  TEST INFRASTRUCTURE ONLY.

All texts are bytes."""
OK = 0
(NO_ADDR, MISSING_PORT, TOO_MANY_COLONS, MISSING_BRACKET, UNEXPECTED_LBRACKET, UNEXPECTED_RBRACKET, PORT, TOO_LONG,
 FAMILY) = range(-77, -86, -1)
MAX_ADDR, LITERAL_MAX, FORMAT_MAX = 2048, 45, 47
HAS_IPV4, HAS_IPV6 = 1, 2
V4_IN_V6 = bytes(10) + b"\xff\xff"


def split(text: bytes):
    """Rule H (and the limit): (status, host_off, host_len, port_off, port_len)."""
    fail = lambda st: (st, 0, 0, 0, 0)   # noqa: E731
    if len(text) > MAX_ADDR:
        return fail(TOO_LONG)
    i = text.rfind(b":")
    if i < 0:
        return fail(MISSING_PORT)
    j = k = 0
    if text[:1] == b"[":
        end = text.find(b"]")
        if end < 0:
            return fail(MISSING_BRACKET)
        if end + 1 == len(text):
            return fail(MISSING_PORT)
        if end + 1 != i:
            return fail(TOO_MANY_COLONS if text[end + 1:end + 2] == b":" else MISSING_PORT)
        host = (1, end - 1)
        j, k = 1, end + 1
    else:
        host = (0, i)
        if b":" in text[:i]:
            return fail(TOO_MANY_COLONS)
    if b"[" in text[j:]:
        return fail(UNEXPECTED_LBRACKET)
    if b"]" in text[k:]:
        return fail(UNEXPECTED_RBRACKET)
    return (OK, host[0], host[1], i + 1, len(text) - i - 1)


def _digits(b: bytes) -> bool:
    return len(b) > 0 and all(0x30 <= c <= 0x39 for c in b)


def parse_port(port: bytes):
    """Rule P: the value, or None."""
    if not _digits(port):
        return None
    v = int(port)   # Python integers do not wrap
    return v if v <= 65535 else None


def _v4_fields(s: bytes):
    f = s.split(b".")
    if len(f) != 4:
        return None
    for x in f:
        if not _digits(x) or (len(x) > 1 and x[0] == 0x30) or int(x) > 255:
            return None
    return bytes(int(x) for x in f)


def _hex_group(g: bytes):
    if not 1 <= len(g) <= 4 or any(c not in b"0123456789abcdefABCDEF" for c in g):
        return None
    return int(g, 16).to_bytes(2, "big")


def parse_ip(s: bytes):
    """Rule I: the 16-byte form, or None."""
    if len(s) > LITERAL_MAX:
        return None
    seps = [p for p in (s.find(b"."), s.find(b":"), s.find(b"%")) if p >= 0]
    if not seps or b"%" in s:
        return None
    if min(seps) == s.find(b"."):
        v4 = _v4_fields(s)
        return None if v4 is None else V4_IN_V6 + v4
    sides = s.split(b"::")
    if len(sides) > 2:
        return None
    fields = [side.split(b":") if side else [] for side in sides]
    flat = [g for side in fields for g in side]
    packed, at = [], 0
    for side in fields:
        out = b""
        for g in side:
            at += 1
            if b"." in g:
                if at != len(flat) or not s.endswith(g):
                    return None   # an embedded IPv4 runs to the end of the text
                x = _v4_fields(g)
            else:
                x = _hex_group(g)
            if x is None:
                return None
            out += x
        packed.append(out)
    total = sum(len(p) for p in packed)
    if len(sides) == 1:
        return packed[0] if total == 16 else None
    if total > 14:
        return None   # the "::" stands for at least one zero group
    return packed[0] + bytes(16 - total) + packed[1]


def to4(ip16: bytes):
    return ip16[12:] if ip16[:12] == V4_IN_V6 else None


def parse(text: bytes):
    """Rules H, P and T: (status, name_off, name_len, ipv4, ipv6, ip_flags, port), zeros
    beside a status that is not OK."""
    zero = (0, 0, bytes(4), bytes(16), 0, 0)
    st, ho, hl, po, pl = split(text)
    if st != OK:
        return (st,) + zero
    port = parse_port(text[po:po + pl])
    if port is None:
        return (PORT,) + zero
    ip = parse_ip(text[ho:ho + hl])
    if ip is None:
        return (OK, ho, hl, bytes(4), bytes(16), 0, port)
    if to4(ip) is not None:
        return (OK, ho, hl, to4(ip), bytes(16), HAS_IPV4, port)
    return (OK, ho, hl, bytes(4), ip, HAS_IPV6, port)


def ip_string(ip: bytes) -> bytes:
    """IP.String() of 4 or 16 bytes."""
    if len(ip) == 16 and to4(ip) is not None:
        ip = to4(ip)
    if len(ip) == 4:
        return b".".join(b"%d" % x for x in ip)
    g = [int.from_bytes(ip[2 * i:2 * i + 2], "big") for i in range(8)]
    best = (0, 0)   # (length, -start): the longest run of zero groups, the first on a tie
    i = 0
    while i < 8:
        j = i
        while j < 8 and g[j] == 0:
            j += 1
        if j - i >= 2 and j - i > best[0]:
            best = (j - i, i)
        i = max(j, i + 1)
    if best[0] == 0:
        return b":".join(b"%x" % x for x in g)
    a, b = best[1], best[1] + best[0]
    return b":".join(b"%x" % x for x in g[:a]) + b"::" + b":".join(b"%x" % x for x in g[b:])


def format(ip: bytes, family: int, port: int):   # noqa: A001
    """Rule F: the text, or FAMILY.  ``ip`` is 16 bytes; family 4 takes its first four."""
    if family not in (4, 16):
        return FAMILY
    host = ip_string(ip[:4] if family == 4 else ip[:16])
    if b":" in host:
        host = b"[" + host + b"]"
    return host + b":" + b"%d" % port
