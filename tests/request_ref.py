"""Restatement of include/hyobfs_request.h's rules V, R, Q, S, T, G, U, K, C and W in
Python, written from the Go text (core/internal/protocol/proxy.go:32-149,
extras/utils/portunion.go, extras/sniff/sniff.go:67-89, 121-125) as a blocking
reader over a byte string, not from hysteria_amd/csrc/request_rules.h.  It never
calls the library; rules H and I come from tests/addr_ref.py, rule G is restated
from the header.  TEST INFRASTRUCTURE ONLY.

All texts are bytes."""
import addr_ref as A

OK = 0
NEED_MORE, ADDR_LEN, PADDING_LEN, MSG_LEN, CAP, NO_ADDR, HOST, UNION = range(-86, -94, -1)
SNIFF_NAME_CAP, SNIFF_NEED_MORE, SNIFF_HOST = -56, -59, -66   # include/hyobfs_sniff.h
MAX_ADDR, MAX_MSG, MAX_PADDING, FRAME_TYPE = 2048, 2048, 4096, 0x401
PADDING_CHARS = b"abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789"
M64 = (1 << 64) - 1


# ------------------------------------------------------------------ rule V
def varint(v: int, size: int = 0) -> bytes:
    """quicvarint.Append; ``size`` forces a (possibly non-minimal) form."""
    size = size or (1 if v < 1 << 6 else 2 if v < 1 << 14 else 4 if v < 1 << 30 else 8)
    assert v < 1 << (8 * size - 2)
    return (v | {1: 0, 2: 1, 4: 2, 8: 3}[size] << (8 * size - 2)).to_bytes(size, "big")


def _read_varint(b: bytes, at: int):
    """quicvarint.Read at b[at:]: (value, end), or (None, the smallest total that lets it finish)."""
    if len(b) < at + 1:
        return None, at + 1
    size = 1 << (b[at] >> 6)   # the first byte says how many bytes the varint has
    if len(b) < at + size:
        return None, at + size
    return int.from_bytes(b[at:at + size], "big") & ((1 << (8 * size - 2)) - 1), at + size


def _text_and_padding(b: bytes, at: int, bad_len, err: int):
    """The part ReadTCPRequest and ReadTCPResponse share, as a blocking reader meets it: a length, the text, the
    padding's length, the padding.  (status, need, text_off, text_len, end)."""
    n, at = _read_varint(b, at)
    if n is None:
        return (NEED_MORE, at, 0, 0, 0)
    if bad_len(n):
        return (err, 0, 0, 0, 0)
    text = b[at:at + n]
    if len(text) < n or len(b) == at + n:   # io.ReadFull blocks; then the next read wants one byte at least
        return (NEED_MORE, at + n + 1, 0, 0, 0)
    p, end = _read_varint(b, at + n)
    if p is None:
        return (NEED_MORE, end, 0, 0, 0)
    if p > MAX_PADDING:
        return (PADDING_LEN, 0, 0, 0, 0)
    if len(b) < end + p:   # io.CopyN(io.Discard, r, paddingLen)
        return (NEED_MORE, end + p, 0, 0, 0)
    return (OK, 0, at, n, end + p)


# ------------------------------------------------------------------ rules R and T
def read_tcp_request(b: bytes):
    """ReadTCPRequest: (status, need, addr_off, addr_len, consumed)."""
    return _text_and_padding(b, 0, lambda n: n == 0 or n > MAX_ADDR, ADDR_LEN)


def read_tcp_response(b: bytes):
    """ReadTCPResponse: (status, need, ok, msg_off, msg_len, consumed)."""
    if len(b) < 1:   # io.ReadFull(r, status[:])
        return (NEED_MORE, 1, 0, 0, 0, 0)
    st, need, off, n, end = _text_and_padding(b, 1, lambda n: n > MAX_MSG, MSG_LEN)
    return (st, need, int(st == OK and b[0] == 0), off, n, end)


# ------------------------------------------------------------------ rule G
def _mix(x):
    x ^= x >> 30
    x = x * 0xBF58476D1CE4E5B9 & M64
    x ^= x >> 27
    x = x * 0x94D049BB133111EB & M64
    return x ^ x >> 31


def padding(seed: int, item: int, n: int) -> bytes:
    s = _mix(seed + 0x9E3779B97F4A7C15 * (item + 1) & M64)
    out = bytearray()
    for k in range(n):
        z = _mix(s + 0x9E3779B97F4A7C15 * (k // 4 + 1) & M64)
        out.append(PADDING_CHARS[(z >> 16 * (k % 4) & 0xFFFF) % 62])
    return bytes(out)


# ------------------------------------------------------------------ rules Q and S
def write_tcp_request(addr: bytes, pad_len: int, seed: int, item: int) -> bytes:
    return varint(FRAME_TYPE) + varint(len(addr)) + addr + varint(pad_len) + padding(seed, item, pad_len)


def write_tcp_response(ok: bool, msg: bytes, pad_len: int, seed: int, item: int) -> bytes:
    return bytes([0 if ok else 1]) + varint(len(msg)) + msg + varint(pad_len) + padding(seed, item, pad_len)


# ------------------------------------------------------------------ rules U and K
def _parse_uint16(s: bytes):
    """strconv.ParseUint(s, 10, 16)."""
    if not s or any(c not in b"0123456789" for c in s):
        return None
    v = int(s)
    return v if v <= 65535 else None


def parse_port_union(s: bytes):
    """ParsePortUnion: the normalised [(start, end)], or None."""
    if s in (b"all", b"*"):
        return [(0, 65535)]
    out = []
    for part in s.split(b","):
        if b"-" in part:
            ends = part.split(b"-")
            if len(ends) != 2:
                return None
            a, b = _parse_uint16(ends[0]), _parse_uint16(ends[1])
            if a is None or b is None:
                return None
            out.append((min(a, b), max(a, b)))
        else:
            p = _parse_uint16(part)
            if p is None:
                return None
            out.append((p, p))
    out.sort()
    norm = [out[0]]
    for cur in out[1:]:
        last = norm[-1]
        if cur[0] <= last[1] + 1:
            norm[-1] = (last[0], max(last[1], cur[1]))
        else:
            norm.append(cur)
    return norm


def contains(union, port: int) -> bool:
    """PortUnion.Contains at Check: None is the nil union."""
    return union is None or any(a <= port <= b for a, b in union)


# ------------------------------------------------------------------ rule C
def atoi(s: bytes):
    """strconv.Atoi: the value, or None."""
    digits = s[1:] if s[:1] in (b"+", b"-") else s
    if not digits or any(c not in b"0123456789" for c in digits):
        return None
    v = -int(digits) if s[:1] == b"-" else int(digits)
    return v if -(1 << 63) <= v < 1 << 63 else None


def check(text: bytes, is_udp: bool, rewrite_domain: bool, tcp_ports, udp_ports) -> bool:
    if text.startswith(b"@"):
        return False
    st, ho, hl, po, pl = A.split(text)
    if st != A.OK:
        return False
    if not rewrite_domain and A.parse_ip(text[ho:ho + hl]) is None:
        return False
    v = atoi(text[po:po + pl])
    if v is None:
        return False
    return contains(udp_ports if is_udp else tcp_ports, v & 0xFFFF)


# ------------------------------------------------------------------ rule W
def join_host_port(host: bytes, port: bytes) -> bytes:
    if b":" in host or b"%" in host:
        return b"[" + host + b"]:" + port
    return host + b":" + port


def rewrite(addr: bytes, checked: bool, name: bytes, sniff_status: int, gate: int = 0):
    """(status, text, rewritten); the text is b"" beside a status that is not OK."""
    if gate != 0:
        return (NO_ADDR, b"", 0)
    if not checked:
        return (OK, addr, 0)
    if sniff_status == OK:
        if not name:
            return (OK, addr, 0)
        i = addr.rfind(b":")
        if i < 0:
            return (A.MISSING_PORT, b"", 0)
        return (OK, join_host_port(name, addr[i + 1:]), 1)
    if sniff_status in (SNIFF_NEED_MORE, SNIFF_HOST, SNIFF_NAME_CAP):
        return (HOST, b"", 0)
    return (OK, addr, 0)
