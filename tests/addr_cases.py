"""Case lattice of the request-address calls (include/hyobfs_addr.h), shared by the
CPU tier (tests/test_addr.py: the scalar ABI, and the kernels compiled for the host
under AddressSanitizer) and the GPU tier (tests/test_gpu_addr.py).  Expected values
come from tests/addr_ref.py alone; tests/golden/addr_vectors.json records them for
the rule corpora (``golden()`` regenerates it).

A parse case is a dict: name, items (the texts), mode ("poison": every text in a
slot whose surroundings are ':' ']' '[' and digits, the offsets running through all
four alignments; "packed": back to back).  A format case: name, items = [(ip16,
family, port)], stride, mis (misalignment of the output's first byte), meta (bool).
"""
from __future__ import annotations

import functools
import ipaddress
import random
import struct

import numpy as np

import addr_ref as R

GUARD = 0xA5
GUARD_BYTES = 64
POISON = b":][0123456789"
NS = (1, 3, 4, 5, 63, 64, 65, 257)
ADDR_LENS = (1, 63, 64, 65, 127, 128, 129, 255, 256, 2047, 2048)   # 0 and 2049: raw_items()

# ------------------------------------------------------------------ rule corpora
H_CORPUS = [b"", b":", b":80", b"host:", b"a:b:80", b"[::1]:80", b"[::1]", b"[::1]80", b"[::1]::80", b"[::1",
            b"[a]b:80", b"a[b:80", b"[a[b]:80", b"a]b:80", b"[a]:8]0", b"[]:80", b"@SpeedTest",
            # two rules at once: the order decides
            b"a:b[:8]0",      # TOO_MANY_COLONS before the brackets
            b"a[b]:80",       # '[' before ']'
            b"[a[b]]:80",     # "]]" is MISSING_PORT before the '['
            b"[a]b]:80",      # MISSING_PORT (the byte behind the first ']') before the second ']'
            b"[a]:[8]0",      # '[' before ']'
            b"[a:80",         # MISSING_BRACKET although the colon is there
            b"[a]:b:80", b"[[a]:80", b"a:80]", b"[a]:80]", b"[a]:", b"]:80", b"[:80", b"[]:", b"1.2.3.4:53",
            b"[2001:db8::1]:443", b"example.com:443", b"2001:db8::1:443"]

P_CORPUS = [b"0", b"65535", b"65536", b"00080", b"0" * 40 + b"80", b"9" * 25, b"+80", b"-1", b"8_0", b" 80", b"80 ",
            "８０".encode(), b"", b"0" * 64, b"99999", b"100000", b"0065535", b"0065536", b"8a", b"a8", b"0x50", b"4294967376",
            b"18446744073709551696"]

I_PASS = [b"::ffff:1.2.3.4", b"1:2:3:4:5:6:7::", b"::2:3:4:5:6:7:8", b"::1.2.3.4", b"1::2:1.2.3.4"]
I_REFUSE = [b"1:2:3:4:5:6:7:8::", b"01.2.3.4", b"fe80::1%eth0", b"00001::", b"1.2.3.4.5", b"::a.2.3.4"]
I_MORE = [b"::", b"::1", b"1::", b":::", b":1", b"1:", b"1:::2", b"1::2::3", b"1:2:3:4:5:6:7", b"1:2:3:4:5:6:7:8:9",
          b"1:2:3:4:5:6:1.2.3.4", b"1:2:3:4:5:6:7:1.2.3.4", b"1.2.3", b"1..2.3", b".1.2.3", b"1.2.3.", b"256.1.1.1",
          b"0.0.0.0", b"255.255.255.255", b"ABCD:EF01:2345:6789:abcd:ef01:2345:6789", b"FE80::A", b"%eth0", b"%1::1",
          b"1%.2.3.4", b"1.2.3.4%5", b"::%", b"::1%", b"1:2:3:4:5:6:7:8", b"1:2:3:4:5:6:7:8:", b":1:2:3:4:5:6:7:8",
          b"::1:2:3:4:5:6:7:8", b"1:2:3:4::5:6:7:8", b"1:2:3::5:6:7:8", b"12345::", b"::fffff", b"g::", b"::g",
          b"1.2.3.4:", b"1:2.3.4.5::", b"::1.2.3", b"::1.2.3.4.5", b"::1.2.3.04", b"::1.2.3.256", b"::1.2.3.4:5",
          b"1:2:3:4:5:1.2.3.4", b"1:2:3:4:5::1.2.3.4", b"1:2:3:4:5:6::1.2.3.4", b"::ffff:102:304", b"0:0:0:0:0:ffff:1.2.3.4",
          b"example.com", b"localhost", b"1234", b"deadbeef", b"", b".", b":", b"1.2.3.4 ", b" 1.2.3.4", b"1.2.3.-4",
          b"00.0.0.0", b"0.00.0.0", b"1.2.3.0004", b"999999999999.1.1.1", b"4294967297.1.1.1", b"::00000", b"::0000",
          b"ffff:ffff:ffff:ffff:ffff:ffff:255.255.255.255",       # 45 bytes: the longest literal
          b"ffff:ffff:ffff:ffff:ffff:ffff:255.255.255.2555",      # 46: a near miss
          b"0000:0000:0000:0000:0000:0000:0000:0000:0000",        # 44, nine groups
          b"ffff:ffff:ffff:ffff:ffff:ffff:ffff:ffff"]
I_CORPUS = I_PASS + I_REFUSE + I_MORE
assert len(I_MORE[-4]) == 45 and len(I_MORE[-3]) == 46

# rule T: v4-mapped against v4-compatible and neighbours
T_CORPUS = [b"::ffff:1.2.3.4", b"::ffff:102:304", b"0:0:0:0:0:ffff:102:304", b"::1.2.3.4", b"::102:304", b"::fffe:1.2.3.4",
            b"::1:ffff:1.2.3.4", b"1.2.3.4", b"::ffff:0.0.0.0", b"::ffff:0:0", b"::", b"example.com"]


def _ip(text: str) -> bytes:
    return ipaddress.ip_address(text).packed.ljust(16, b"\0")


# rule F: (16 bytes, family, port)
F_CORPUS = [(bytes(16), 16, 0), (_ip("::1"), 16, 9), (_ip("1::"), 16, 10), (_ip("2001:db8:0:0:1:0:0:1"), 16, 65535),
            (_ip("2001:0:0:1:0:0:0:1"), 16, 443), (_ip("1:0:2:3:4:5:6:7"), 16, 53), (_ip("1:2:3:4:5:6:7:0"), 16, 1),
            (_ip("0:2:3:4:5:6:7:8"), 16, 2), (_ip("1:0:0:2:0:0:0:0"), 16, 3), (_ip("0:0:1:0:0:2:0:0"), 16, 4),
            (_ip("::ffff:1.2.3.4"), 16, 80), (_ip("::1.2.3.4"), 16, 80), (_ip("::fffe:1.2.3.4"), 16, 80),
            (b"\xff" * 16, 16, 65535), (_ip("a:b:c:d:e:f:10:100"), 16, 100), (_ip("1000:200:30:4:0:0:0:5"), 16, 1000),
            (_ip("1.2.3.4"), 4, 53), (_ip("0.0.0.0"), 4, 0), (_ip("255.255.255.255"), 4, 65535), (_ip("10.0.100.9"), 4, 10000),
            (bytes([1, 2, 3, 4]) + b"\xee" * 12, 4, 99),   # family 4 takes the first four bytes only
            (_ip("::1"), 0, 80), (_ip("::1"), 6, 80), (_ip("::1"), 15, 80), (_ip("1.2.3.4"), 255, 80), (_ip("::1"), 17, 80)]


# ------------------------------------------------------------------ the kernel lattice
def _host(n: int) -> bytes:
    return bytes((b"abcdefghijklmnopqrstuvwxyz0123456789.-"[(i * 7 + n) % 38]) for i in range(n))


def length_items() -> list[bytes]:
    """Every address length of the lattice: valid plain and bracketed forms, a port of
    leading zeros that fills the length, and for the lengths beyond one window every
    rule-H failure (and a port failure) with its cause in the last window."""
    out = [b":", b"a"]   # length 1
    for n in ADDR_LENS[1:]:
        out.append(_host(n - 3) + b":80")
        out.append(b"[" + _host(n - 5) + b"]:80")
        out.append(b"h:" + b"0" * (n - 4) + b"80")
        out.append(b"h:" + b"0" * (n - 7) + b"65536")
        out.append(b"h:" + b"1" + b"0" * (n - 3))
        out.append(_host(n - 6) + b":12345")   # at 65 and 129 the digits lie in two windows
        if n > 64:   # six bytes at the end hold the cause
            plain = (b"abcx80", b"a:8:80", b"[a:800", b"]a:800", b"a:8x00", b"a:+800")
            out += [_host(n - 6) + t for t in plain]
            brack = (b"aa:800", b"a]x:80", b"]::800", b"aaa]80", b"a:aaa]", b"[]:800", b"]:8]00", b"a]:80]", b"a]:8 0")
            out += [b"[" + _host(n - 7) + t for t in brack]
    assert all(len(x) <= R.MAX_ADDR for x in out) and {len(x) for x in out} >= set(ADDR_LENS)
    return out


def raw_items() -> list[bytes]:
    """Lengths the convenience layers never produce: 0 and 2049 (TOO_LONG although it would split)."""
    return [b"", _host(2049 - 3) + b":80"]


def literal_items() -> list[bytes]:
    out = []
    for s in I_CORPUS + T_CORPUS:
        out.append((b"[" + s + b"]:53") if b":" in s else (s + b":53"))
        if b":" in s:
            out.append(s + b":53")   # unbracketed: TOO_MANY_COLONS, or a shorter literal in front of the last ':'
    return out


def random_items(n: int = 300, seed: int = 0xADD2) -> list[bytes]:
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        kind = rng.randrange(6)
        if kind == 0:
            t = b"%d.%d.%d.%d:%d" % (*(rng.randrange(256) for _ in range(4)), rng.randrange(65536))
        elif kind == 1:
            ip = bytes(rng.choice((0, 0, rng.randrange(256))) for _ in range(16))
            t = b"[" + str(ipaddress.IPv6Address(ip)).encode() + b"]:%d" % rng.randrange(65536)
        elif kind == 2:
            t = _host(rng.randrange(1, 300)) + b":%d" % rng.randrange(70000)
        else:   # a valid text with a few bytes mutated
            t = bytearray(rng.choice((b"10.20.30.40:8080", b"[2001:db8::8:800:200c:417a]:443", b"www.example.org:65535",
                                      b"[::ffff:192.0.2.128]:00053")))
            for _ in range(rng.randrange(1, 4)):
                p = rng.randrange(len(t))
                op = rng.randrange(3)
                if op == 0:
                    t[p] = rng.choice(b":[]%.0189afg ")
                elif op == 1:
                    t.insert(p, rng.choice(b":[]%.0189afg "))
                else:
                    del t[p]
            t = bytes(t)
        out.append(t)
    return out


@functools.lru_cache(maxsize=None)
def all_items() -> tuple:
    ports = [b"h:" + p for p in P_CORPUS] + [b"[::1]:" + p for p in P_CORPUS[:6]]
    return tuple(H_CORPUS + ports + literal_items() + length_items() + raw_items() + random_items())


def parse_cases() -> list[dict]:
    items = list(all_items())
    rng = random.Random(0x51CE)
    cases = [dict(name="lattice", items=items, mode="poison"), dict(name="lattice_packed", items=items, mode="packed")]
    for n in NS:
        cases.append(dict(name=f"n{n}", items=[rng.choice(items) for _ in range(n)], mode="poison"))
    return cases


def layout(case) -> tuple[bytes, list[int], list[int]]:
    """(src, off, len).  "poison": gaps of 1..8 poison bytes between the texts (and
    before the first, after the last), so the offsets take every alignment."""
    rng = random.Random(len(case["items"]))
    buf, off = bytearray(), []
    for k, t in enumerate(case["items"]):
        if case["mode"] == "poison":
            gap = 1 + (k * 3 + len(buf)) % 8
            buf += bytes(rng.choice(POISON) for _ in range(gap))
        off.append(len(buf))
        buf += t
    if case["mode"] == "poison":
        buf += bytes(rng.choice(POISON) for _ in range(9))
    return bytes(buf), off, [len(t) for t in case["items"]]


def expected_parse(items, offs) -> list[tuple]:
    """Per item (status, name_off, name_len, ipv4, ipv6, ip_flags, port), name_off from the buffer's start."""
    out = []
    for t, o in zip(items, offs):
        r = R.parse(t)
        out.append((r[0], (o + r[1]) if r[0] == R.OK else 0) + r[2:])
    return out


PARSE_OUT = (("status", np.int32, 1), ("name_off", np.uint64, 1), ("name_len", np.uint32, 1), ("ipv4", np.uint8, 4),
             ("ipv6", np.uint8, 16), ("ip_flags", np.uint8, 1), ("port", np.uint16, 1))


def check_parse(name, items, offs, got: dict) -> None:
    """``got``: the seven output arrays by name (numpy), exactly n items each."""
    exp = expected_parse(items, offs)
    for i, e in enumerate(exp):
        g = (int(got["status"][i]), int(got["name_off"][i]), int(got["name_len"][i]), bytes(got["ipv4"][4 * i:4 * i + 4]),
             bytes(got["ipv6"][16 * i:16 * i + 16]), int(got["ip_flags"][i]), int(got["port"][i]))
        assert g == e, (name, i, items[i][:80], g, e)


# ------------------------------------------------------------------ relay datagrams
def datagram(addr: bytes, data: bytes = b":]8[0", session: int = 0x3A5D5B3A, varint_len: int = 0) -> bytes:
    """A relay message whose fixed bytes and data are poison for the address parser."""
    n = len(addr)
    forms = [bytes([n])] if n < 64 else []
    forms += [struct.pack(">H", 0x4000 | n)] if n < 16384 else []
    v = forms[0] if not varint_len else {2: struct.pack(">H", 0x4000 | n), 4: struct.pack(">I", 0x80000000 | n)}[varint_len]
    return struct.pack(">IHBB", session, 0x3A3A, 0x5D, 0x5B) + v + addr + data


def udp_datagrams() -> tuple[list[bytes], list, list[int]]:
    """(datagrams, the address of each or None where the message does not parse, where it starts in the datagram)."""
    ds, addrs, at = [], [], []
    for k, t in enumerate(all_items()):
        if not 1 <= len(t) <= R.MAX_ADDR:
            continue
        vl = (1, 2, 4)[k % 3] if len(t) < 64 else (2, 4)[k % 2]
        ds.append(datagram(t, varint_len=0 if vl == 1 else vl))
        addrs.append(t)
        at.append(8 + vl)
    bad = [b"", bytes(8), datagram(b"a:1")[:10], datagram(b"a:1", data=b""),
           struct.pack(">IHBB", 1, 2, 0, 1) + b"\x00" + b"x",                      # address length 0
           struct.pack(">IHBB", 1, 2, 0, 1) + struct.pack(">H", 0x4000 | 2049) + _host(2046) + b":80" + b"d"]
    for k, d in enumerate(bad):
        ds.insert(7 * k, d)
        addrs.insert(7 * k, None)
        at.insert(7 * k, 0)
    return ds, addrs, at


# ------------------------------------------------------------------ format
def format_items(seed: int = 0xF0F0, n: int = 200) -> list[tuple]:
    rng = random.Random(seed)
    out = list(F_CORPUS)
    for _ in range(n):
        ip = b"".join(rng.choice((b"\0\0", b"\0\0", b"\0" + bytes([rng.randrange(256)]), rng.randbytes(2))) for _ in range(8))
        fam = rng.choice((16, 16, 16, 4, 4, rng.randrange(256)))
        out.append((ip, fam, rng.choice((0, 9, 10, 99, 100, 999, 1000, 9999, 10000, 65535, rng.randrange(65536)))))
    return out


def format_cases() -> list[dict]:
    items = format_items()
    rng = random.Random(0xF0C)
    cases = [dict(name="lattice47", items=items, stride=47, mis=0, meta=True),
             dict(name="lattice48_mis1", items=items, stride=48, mis=1, meta=True),
             dict(name="lattice53_mis3", items=items, stride=53, mis=3, meta=False),
             dict(name="lattice200_mis2", items=items[:70], stride=200, mis=2, meta=True)]
    for k, n in enumerate(NS):
        cases.append(dict(name=f"n{n}", items=[rng.choice(items) for _ in range(n)], stride=(47, 49, 50, 64)[k % 4], mis=k % 4,
                          meta=bool(k % 2)))
    return cases


META_DTYPE = np.dtype([("session_id", "<u4"), ("packet_id", "<u2"), ("reserved_", "<u2"), ("max_size", "<u4"),
                       ("addr_len", "<u4"), ("addr_off", "<u8")])
BASE_OFF = 0x1_0000_0040


def check_format(case, status, out_len, meta, out) -> None:
    """status / out_len: n items; meta: n META_DTYPE records that were filled with GUARD
    bytes before the call (or None); out: the n * stride bytes."""
    n, stride = len(case["items"]), case["stride"]
    guard32, guard64 = int.from_bytes(bytes([GUARD]) * 4, "little"), int.from_bytes(bytes([GUARD]) * 8, "little")
    assert len(out) == n * stride
    for i, (ip, fam, port) in enumerate(case["items"]):
        e = R.format(ip, fam, port)
        row = bytes(out[i * stride:(i + 1) * stride])
        if e == R.FAMILY:
            assert (int(status[i]), int(out_len[i]), row) == (R.FAMILY, 0, bytes(stride)), (case["name"], i)
        else:
            assert (int(status[i]), int(out_len[i]), row) == (R.OK, len(e), e + bytes(stride - len(e))), (case["name"], i, e)
        if meta is not None:
            m = meta[i]
            assert (int(m["session_id"]), int(m["max_size"])) == (guard32, guard32)   # the other fields are the caller's
            if e == R.FAMILY:
                assert (int(m["addr_len"]), int(m["addr_off"])) == (guard32, guard64)
            else:
                assert (int(m["addr_len"]), int(m["addr_off"])) == (len(e), BASE_OFF + i * stride)


# ------------------------------------------------------------------ the emulated driver's files
def blob_parse(case) -> bytes:
    buf, off, lens = layout(case)
    return (struct.pack("<III", 1, len(off), len(buf)) + buf + np.array(off, "<u8").tobytes()
            + np.array(lens, "<u4").tobytes())


def blob_parse_udp(datagrams) -> bytes:
    """Datagrams in a poison layout of their own; the driver parses them first."""
    case = dict(items=datagrams, mode="poison")
    buf, off, lens = layout(case)
    return (struct.pack("<III", 2, len(off), len(buf)) + buf + np.array(off, "<u8").tobytes()
            + np.array(lens, "<u4").tobytes())


def blob_format(case) -> bytes:
    b = struct.pack("<IIIIIQ", 3, len(case["items"]), case["stride"], case["mis"], int(case["meta"]), BASE_OFF)
    for ip, fam, port in case["items"]:
        b += ip + struct.pack("<BH", fam, port)
    return b


# ------------------------------------------------------------------ the golden file
def golden() -> dict:
    def hx(b):
        return bytes(b).hex()

    def txt(b):
        return bytes(b).decode("latin-1")
    g = {"split": [], "port": [], "ip": [], "parse": [], "format": []}
    for t in H_CORPUS:
        st, ho, hl, po, pl = R.split(t)
        g["split"].append({"text": txt(t), "hex": hx(t), "status": st, "host": [ho, hl], "port": [po, pl]})
    for t in P_CORPUS:
        g["port"].append({"text": txt(t), "hex": hx(t), "value": R.parse_port(t)})
    for t in I_CORPUS:
        ip = R.parse_ip(t)
        g["ip"].append({"text": txt(t), "hex": hx(t), "ip16": None if ip is None else hx(ip)})
    for t in T_CORPUS + H_CORPUS:
        t = (b"[" + t + b"]:53") if t in T_CORPUS and b":" in t else (t + b":53") if t in T_CORPUS else t
        st, no, nl, v4, v6, fl, port = R.parse(t)
        g["parse"].append({"text": txt(t), "hex": hx(t), "status": st, "name": [no, nl], "ipv4": hx(v4), "ipv6": hx(v6),
                           "ip_flags": fl, "port": port})
    for ip, fam, port in F_CORPUS:
        e = R.format(ip, fam, port)
        g["format"].append({"ip16": hx(ip), "family": fam, "port": port, "text": e if isinstance(e, int) else txt(e)})
    return g
