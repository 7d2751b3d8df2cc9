"""ClientHello cases for the SNI kernel (hysteria_amd/csrc/sniff.hip), shared by
the CPU tier (tests/test_sniff.py, through tests/emu/sniff_main.cpp) and the GPU
tier (tests/test_gpu_sniff.py).  Expected results come from tests/sni_ref.py.
"""
import functools

import numpy as np

import sni_ref

SENTINEL = 0xA5
NAME_STRIDE = 255
GRID_CAP_MSGS = (1 << 16) * 4   # sniff.hip: kGridCap workgroups of kWaves messages


def _u16(v):
    return int(v).to_bytes(2, "big")


def ext(typ, body):
    return _u16(typ) + _u16(len(body)) + body


def sni_body(names, list_len=None, trail=b""):
    """server_name extension body from (name type, name) entries."""
    lst = b"".join(bytes([t]) + _u16(len(nm)) + nm for t, nm in names)
    return _u16(len(lst) if list_len is None else list_len) + lst + trail


def hello(exts=(), sid=32, suites=b"\x13\x01\x13\x02", comp=b"\x00", ext_len=None, tail=b"", raw_exts=None,
          body_len=None, typ=1):
    """A ClientHello handshake message.  exts: (type, body) pairs, or None for no
    extensions block at all; raw_exts replaces the encoded extensions."""
    body = b"\x03\x03" + bytes((7 * i + 1) & 0xFF for i in range(32)) + bytes([sid]) + bytes(range(sid))
    body += _u16(len(suites)) + suites + bytes([len(comp)]) + comp
    if exts is not None or raw_exts is not None:
        e = raw_exts if raw_exts is not None else b"".join(ext(t, b) for t, b in exts)
        body += _u16(len(e) if ext_len is None else ext_len) + e
    body += tail
    n = len(body) if body_len is None else body_len
    return bytes([typ]) + n.to_bytes(3, "big") + body


def _name(n, last=b"m"):
    return (b"abcdefghi." * 30)[:n - 1] + last if n else b""


COMMON = [(0x0a, b"\x00\x02\x00\x1d"), (0x0b, b"\x01\x00"), (0x2b, b"\x02\x03\x04"), (0x10, b"\x00\x03\x02h2")]


def with_sni(body, before=COMMON[:2], after=COMMON[2:], **kw):
    return hello(list(before) + [(0, body)] + list(after), **kw)


@functools.lru_cache(maxsize=None)
def generator_cases():
    """(name, message) pairs, each built from a valid hello."""
    host = b"example.org"
    good = sni_body([(0, host)])
    c = [
        ("valid", with_sni(good)),
        ("valid_sni_first", with_sni(good, before=())),
        ("valid_sni_last", with_sni(good, after=())),
        ("no_extensions_block", hello(None)),
        ("empty_extensions_block", hello([])),
        ("no_type_0", hello(COMMON)),
        ("only_non_host_entries", with_sni(sni_body([(1, b"abc"), (7, b"q")]))),
        ("host_after_other_entry", with_sni(sni_body([(3, b"zz"), (0, host)]))),
        ("host_before_other_entry", with_sni(sni_body([(0, host), (3, b"zz")]))),
        ("trailing_dot", with_sni(sni_body([(0, b"example.org.")]))),
        ("inner_dot_only", with_sni(sni_body([(0, b".example.org")]))),
        ("two_host_names", with_sni(sni_body([(0, b"a.example"), (0, b"b.example")]))),
        ("two_host_names_apart", with_sni(sni_body([(0, b"a.example"), (2, b"x"), (0, b"b.example")]))),
        ("empty_name", with_sni(sni_body([(0, b"")]))),
        ("empty_name_other_type", with_sni(sni_body([(5, b""), (0, host)]))),
        ("empty_name_list", with_sni(sni_body([]))),
        ("empty_sni_body", with_sni(b"")),
        ("one_byte_sni_body", with_sni(b"\x00")),
        ("list_len_short", with_sni(sni_body([(0, host)], list_len=len(host) + 2))),
        ("list_len_long", with_sni(sni_body([(0, host)], list_len=len(host) + 4))),
        ("list_trailing_bytes", with_sni(sni_body([(0, host)], trail=b"\x00"))),
        ("entry_header_truncated", with_sni(_u16(len(host) + 5) + b"\x00" + _u16(len(host)) + host + b"\x00\x00")),
        ("entry_name_truncated", with_sni(_u16(len(host) + 2) + b"\x00" + _u16(len(host) + 1) + host[:-1])),
        ("odd_cipher_suites", with_sni(good, suites=b"\x13\x01\x13")),
        ("no_cipher_suites", with_sni(good, suites=b"")),
        ("no_compression", with_sni(good, comp=b"")),
        ("duplicate_type_0", hello([(0, good), COMMON[0], (0, good)])),
        ("duplicate_type_0_adjacent", hello([(0, good), (0, good)])),
        ("duplicate_other_type", hello([COMMON[0], (0, good), COMMON[1], COMMON[0]])),
        ("duplicate_other_type_before_sni", hello([COMMON[0], COMMON[0], (0, good)])),
        ("ext_header_truncated", hello(raw_exts=ext(0, good) + b"\x00\x0a\x00")),
        ("ext_body_truncated", hello(raw_exts=ext(0, good) + b"\x00\x0a\x00\x05abc")),
        ("ext_block_shorter", with_sni(good, ext_len=len(ext(0, good)))),
        ("ext_block_longer", with_sni(good, ext_len=1000)),
        ("ext_len_truncated", hello(None, tail=b"\x00")),
        ("trailing_after_extensions", with_sni(good, tail=b"\x00")),
        ("wrong_uint24_length", with_sni(good, body_len=3)),
        ("uint24_length_max", with_sni(good, body_len=0xFFFFFF)),
        ("type_byte_2", with_sni(good, typ=2)),
        ("type_byte_0", with_sni(good, typ=0)),
        ("type_byte_22", with_sni(good, typ=0x16)),
        ("sid_past_end", hello(None)[:50]),
        ("suites_past_end", hello(None, suites=b"\x13\x01" * 4)[:-7]),
        ("compression_past_end", hello(None, comp=b"\x00\x01")[:-1]),
        ("truncated_random", hello(None)[:30]),
    ]
    full = with_sni(good)
    c += [(f"len_{k}", full[:k]) for k in range(5)]
    c += [("len_38", full[:38]), ("len_39", full[:39])]
    for n in (1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 300):
        c.append((f"name_len_{n}", with_sni(sni_body([(0, _name(n))]))))
    c.append(("name_len_255_dot", with_sni(sni_body([(0, _name(255, b"."))]))))
    c.append(("name_len_256_then_dup", hello([(0, sni_body([(0, _name(256))])), COMMON[0], COMMON[0]])))
    for k in (255, 256, 257, 300):
        exts = [(t, bytes([t & 0xFF])) for t in range(1, k)] + [(0, good)]
        c.append((f"extensions_{k}", hello(exts)))
    c.append(("extensions_257_sni_first", hello([(0, good)] + [(t, b"") for t in range(1, 257)])))
    c.append(("extensions_256_dup_last", hello([(0, good)] + [(t, b"") for t in range(1, 255)] + [(200, b"")])))
    c.append(("extensions_257_truncated_last", hello(raw_exts=b"".join(ext(t, b"") for t in range(1, 257))
                                                     + b"\x01\x01\x00\x04ab")))
    # a duplicate found by each lane group of the search (entries 0, 63, 64, 191)
    for at in (0, 63, 64, 191):
        exts = [(t + 1, b"") for t in range(200)]
        c.append((f"dup_of_entry_{at}", hello(exts + [(at + 1, b"")] + [(0, good)])))
    assert len({n for n, _ in c}) == len(c)
    return tuple(c)


def _offsets(sid, pad):
    """A hello with a padding extension of `pad` bytes before server_name, and
    where its fields start."""
    host = b"window.example"
    msg = hello([(21, bytes(pad)), (0, sni_body([(0, host)])), COMMON[0]], sid=sid)
    ext_len_at = 4 + 34 + 1 + sid + 2 + 4 + 1 + 1
    sni_hdr = ext_len_at + 2 + 4 + pad
    return msg, {"ext_len": ext_len_at, "pad_hdr": ext_len_at + 2, "sni_hdr": sni_hdr, "list_hdr": sni_hdr + 4,
                 "entry_hdr": sni_hdr + 6, "name": sni_hdr + 9, "name_end": sni_hdr + 9 + len(host) - 1,
                 "next_hdr": sni_hdr + 9 + len(host)}


WINDOW_EDGE = (62, 63, 64, 65, 126, 127, 128, 129)
STAGE_EDGE = (1022, 1023, 1024, 1025)   # sniff.hip stages kStage = 1024 bytes of a message at a time


@functools.lru_cache(maxsize=None)
def window_cases():
    """Hellos whose extensions length field, extension headers, name-list header,
    entry header and name each start at bytes 62..65 (and 126..129) of the
    message, the edges of a 64-byte read window filled at byte 0; and, behind a
    long padding extension, at bytes 1022..1025, where the kernel stages the
    next part of the message."""
    fields = ("ext_len", "pad_hdr", "sni_hdr", "list_hdr", "entry_hdr", "name", "name_end", "next_hdr")
    want = {(f, p) for f in fields for p in WINDOW_EDGE}
    want |= {(f, p) for f in fields[2:] for p in STAGE_EDGE}
    out = []
    for sid in range(33):
        for pad in list(range(0, 80)) + (list(range(930, 985)) if sid == 0 else []):
            msg, o = _offsets(sid, pad)
            hit = {(f, p) for f, p in o.items() if (f, p) in want}
            if hit:
                want -= hit
                assert msg[o["name"]:o["name"] + 14] == b"window.example"
                out.append((f"window_sid{sid}_pad{pad}", msg))
    # what the list must hold: these four fields at bytes 62..65 (the rest is reached where the layout allows)
    assert not {w for w in want if w[0] in ("ext_len", "sni_hdr", "list_hdr", "name") and w[1] < 100}, want
    assert not {w for w in want if w[1] > 1000}, want
    return tuple(out)


FUZZ_SEED = 7


@functools.lru_cache(maxsize=None)
def fuzz_cases(seed=FUZZ_SEED, count=512):
    """`count` single-byte mutations of one valid hello with many small extensions."""
    rng = np.random.default_rng(seed)
    exts = [(t, bytes([t, t])) for t in range(40, 64)] + [(0, sni_body([(0, b"fuzz.example.net")]))] + \
           [(t, bytes([t])) for t in range(64, 84)]
    base = hello(exts, sid=8)
    out = []
    for k in range(count):
        pos = int(rng.integers(0, len(base)))
        m = bytearray(base)
        m[pos] ^= int(rng.integers(1, 256))
        out.append((f"fuzz{k}_at{pos}", bytes(m)))
    return tuple(out)


def all_cases():
    return list(generator_cases()) + list(window_cases()) + list(fuzz_cases())


def as_record(msg, version=b"\x03\x01", ctype=0x16):
    return bytes([ctype]) + version + _u16(len(msg)) + msg


@functools.lru_cache(maxsize=None)
def record_cases():
    """(name, first bytes of a TCP stream): every hello case as the body of one
    TLS record, then the record layer's own cases."""
    c = [("rec_" + n, as_record(m)) for n, m in all_cases()]
    good = as_record(generator_cases()[0][1])
    c += [(f"rec_prefix_{k}", good[:k]) for k in range(8)]
    c += [
        ("rec_one_short", good[:-1]),
        ("rec_stream_goes_on", good + b"\x17\x03\x03\x00\x02hi"),
        ("rec_content_type_15", b"\x15" + good[1:]),
        ("rec_content_type_17", b"\x17" + good[1:]),
        ("rec_content_type_18", b"\x18" + good[1:]),
        ("rec_major_2", good[:1] + b"\x02" + good[2:]),
        ("rec_minor_9", good[:2] + b"\x09" + good[3:]),
        ("rec_minor_10", good[:2] + b"\x0a" + good[3:]),
        ("rec_empty_body", b"\x16\x03\x01\x00\x00"),
        ("rec_body_3", b"\x16\x03\x01\x00\x03\x01\x00\x00"),
        ("rec_http", b"GET / HTTP/1.1\r\nHost: example.com\r\n\r\n"),
        ("rec_need_max", b"\x16\x03\x03\xff\xff" + bytes(100)),
    ]
    assert len({n for n, _ in c}) == len(c)
    return tuple(c)


def expected(cases, fn, stride=NAME_STRIDE):
    """[(status, name_len, name_off, need, name)] by the restatement."""
    return [fn(m, stride) for _, m in cases]


def small_templates():
    """Hellos of 45 to 64 bytes for the batch above the grid cap: no extensions,
    a short name, and malformed ones."""
    t = [hello(None, sid=0, suites=b"\x13\x01")]
    for nm in (b"a", b"bc", b"d.e", b"f.gh"):
        t.append(hello([(0, sni_body([(0, nm)]))], sid=0, suites=b"\x13\x01"))
    t.append(hello([(0, sni_body([(0, b"x.")]))], sid=0, suites=b"\x13\x01"))
    t.append(hello([(0, sni_body([(0, b"xy")]))], sid=0, suites=b"\x13\x01", tail=b"\x00"))
    t.append(hello([(0, sni_body([(0, b"xy")]))], sid=0, suites=b"\x13\x01", typ=2))
    t.append(hello([(5, b""), (5, b"")], sid=0, suites=b"\x13\x01"))
    assert all(45 <= len(x) <= 64 for x in t)
    return t


def pack(msgs, gap=0, fill=SENTINEL, align=1):
    """(buffer, off, len): messages one after another, `gap` fill bytes (or more,
    up to the next multiple of `align`) after each."""
    lens = np.array([len(m) for m in msgs], np.uint32)
    off = np.zeros(len(msgs), np.uint64)
    parts, at = [], 0
    for i, m in enumerate(msgs):
        off[i] = at
        end = at + len(m) + gap
        end += -end % align
        parts.append(m + bytes([fill]) * (end - at - len(m)))
        at = end
    return np.frombuffer(b"".join(parts) + bytes([fill]) * max(gap, 1), np.uint8).copy(), off, lens


# ------------------------------------------------------------------ QUIC Initials
def initial_for(msg, k):
    """A client Initial whose CRYPTO data is `msg`: one frame, two shuffled
    frames or a frame behind padding, by k; V1 and V2."""
    import quic_cases as qc
    from oracle import quic_ref as ref
    if k % 3 == 1 and len(msg) > 1:
        cut = 1 + (k * 37) % (len(msg) - 1)
        frames = qc._crypto(cut, msg[cut:]) + b"\x00" * (k % 5) + qc._crypto(0, msg[:cut])
    elif k % 3 == 2:
        frames = b"\x00" * (k % 70) + b"\x01" + qc._crypto(0, msg)
    else:
        frames = qc._crypto(0, msg)
    frames += b"\x00" * max(0, 24 - len(frames))   # room for the header-protection sample
    dcid = bytes((k * 11 + j) & 0xFF for j in range(8 + k % 13))
    return ref.client_initial(dcid, b"", ref.V2 if k % 2 else ref.V1, b"", 2, 1 + k % 4, frames)


@functools.lru_cache(maxsize=None)
def quic_cases(fuzz=True):
    """(name, packet, expected CRYPTO payload or None): every hello case inside a
    client Initial, then quic_cases.crypto_packets() (good and bad Initials with
    random payloads).  None where the device's ReadCryptoPayload fails."""
    import quic_cases as qc
    hellos = list(generator_cases()) + list(window_cases()) + (list(fuzz_cases()) if fuzz else [])
    out = [("quic_" + n, initial_for(m, k), m) for k, (n, m) in enumerate(hellos)]
    for n, p in qc.crypto_packets(1):
        st, data = qc.oracle_read(p)
        out.append(("quic_pkt_" + n, p, None if st or n == "too_many_frames" else data))
    return tuple(out)


def expected_quic(cases, stride=NAME_STRIDE):
    return [sni_ref.quic_sniff(pl, stride) for _, _, pl in cases]
