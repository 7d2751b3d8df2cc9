"""Edge-lattice cases for the realm punch matcher (hysteria_amd/csrc/realm.hip) and
the Gecko parse and encode kernels (hysteria_amd/csrc/gecko.hip), shared by the CPU
tier (tests/test_wire_cases.py, through tests/emu/wire_main.cpp under
AddressSanitizer) and the GPU tier (tests/test_gpu_realm.py, tests/test_gpu_gecko.py).

No side effects; imports only oracle.* and numpy.  Every expected value comes from
oracle/realm_ref.py and oracle/gecko_ref.py, never from the library.  Buffers carry
no slack: the last datagram, chunk or frame ends at its buffer's last byte, and an
entry whose bytes do not exist points at the end of the buffer.
"""
import functools
import random
import struct

import numpy as np

from oracle import gecko_ref as gref
from oracle import realm_ref as rref
from oracle import salamander_ref as sref

SENTINEL = 0xA5
GUARD = 100   # sentinel bytes compared on either side of a far-offset segment

# struct hyobfs_gecko_frame / hyobfs_gecko_parsed (include/hyobfs_gecko.h), 16 bytes each
FRAME_DTYPE = np.dtype([("chunk_off", "<u8"), ("chunk_len", "<u4"), ("pad_len", "<u2"), ("msg_id", "u1"),
                        ("idx_total", "u1")])
PARSED_DTYPE = np.dtype([("status", "<i4"), ("pad_len", "<u2"), ("msg_id", "u1"), ("idx_total", "u1"),
                         ("payload_off", "<u4"), ("payload_len", "<u4")])
# include/hyobfs_gecko.h status codes by the oracle's classes
PARSE_STATUS = {gref.PASS: 0, gref.FRAGMENT: 1, gref.EMPTY: -22, gref.TRUNCATED: -20, gref.INVALID: -21}


# ------------------------------------------------------------------ realm punch
PUNCH_PADDINGS = (0, 1, 31, 32, 33, 1023, 1024)
PUNCH_BAD_TYPES = (0x00, 0x03, 0x81, 0xFF)
PUNCH_ABSENT_LENGTHS = (0, 8, 32, 1058, 1059, 2048, 65536)   # out of range: no bytes behind them
PUNCH_PREFIXES = (1, 255, 256, 257)


def _punch_raw(ptype, nonce, key, salt, padding):
    """A punch packet with any type byte (rref.encode refuses unknown types)."""
    plain = rref.MAGIC + bytes([ptype]) + bytes(nonce) + bytes(padding)
    m = rref.mask(key, salt)
    return bytes(salt) + bytes(b ^ m[i % 32] for i, b in enumerate(plain))


@functools.lru_cache(maxsize=None)
def punch_lattice():
    """dict(attempts [(nonce, key)], buf, off, len, real, exp [(match, type, padding)], labels).

    Attempts: A0 = (k0, n0), A1 = (k0, n1) shares A0's key, A2 = A1 (a duplicate: the
    lowest index wins), A3 = (k1, n0) shares A0's nonce, A4 random.  Entries come in
    shuffled order; the datagrams lie in another shuffled order with gaps of 0..7
    bytes, and two entries alias one datagram."""
    rng = random.Random(20)
    k0, k1, n0, n1 = rng.randbytes(32), rng.randbytes(32), rng.randbytes(16), rng.randbytes(16)
    atts = [(n0, k0), (n1, k0), (n1, k0), (n0, k1), (rng.randbytes(16), rng.randbytes(32))]
    ent = []   # (label, packet bytes, or an int: the length of a datagram that does not exist)
    for j, (nonce, key) in enumerate(atts):
        for t in (rref.HELLO, rref.ACK):
            for pad in PUNCH_PADDINGS:
                ent.append(("A%d t%d pad%d" % (j, t, pad), rref.encode(t, nonce, key, rng.randbytes(8), rng.randbytes(pad))))
    for pad in (0, 40):   # decodes under A0's and A1's key, fails both nonces
        ent.append(("k0 other nonce pad%d" % pad, rref.encode(rref.ACK, rng.randbytes(16), k0, rng.randbytes(8),
                                                               rng.randbytes(pad))))
    for t in PUNCH_BAD_TYPES:
        for nonce, key in (atts[0], atts[3]):
            ent.append(("type %#x" % t, _punch_raw(t, nonce, key, rng.randbytes(8), rng.randbytes(5))))
    base = rref.encode(rref.HELLO, n1, k0, rng.randbytes(8), rng.randbytes(31))
    for bit in range(8 * rref.MIN_WIRE):
        p = bytearray(base)
        p[bit >> 3] ^= 1 << (bit & 7)
        ent.append(("flip bit %d" % bit, bytes(p)))
    for pad in (1, 33, 1024):   # only the first 25 plain bytes decide
        for where in (0, pad - 1):
            p = bytearray(rref.encode(rref.ACK, n0, k1, rng.randbytes(8), rng.randbytes(pad)))
            p[rref.MIN_WIRE + where] ^= 0xFF
            ent.append(("pad%d byte %d corrupted" % (pad, where), bytes(p)))
    for wire in (rref.MIN_WIRE, rref.MAX_WIRE):
        ent.append(("wire %d" % wire, rref.encode(rref.HELLO, *atts[4], rng.randbytes(8), rng.randbytes(wire - rref.MIN_WIRE))))
    for wire in PUNCH_ABSENT_LENGTHS:
        ent.append(("absent %d" % wire, wire))
    rng.shuffle(ent)
    # the datagrams, placed in another order
    place = [i for i, e in enumerate(ent) if not isinstance(e[1], int)]
    rng.shuffle(place)
    off = np.zeros(len(ent) + 2, np.uint64)
    buf = bytearray()
    for i in place:
        buf += bytes([SENTINEL]) * rng.randrange(8)
        off[i] = len(buf)
        buf += ent[i][1]
    real = [not isinstance(e[1], int) for e in ent] + [True, True]
    for i, e in enumerate(ent):
        if isinstance(e[1], int):
            off[i] = len(buf)
    # two more entries alias earlier datagrams (a hit and a miss)
    hit = next(i for i, e in enumerate(ent) if e[0] == "A2 t2 pad33")
    miss = next(i for i, e in enumerate(ent) if e[0] == "flip bit 70")
    ent += [("alias of %d" % hit, ent[hit][1]), ("alias of %d" % miss, ent[miss][1])]
    off[-2:] = off[hit], off[miss]
    ln = np.array([e[1] if isinstance(e[1], int) else len(e[1]) for e in ent], np.uint32)
    exp = [rref.match(bytes(e[1]) if isinstance(e[1], int) else e[1], atts) for e in ent]
    by = dict(zip((e[0] for e in ent), exp))
    for j in range(5):   # a packet under the duplicate A2 reports index 1
        assert all(by["A%d t%d pad%d" % (j, t, p)] == ((1 if j == 2 else j), t, p) for t in (1, 2) for p in PUNCH_PADDINGS)
    assert all(x == (-1, 0, 0) for lbl, x in by.items() if lbl.startswith(("k0 other", "type ", "flip bit", "absent")))
    assert all(x[0] == 3 for lbl, x in by.items() if "corrupted" in lbl)
    assert by["wire 33"] == (4, 1, 0) and by["wire 1057"] == (4, 1, 1024)
    assert sorted(off[np.array(real)].tolist()) != off[np.array(real)].tolist() and len(buf) < 60_000
    assert len(ent) > max(PUNCH_PREFIXES)
    return dict(attempts=atts, buf=np.frombuffer(bytes(buf), np.uint8).copy(), off=off, len=ln,
                real=np.array(real, np.uint8), exp=exp, labels=[e[0] for e in ent])


def attempts_bytes(atts):
    """hyobfs_punch_attempt records: nonce(16) || key(32)."""
    return b"".join(bytes(n) + bytes(k) for n, k in atts)


def punch_runs():
    """(name, n, m, null_out) of every run over the lattice: the whole of it, its first
    n entries, no attempts at all (`attempts` null), and `type` / `padding` null."""
    n = len(punch_lattice()["len"])
    return ([("all", n, 5, False), ("null_outputs", n, 5, True), ("no_attempts", n, 0, False)]
            + [("first_%d" % k, k, 5, False) for k in PUNCH_PREFIXES])


def punch_expected(n, m):
    lat = punch_lattice()
    return [e if m else (-1, 0, 0) for e in lat["exp"][:n]]


# ------------------------------------------------------------------ Gecko parse
def _parse_pads(ln):
    """Around the padding check (5 + pad > len), and the u16's byte boundaries."""
    return sorted({0, max(ln - 6, 0), max(ln - 5, 0), (ln - 4) & 0xFFFF, 0x00FF, 0x0100, 0xFFFF})


def parse_record(datagram):
    """The six fields of hyobfs_gecko_parsed for one datagram, from oracle/gecko_ref.py."""
    kind, h, payload = gref.parse(datagram)
    if kind == gref.PASS:
        return PARSE_STATUS[kind], 0, 0, 0, 0, len(datagram)
    if kind != gref.FRAGMENT:
        return PARSE_STATUS[kind], 0, 0, 0, 0, 0
    off = gref.HEADER_LEN + h.pad_len
    assert datagram[off:] == payload
    return PARSE_STATUS[kind], h.pad_len, h.msg_id, h.chunk_idx << 4 | h.total_chunks, off, len(datagram) - off


@functools.lru_cache(maxsize=None)
def parse_lattice():
    """dict(buf, off, len, exp [PARSED_DTYPE], counts): len 0..8 x first byte x every
    idx_total x pad lengths around the checks, plus two 2040-byte datagrams.  Each
    datagram ends on an 8-byte boundary with at least 8 unused bytes before the next
    one starts, so the CPU tier can poison every byte after a datagram's last; an
    empty datagram points at the end of the buffer, which ends with the last datagram."""
    grams = []
    for ln in range(9):
        for first in (0x00, 0x7F, 0x80, 0xFF):
            for it in range(256):
                for pad in _parse_pads(ln):
                    d = bytes([first, (it * 7 + ln + 1) & 0xFF, it, pad >> 8, pad & 0xFF, 0xC1, 0xC2, 0xC3])[:ln]
                    grams.append(d)
    for pad in (2040 - 5, 2040 - 4):
        grams.append(bytes([0x80, 0x5A, 0x12, pad >> 8, pad & 0xFF]) + bytes(2035))
    random.Random(21).shuffle(grams)
    grams.append(bytes([0x80, 0x11]))   # the buffer ends after a datagram shorter than the header
    off = np.zeros(len(grams), np.uint64)
    buf = bytearray()
    for i, d in enumerate(grams):
        if d:
            buf += bytes([SENTINEL]) * (8 + -len(d) % 8)
            off[i] = len(buf)
            buf += d
    off[[i for i, d in enumerate(grams) if not d]] = len(buf)
    exp = np.array([parse_record(d) for d in grams], dtype=PARSED_DTYPE)
    counts = {k: int((exp["status"] == v).sum()) for k, v in PARSE_STATUS.items()}
    assert min(counts.values()) >= 100, counts
    assert len(buf) % 8 == 0 and all(int(o) + len(d) <= len(buf) for o, d in zip(off, grams))
    return dict(buf=np.frombuffer(bytes(buf), np.uint8).copy(), off=off,
                len=np.array([len(d) for d in grams], np.uint32), exp=exp, counts=counts)


# ------------------------------------------------------------------ Gecko encode
PAD_KEY, PAD_NONCE = bytes(range(7, 39)), bytes(range(100, 112))
IMPOSSIBLE = (0x00, 0x01, 0x09, 0x22, 0x88, 0x0F, 0xF2)   # idx_total no encodeFrame call accepts
ENCODE_MODES = ("tiny", "big", "limit")
ENCODE_NS = (1, 63, 64, 65, 130, 257)
ENCODE_ORDERS = ("ascending", "shuffled")
PSK_LENGTHS = (4, 16, 121, 300)


def psk_of(n):
    return bytes((7 * i + n) & 0xFF for i in range(n))


def frame_wire(psk, msg, fr, salt, out_off):
    """The wire datagram of one frame record, or None where the device skips it: a
    frame encodeFrame refuses, or one longer than the reference's buffer."""
    off, clen, plen, mid, it = (int(x) for x in fr)
    h = gref.Header(pad_len=plen, msg_id=mid, chunk_idx=it >> 4, total_chunks=it & 0x0F)
    try:
        plain = gref.encode_frame(h, msg[off:off + clen], gref.pad_bytes(PAD_KEY, PAD_NONCE, int(out_off), plen))
    except gref.FrameError:
        return None
    if sref.SM_SALT_LEN + len(plain) > gref.BUFFER_SIZE:
        return None
    return sref.obfuscate(psk, plain, int(salt).to_bytes(8, "little"))


def _frames(rng, mode, n, msg_len, skip_first):
    """n frame records: every chunk inside msg, half of them ending at its last byte."""
    fr = np.zeros(n, FRAME_DTYPE)
    bad = set(rng.choice(n, int(round(0.15 * n)), replace=False).tolist())
    if skip_first:
        bad.add(0)
    over = set(rng.choice(n, n // 10, replace=False).tolist()) if mode == "limit" else set()
    for i in range(n):
        if mode == "tiny":
            clen, pad = int(rng.integers(0, 20)), int(rng.choice([0, 1, 2, 3, 17, 40]))
        elif mode == "big":
            clen, pad = int(rng.integers(0, 1500)), int(rng.integers(0, 600))
        else:   # wire datagrams of 2046..2048 bytes, and 2049 / 2050: skipped
            wire = int(rng.choice([2049, 2050])) if i in over else int(rng.choice([2046, 2047, 2048]))
            pad = int(rng.integers(0, 600))
            clen = wire - 13 - pad
        kind = 0 if i == n - 1 else rng.integers(0, 10)
        coff = msg_len - clen if kind < 5 else 0 if kind == 5 else int(rng.integers(0, msg_len - clen + 1))
        total = int(rng.integers(2, 9))
        it = int(rng.choice(IMPOSSIBLE)) if i in bad else int(rng.integers(0, total)) << 4 | total
        fr[i] = (coff, clen, pad, int(rng.integers(0, 256)), it)
    return fr


def _place(rng, widths, order, start=0):
    """out_off of each frame: slots of the wire lengths, gaps of 0..40 bytes before
    half of them, in ascending order or placed in a shuffled order."""
    n = len(widths)
    seq = rng.permutation(n) if order == "shuffled" else np.arange(n)
    gaps = np.where(rng.integers(0, 2, n) == 1, rng.integers(0, 41, n), 0)
    off = np.zeros(n, np.uint64)
    cur = start
    for i in seq:
        cur += int(gaps[i])
        off[i] = cur
        cur += int(widths[i])
    return off, cur


def _encode_case(name, mode, n, order, psk_len, seed, skip_first):
    rng = np.random.default_rng(seed)
    msg_len = 64 if mode == "tiny" else 4096
    msg = rng.integers(0, 256, msg_len, dtype=np.uint8)
    fr = _frames(rng, mode, n, msg_len, skip_first)
    widths = 13 + fr["pad_len"].astype(np.int64) + fr["chunk_len"].astype(np.int64)
    off, total = _place(rng, widths, order)
    salts = sref.splitmix64_array(seed, 0, n)
    psk = psk_of(psk_len)
    exp = np.full(total, SENTINEL, np.uint8)
    mb = msg.tobytes()
    valid = 0
    for i in range(n):
        w = frame_wire(psk, mb, fr[i], salts[i], off[i])
        if w is not None:
            assert len(w) == widths[i]
            exp[int(off[i]):int(off[i]) + len(w)] = np.frombuffer(w, np.uint8)
            valid += 1
    first_valid = frame_wire(psk, mb, fr[0], salts[0], off[0]) is not None
    return dict(name=name, mode=mode, n=n, order=order, psk=psk, msg=msg, frames=fr, salts=salts, off=off,
                out_len=total, exp=exp, valid=valid, first_skipped=not first_valid)


@functools.lru_cache(maxsize=None)
def encode_cases():
    """Mode x n x placement, the PSK lengths (one kernel instantiation per salt word)
    rotating so that each mode and placement meets all four."""
    cases = []
    for a, mode in enumerate(ENCODE_MODES):
        for b, n in enumerate(ENCODE_NS):
            for c, order in enumerate(ENCODE_ORDERS):
                k = len(cases)
                psk_len = PSK_LENGTHS[(a + b + 2 * c) % 4]
                cases.append(_encode_case("%s-%d-%s-psk%d" % (mode, n, order, psk_len), mode, n, order, psk_len,
                                          seed=100 + k, skip_first=(b + c) % 2 == 0))
    for cs in cases:
        if cs["n"] >= 63:
            assert cs["n"] - cs["valid"] >= 1 and cs["valid"] >= 40, (cs["name"], cs["valid"])
    assert any(cs["n"] >= 64 and cs["first_skipped"] and cs["order"] == "ascending" for cs in cases)
    assert any(cs["n"] >= 64 and not cs["first_skipped"] for cs in cases)
    for mode in ENCODE_MODES:
        for order in ENCODE_ORDERS:
            assert {len(cs["psk"]) for cs in cases if (cs["mode"], cs["order"]) == (mode, order)} == set(PSK_LENGTHS)
    assert any((cs["frames"]["chunk_len"] == 0).any() for cs in cases)
    return cases


# ------------------------------------------------------------------ far offsets
def _windows(segments, lo, hi):
    """[(start, expected bytes)]: the segments with GUARD sentinel bytes on either
    side, overlapping windows merged, clipped to [lo, hi)."""
    spans = []
    for s, w in sorted(segments):
        a, b = max(s - GUARD, lo), min(s + len(w) + GUARD, hi)
        if spans and a <= spans[-1][1]:
            spans[-1][1] = max(spans[-1][1], b)
        else:
            spans.append([a, b])
    out = []
    for a, b in spans:
        e = np.full(b - a, SENTINEL, np.uint8)
        for s, w in segments:
            if a <= s < b:
                e[s - a:s - a + len(w)] = np.frombuffer(w, np.uint8)
        out.append((a, e))
    return out


def _far_case(name, seed, n, order, start, lo, hi, jump=None, small=False):
    """n frames (every eighth skipped) from `start`; `jump`: extra bytes between the
    two halves of an ascending group.  [lo, hi) is the part of `out` that exists."""
    rng = np.random.default_rng(seed)
    msg = rng.integers(0, 256, 1024, dtype=np.uint8)
    fr = np.zeros(n, FRAME_DTYPE)
    for i in range(n):
        clen, pad = (int(rng.integers(0, 16)), int(rng.integers(0, 20))) if small else \
            (int(rng.integers(0, 700)), int(rng.integers(1, 300)))
        total = int(rng.integers(2, 9))
        it = 0x22 if i % 8 == 3 else int(rng.integers(0, total)) << 4 | total
        fr[i] = (1024 - clen if i % 2 else int(rng.integers(0, 1024 - clen + 1)), clen, pad, i, it)
    widths = 13 + fr["pad_len"].astype(np.int64) + fr["chunk_len"].astype(np.int64)
    off, end = _place(rng, widths, order, start)
    if jump is not None:
        off[n // 2:] += np.uint64(jump)
        end += jump
    salts = sref.splitmix64_array(seed, 0, n)
    psk = psk_of(16)
    segs = []
    for i in range(n):
        w = frame_wire(psk, msg.tobytes(), fr[i], salts[i], off[i])
        if w is not None:
            segs.append((int(off[i]), w))
    assert lo <= min(s for s, _ in segs) and max(s + len(w) for s, w in segs) <= hi, name
    return dict(name=name, psk=psk, msg=msg, frames=fr, salts=salts, off=off, lo=lo, hi=hi,
                windows=_windows(segs, lo, hi), first=min(s for s, _ in segs), end=max(s + len(w) for s, w in segs))


@functools.lru_cache(maxsize=None)
def far_cases():
    """Frames straddling out_off = 2^32 and 2^38 (the pad keystream's block index
    passes 32 bits there), and ascending 40-frame groups whose wire span stays just
    under 2^31 (the aligned sweep), reaches it, or passes 2^32 (the window path)."""
    K64 = 64 << 10
    cases = {}
    for bits in (32, 38):
        for order in ENCODE_ORDERS:
            e = 1 << bits
            name = "straddle%d_%s" % (bits, order)
            cs = _far_case(name, 200 + bits + len(order), 40, order, e - 10_000, e - K64, e + K64)
            # frames (each with padding) on both sides of the edge: the block index's high word changes
            assert cs["first"] < e - 5_000 and cs["end"] > e + 2_000
            cases[name] = cs
    for name, jump, hi in (("span31_aligned", (1 << 31) - 2000, (1 << 31) + K64),
                           ("span31_window", (1 << 31) + 5, (1 << 31) + K64),
                           ("span32_window", (1 << 32) + 5, (1 << 32) + K64),
                           # the aligned sweep across a gap short enough for the CPU tier's emulated lanes
                           ("span24_aligned", 1 << 24, (1 << 24) + K64)):
        cs = _far_case(name, 300 + len(cases), 40, "ascending", 300, 0, hi, jump=jump, small=True)
        span = cs["end"] - (cs["first"] & ~255)
        assert (span < 1 << 31) == name.endswith("_aligned"), (name, span)   # gecko.hip: `aligned`
        assert 0x22 != int(cs["frames"]["idx_total"][0]) and cs["end"] - jump < 4000
        cases[name] = cs
    return cases


# ------------------------------------------------------------------ the CPU tier's case file
def _u32(*v):
    return struct.pack("<%dI" % len(v), *v)


def _u64(*v):
    return struct.pack("<%dQ" % len(v), *v)


def punch_section(n, m, null_out):
    """tests/emu/wire_main.cpp, section 1."""
    lat = punch_lattice()
    return b"".join([_u32(1, m, int(null_out)), _u64(n, len(lat["buf"]), len(lat["len"])),
                     attempts_bytes(lat["attempts"][:m]), lat["off"].tobytes(), lat["len"].tobytes(),
                     lat["real"].tobytes(), lat["buf"].tobytes()])


def parse_section():
    """Section 2."""
    lat = parse_lattice()
    return b"".join([_u32(2), _u64(len(lat["len"]), len(lat["buf"])), lat["off"].tobytes(), lat["len"].tobytes(),
                     lat["buf"].tobytes(), lat["exp"].tobytes()])


def _encode_head(tag, cs):
    return b"".join([_u32(tag, len(cs["psk"])), cs["psk"], _u64(len(cs["frames"]), len(cs["msg"])), PAD_KEY, PAD_NONCE,
                     cs["frames"].tobytes(), cs["salts"].tobytes(), cs["off"].tobytes(), cs["msg"].tobytes()])


def encode_section(cs):
    """Section 3: the whole expected `out`."""
    return _encode_head(3, cs) + _u64(cs["out_len"]) + cs["exp"].tobytes()


def far_section(cs):
    """Section 4: `out` is a sparse mapping of [lo, hi); only the windows are compared."""
    return b"".join([_encode_head(4, cs), _u64(cs["lo"], cs["hi"] - cs["lo"], len(cs["windows"]))]
                    + [_u64(a, len(e)) + e.tobytes() for a, e in cs["windows"]])
