"""QUIC Initial unprotection cases shared by the CPU-emulated tier
(tests/emu/run_case.py quic) and the GPU tier (tests/test_gpu_quic.py).

Expected results come from oracle/quic_ref.py, which tests/test_quic.py pins to
the reference's own vectors (packet_protector_test.go:15-77).
"""
import functools
import re

import numpy as np

from oracle import quic_ref as ref

# packet_protector_test.go:17-31 (draft-ietf-quic-tls-32 A.3, server Initial)
_h = lambda s: bytes.fromhex(re.sub(r"\s", "", s))  # noqa: E731
AES_PROTECTED = _h("""c7ff0000200008f067a5502a4262b500 4075fb12ff07823a5d24534d906ce4c7
    6782a2167e3479c0f7f6395dc2c91676 302fe6d70bb7cbeb117b4ddb7d173498
    44fd61dae200b8338e1b932976b61d91 e64a02e9e0ee72e3a6f63aba4ceeeec5
    be2f24f2d86027572943533846caa13e 6f163fb257473d0eda5047360fd4a47e
    fd8142fafc0f76""")
AES_PLAIN = _h("""02000000000600405a020000560303ee fce7f7b37ba1d1632e96677825ddf739
    88cfc79825df566dc5430b9a045a1200 130100002e00330024001d00209d3c94
    0d89690b84d08a60993c144eca684d10 81287c834d5311bcf32bb9da1a002b00
    020304""")
AES_CONN_ID = _h("8394c8f03e515708")
# packet_protector_test.go:57-61 (draft-ietf-quic-tls-32 A.5, ChaCha20 short header)
CHACHA_PROTECTED = _h("4cfe4189655e5cd55c41f69080575d7999c25a5bfb")
CHACHA_PLAIN = _h("01")
CHACHA_HDR = _h("4200bff4")
CHACHA_SECRET = _h("9ac312a7f877468ebe69422748ad00a15443f18203a07d6060f688f30f21632b")
CHACHA_PN_MAX = 654360564

STATUS = {
    "EOF": -40, "not a QUIC packet": -41, "unsupported version": -42, "invalid packet": -43,
    "packet is too short": -44, "packet with long header is too small": -45,
    "packet too small for the header protection sample": -45, "negative packet-number offset": -45, "message authentication failed": -46,
    "ciphertext shorter than the tag": -46, "encountered unexpected frame type": -47, "unexpected EOF": -48,
    "crypto frame data too large": -49, "unable to assemble crypto frames": -50,
}


def status_of(exc: Exception) -> int:
    msg = str(exc)
    if msg.startswith("encountered unexpected frame type"):
        msg = "encountered unexpected frame type"
    return STATUS[msg]


def oracle_read(packet: bytes):
    """(status, crypto data) by the oracle's ReadCryptoPayload."""
    try:
        return 0, ref.read_crypto_payload(packet)
    except ref.QuicError as e:
        return status_of(e), b""


def oracle_unprotect(key, packet: bytes, pn_offset: int, pn_max: int):
    """(status, unmasked header, plaintext, pn)."""
    buf = bytearray(packet)
    try:
        hdr, plain, pn = ref.unprotect(key, buf, pn_offset, pn_max)
        return 0, hdr, plain, pn
    except ref.QuicError as e:
        return status_of(e), b"", b"", 0


def _crypto(off, data, n_off=None, n_len=None):
    return b"\x06" + ref.encode_varint(off, n_off) + ref.encode_varint(len(data), n_len) + data


def client_hello_like(rng, n):
    return b"\x01\x00" + n.to_bytes(2, "big") + rng.integers(0, 256, n, dtype=np.uint8).tobytes()


def frame_layouts(rng):
    """(name, frames payload) covering extractCryptoFrames / assembleCryptoFrames."""
    ch = client_hello_like(rng, 300)
    out = [
        ("single", _crypto(0, ch) + b"\x00" * 800),
        ("single_at_offset", _crypto(77, ch[:100]) + b"\x00" * 50),    # one frame: returned as is, offset ignored
        ("padding_first", b"\x00" * 200 + b"\x01" + _crypto(0, ch) + b"\x00" * 500),
        ("split_sorted", _crypto(0, ch[:100]) + _crypto(100, ch[100:]) + b"\x00" * 400),
        ("split_shuffled", _crypto(200, ch[200:]) + b"\x01\x00\x00" + _crypto(0, ch[:120]) + b"\x01" +
         _crypto(120, ch[120:200]) + b"\x00" * 333),
        ("nonminimal_varints", _crypto(0, ch[:50], 8, 4) + b"\x40\x00" + b"\x80\x00\x00\x01" +
         _crypto(50, ch[50:], 2, 2) + b"\x00" * 64),
        ("zero_prefix", _crypto(1000, ch[:40]) + _crypto(1040, ch[40:90])),   # assembled with 1000 zero bytes
        ("zero_len_frames", _crypto(0, b"") + _crypto(0, ch[:10]) + _crypto(10, b"") + _crypto(10, ch[10:30])),
        ("many_frames", b"".join(_crypto(5 * k, ch[5 * k:5 * k + 5]) for k in range(40)) + b"\x00" * 64),
        ("padding_tail_63", _crypto(0, ch[:70]) + b"\x00" * 63),
        ("padding_tail_64", _crypto(0, ch[:70]) + b"\x01" * 64),
        ("padding_tail_65", _crypto(0, ch[:70]) + b"\x00" * 65),
        # errors
        ("gap", _crypto(0, ch[:50]) + _crypto(60, ch[60:100]) + b"\x00" * 100),
        ("overlap", _crypto(0, ch[:50]) + _crypto(40, ch[40:100]) + b"\x00" * 100),
        ("no_crypto", b"\x01" + b"\x00" * 300),
        ("ack_frame", _crypto(0, ch[:50]) + b"\x02\x00\x00\x00\x00" + b"\x00" * 100),
        ("frame_eof_len", _crypto(0, ch[:50]) + b"\x06\x00"),
        ("frame_eof_data", _crypto(0, ch[:50]) + b"\x06\x00\x44\x00" + ch[:20]),
        ("frame_too_large", b"\x06\x00\x80\x04\x00\x01" + b"\x00" * 40),
        ("end_past_max_payload", _crypto(256 * 1024 - 10, ch[:5]) + _crypto(256 * 1024 - 5, ch[5:20])),
        ("offset_past_max_payload", _crypto(256 * 1024 + 1, ch[:3]) + _crypto(256 * 1024 + 4, ch[3:6])),
        ("single_far_offset", _crypto(1 << 40, ch[:33], 8)),   # one frame: no offset check at all
        ("too_many_frames", b"".join(_crypto(k, ch[k:k + 1]) for k in range(300))),
        ("type_varint_eof", _crypto(0, ch[:30]) + b"\x40"),
    ]
    return out


def crypto_packets(seed: int = 1):
    """A list of (name, packet bytes) of client Initials, good and bad."""
    rng = np.random.default_rng(seed)
    pkts = []
    layouts = frame_layouts(rng)
    for k, (name, frames) in enumerate(layouts):
        version = ref.V2 if k % 3 == 2 else ref.V1
        dl = [8, 0, 20, 1, 255, 18][k % 6]
        dcid = rng.integers(0, 256, dl, dtype=np.uint8).tobytes()
        scid = rng.integers(0, 256, k % 9, dtype=np.uint8).tobytes()
        token = rng.integers(0, 256, [0, 0, 33][k % 3], dtype=np.uint8).tobytes()
        pn_len = 1 + k % 4
        pkts.append((name, ref.client_initial(dcid, scid, version, token, 2, pn_len, frames)))
    ch = client_hello_like(rng, 200)
    good = _crypto(0, ch) + b"\x00" * 900
    dcid = bytes(range(8))
    base = ref.client_initial(dcid, b"", ref.V1, b"", 2, 4, good)
    tampered = bytearray(base)
    tampered[-1] ^= 1
    ct_flip = bytearray(base)
    ct_flip[60] ^= 0x80
    pkts += [
        ("v1_plain", base),
        ("coalesced_tail", ref.client_initial(dcid, b"", ref.V1, b"", 2, 4, good, tail=b"\xaa" * 50)),
        ("tag_tampered", bytes(tampered)),
        ("ct_tampered", bytes(ct_flip)),
        ("draft29_version", ref.client_initial(dcid, b"", 0xFF00001D, b"", 2, 4, good)),
        ("version_zero", bytes([0x80]) + b"\0\0\0\0" + b"\x08" + dcid + b"\x00\x00\x05" + b"\0" * 30),
        ("not_quic", bytes([0x80]) + b"\0\0\0\1" + b"\x08" + dcid + b"\x00" * 40),
        ("length_past_end", ref.client_initial(dcid, b"", ref.V1, b"", 2, 4, good, length_override=5000)),
        ("length_zero", base[:base.index(dcid) + 9 + 1] + b"\x40\x00" + base[base.index(dcid) + 12:]),
        ("length_tiny", ref.client_initial(dcid, b"", ref.V1, b"", 2, 1, good, length_override=12)),
        ("truncated_4", base[:4]),
        ("truncated_dcid", base[:9]),
        ("truncated_scid_len", base[:14]),
        ("truncated_token_len", base[:15]),
        ("truncated_length", base[:17]),
        ("empty", b""),
        ("short_header_bit", bytes([base[0] & 0x7F]) + base[1:]),
        ("v2_long_dcid", ref.client_initial(bytes(range(20)) * 2, b"abc", ref.V2, b"tok" * 20, 2, 2, good)),
    ]
    return pkts


def unprotect_cases(seed: int = 2):
    """(name, key, packet, pn_offset, pn_max) for UnProtect with explicit keys,
    both suites, long and short headers, several packet-number windows."""
    rng = np.random.default_rng(seed)
    cases = []
    aes_key = ref.initial_protection_key(ref.initial_secret(AES_CONN_ID, 0xFF000020, True), 0xFF000020)
    cases.append(("ref_aes_server_initial", aes_key, AES_PROTECTED, 18, 1))
    cc_key = ref.ProtectionKey(ref.TLS_CHACHA20_POLY1305_SHA256, CHACHA_SECRET, ref.V1)
    cases.append(("ref_chacha_short_header", cc_key, CHACHA_PROTECTED, 1, CHACHA_PN_MAX))
    for k in range(24):
        suite = ref.TLS_AES_128_GCM_SHA256 if k % 2 == 0 else ref.TLS_CHACHA20_POLY1305_SHA256
        version = [ref.V1, ref.V2, 0xFF00001D][k % 3]
        key = ref.ProtectionKey(suite, rng.integers(0, 256, 32, dtype=np.uint8).tobytes(), version)
        pn_len = 1 + (k // 2) % 4
        long_hdr = k % 4 < 2
        plen = [0, 1, 15, 16, 17, 63, 64, 65, 700, 1150, 2047, 4100][k % 12]
        payload = rng.integers(0, 256, plen, dtype=np.uint8).tobytes()
        pn_max = int(rng.integers(0, 1 << 40))
        pn = pn_max + 1 + int(rng.integers(-(1 << (8 * pn_len - 2)), 1 << (8 * pn_len - 2)))
        pn = max(pn, 0)
        if long_hdr:
            first = 0xC0 | (pn_len - 1)
            pre = bytes([first]) + struct_be(version) + b"\x04abcd\x00" + b"\x00" + ref.encode_varint(
                pn_len + plen + 16, 2)
        else:
            first = 0x40 | (pn_len - 1)
            pre = bytes([first]) + rng.integers(0, 256, 8, dtype=np.uint8).tobytes()
        hdr = pre + (pn & ((1 << (8 * pn_len)) - 1)).to_bytes(pn_len, "big")
        if len(hdr) + plen + 16 < len(pre) + 20:   # pad the payload so the sample fits
            payload += bytes(len(pre) + 20 - len(hdr) - plen - 16)
        pkt = ref.protect(key, hdr, len(pre), pn, payload)
        cases.append((f"rand{k}", key, pkt, len(pre), pn_max))
    # errors: too small for the sample, tampered tag, negative offset
    key = cases[2][1]
    pkt = cases[2][2]
    bad = bytearray(pkt)
    bad[-3] ^= 0x10
    cases += [("tag_flip", key, bytes(bad), cases[2][3], cases[2][4]),
              ("too_small", key, pkt[:cases[2][3] + 19], cases[2][3], 0),
              ("neg_offset", key, pkt, -1, 0),
              ("offset_past_end", key, pkt, len(pkt) + 3, 0)]
    return cases


def struct_be(v: int) -> bytes:
    return v.to_bytes(4, "big")


def key_record(key) -> bytes:
    """oracle ProtectionKey -> struct hyobfs_quic_key bytes (80)."""
    k = key.key + bytes(32 - len(key.key))
    hp = key.hp + bytes(32 - len(key.hp))
    return key.suite.to_bytes(4, "little") + key.iv + k + hp


def pack(packets):
    lens = np.array([len(p) for p in packets], np.uint32)
    off = np.zeros(len(packets), np.uint64)
    if len(packets) > 1:
        np.cumsum(lens[:-1], out=off[1:])
    buf = np.frombuffer(b"".join(packets) + bytes(64), np.uint8).copy()
    return buf, off, lens


def check_unprotect(cases, buf, off, res):
    """Compare device results (in-place buffer + RESULT_DTYPE records) with the oracle."""
    for i, (name, key, pkt, pn_offset, pn_max) in enumerate(cases):
        st, hdr, plain, pn = oracle_unprotect(key, pkt, pn_offset, pn_max)
        r = res[i]
        assert int(r["status"]) == st, (name, int(r["status"]), st)
        if st:
            continue
        o = int(off[i])
        got_hdr = buf[o:o + int(r["hdr_len"])].tobytes()
        got = buf[o + int(r["hdr_len"]):o + int(r["hdr_len"]) + int(r["plain_len"])].tobytes()
        assert (got_hdr, got, int(r["pn"])) == (hdr, plain, pn), name


def check_crypto(pkts, out, out_off, caps, res):
    """Device ReadCryptoPayload results vs the oracle.  Two device limits with no
    reference counterpart: more than 256 CRYPTO frames (-52) and assembled data
    larger than the caller's out_cap (-51, out_len = the size needed)."""
    for i, (name, pkt) in enumerate(pkts):
        st, data = oracle_read(pkt)
        r = res[i]
        if st == 0 and name == "too_many_frames":
            st = -52
        if st == 0 and len(data) > int(caps[i]):
            assert int(r["status"]) == -51 and int(r["out_len"]) == len(data), name
            continue
        assert int(r["status"]) == st, (name, int(r["status"]), st)
        if st == 0:
            o = int(out_off[i])
            assert int(r["out_len"]) == len(data), (name, int(r["out_len"]), len(data))
            assert out[o:o + len(data)].tobytes() == data, name


# ------------------------------------------------------------------ edge lattices
# The builders below aim at the places where quic_open_kernel changes path: the
# 64-lane split of the tag polynomial, the lane-strided frame loops, the 64-byte
# parse window, the SHA-256 padding of the key schedule and the three returns of
# decodePacketNumber.  The checkers compare whole buffers, so bytes the kernel
# must leave alone (tag, neighbours, out past out_len) are covered as well.
SENTINEL = 0xA5
GAP = 7
AES = ref.TLS_AES_128_GCM_SHA256
CHACHA = ref.TLS_CHACHA20_POLY1305_SHA256
LANE_SPLIT_M = (62, 63, 64, 65, 66, 126, 127, 128, 129, 130, 192, 193)


class RawKey:
    """Key material with any suite id: a record ProtectionKey refuses to make."""

    def __init__(self, suite, iv, key, hp):
        self.suite, self.iv, self.key, self.hp = suite, iv, key, hp


def _rbytes(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


def _sealed(rng, key, version, long_hdr, pn_len, pn, payload):
    """(packet, pn_offset): `payload` sealed under `pn` behind a 14-byte long
    header prefix or a 9-byte short one."""
    if long_hdr:
        pre = (bytes([0xC0 | (pn_len - 1)]) + struct_be(version) + b"\x04abcd\x00" + b"\x00"
               + ref.encode_varint(pn_len + len(payload) + 16, 2))
    else:
        pre = bytes([0x40 | (pn_len - 1)]) + _rbytes(rng, 8)
    hdr = pre + (pn & ((1 << (8 * pn_len)) - 1)).to_bytes(pn_len, "big")
    return ref.protect(key, hdr, len(pre), pn, payload), len(pre)


@functools.lru_cache(maxsize=None)
def _lane_split_cases():
    rng = np.random.default_rng(21)
    cases = []
    k = 0
    for suite in (AES, CHACHA):
        for m in LANE_SPLIT_M:
            for long_hdr, pn_len in ((True, 1), (True, 4), (False, 2), (False, 3)):
                hdr_len = (14 if long_hdr else 9) + pn_len
                for short in (0, 1, 15):
                    ct_len = 16 * (m - 1 - (hdr_len + 15) // 16) - short
                    version = ref.V2 if k % 2 else ref.V1
                    key = ref.ProtectionKey(suite, _rbytes(rng, 32), version)
                    pn_max = int(rng.integers(0, 1 << 40))
                    pn = pn_max + 1 + int(rng.integers(-(1 << (8 * pn_len - 2)), 1 << (8 * pn_len - 2)))
                    pkt, pn_off = _sealed(rng, key, version, long_hdr, pn_len, pn, _rbytes(rng, ct_len))
                    name = f"{suite:x}_m{m}_{'long' if long_hdr else 'short'}{pn_len}_short{short}"
                    cases.append((name, key, pkt, pn_off, pn_max))
                    if k % 7 == 3:
                        bad = bytearray(pkt)
                        bad[len(pkt) - 16 + k % 16] ^= 1 << (k % 8)
                        cases.append((name + "_tagflip", key, bytes(bad), pn_off, pn_max))
                        bad = bytearray(pkt)
                        bad[hdr_len + (k * 131) % ct_len] ^= 0x80 >> (k % 8)
                        cases.append((name + "_ctflip", key, bytes(bad), pn_off, pn_max))
                    k += 1
    return tuple(cases)


def lane_split_cases():
    """(name, key, packet, pn_offset, pn_max) with m = ceil(hdr_len/16) +
    ceil(ct_len/16) + 1 tag-polynomial blocks at the edges of the 64-lane split
    (lane 63 idle / one block per lane / lane 0 takes two, and the same one and
    two trips later), for each suite x header shape x fill of the last block;
    every 7th case has a tag-flipped and a ciphertext-flipped twin."""
    return list(_lane_split_cases())


def lane_split_m(case):
    """m of a case, from the oracle's view of the packet (None if too small)."""
    st, hdr_len, _, _, _ = expected_unprotect(*case[1:])
    if st not in (0, -46):
        return None
    return (hdr_len + 15) // 16 + (len(case[2]) - hdr_len - 16 + 15) // 16 + 1


def _pn_lattice(pn_len):
    win = 1 << (8 * pn_len)
    h = win // 2
    top = 1 << 62
    maxes = [-1, 0, 1, h - 2, h - 1, h, win - 2, win - 1, win, win + h - 1, 3 * win + h, (1 << 32) - 1, 1 << 32,
             top - win - 2, top - win - 1, top - win, top - 2, top - 1]
    for pn_max in sorted(set(maxes)):
        e = pn_max + 1
        truncs = [0, 1, h - 1, h, h + 1, win - 1, (e + h) % win, (e - h) % win, (e + h + 1) % win,
                  (e - h + 1) % win, e % win]
        for trunc in sorted(set(truncs)):
            yield pn_max, trunc


@functools.lru_cache(maxsize=None)
def _pn_decode_cases():
    rng = np.random.default_rng(22)
    cases = []
    for pn_len in (1, 2, 3, 4):
        for pn_max, trunc in _pn_lattice(pn_len):
            pn = ref.decode_packet_number(pn_max, trunc, pn_len)
            if pn < 0:
                continue
            suite = CHACHA if len(cases) % 2 else AES
            key = ref.ProtectionKey(suite, _rbytes(rng, 32), ref.V1)
            pkt, pn_off = _sealed(rng, key, ref.V1, False, pn_len, pn, _rbytes(rng, 8))
            cases.append((f"pn{pn_len}_max{pn_max:x}_t{trunc:x}", key, pkt, pn_off, pn_max))
    return tuple(cases)


def pn_decode_cases():
    """Short-header packets sealed under decodePacketNumber(pn_max, trunc, pn_len)
    of the oracle, over the half-window edges of each pn_len, pn_max = -1 and the
    2^62 - win guard: authentication passes exactly when the device decodes the
    same packet number."""
    return list(_pn_decode_cases())


def pn_decode_branch(case):
    """Which return of decodePacketNumber a case takes: +1 (candidate + win),
    -1 (candidate - win) or 0."""
    _, key, pkt, pn_off, pn_max = case
    st, hdr_len, _, pn, want = expected_unprotect(key, pkt, pn_off, pn_max)
    assert st == 0
    win = 1 << (8 * (hdr_len - pn_off))
    candidate = ((pn_max + 1) & ~(win - 1)) | int.from_bytes(want[pn_off:hdr_len], "big")
    return {win: 1, -win: -1, 0: 0}[pn - candidate]


def bad_suite_case(seed: int = 23):
    """A well-formed AES packet whose key record says TLS_AES_256_GCM_SHA384."""
    rng = np.random.default_rng(seed)
    key = ref.ProtectionKey(AES, _rbytes(rng, 32), ref.V1)
    pkt, pn_off = _sealed(rng, key, ref.V1, False, 2, 7, _rbytes(rng, 8))
    return ("suite_1302", RawKey(0x1302, key.iv, key.key, key.hp), pkt, pn_off, 6)


@functools.lru_cache(maxsize=None)
def _initial_edge_packets():
    rng = np.random.default_rng(24)
    ch = client_hello_like(rng, 1100)
    pkts = []

    def add(name, frames, dcid=None):
        k = len(pkts)
        dcid = _rbytes(rng, 8) if dcid is None else dcid
        version = ref.V2 if k % 2 else ref.V1
        token = _rbytes(rng, [0, 5][k % 2])
        pkts.append((name, ref.client_initial(dcid, _rbytes(rng, k % 5), version, token, 2, 1 + k % 4, frames)))

    # SHA-256 padding of the key schedule: dl + 9 crosses a 64-byte block at 55/56, ...
    for dl in (0, 1, 54, 55, 56, 57, 63, 64, 65, 118, 119, 120, 121, 127, 128, 183, 184, 247, 248, 255):
        add(f"dcid_{dl}", _crypto(0, ch[:60 + dl % 7]) + b"\x00" * (dl % 5), _rbytes(rng, dl))

    # lane-strided rank sort and gap check
    def three_byte_frames(count, r=None, shift=0):
        fs = [_crypto(3 * j + (shift if r is not None and j >= r else 0), ch[3 * j:3 * j + 3]) for j in range(count)]
        return b"".join(fs[j] for j in rng.permutation(count))

    for count in (2, 63, 64, 65, 127, 128, 129, 255, 256, 257):
        add(f"frames_{count}", three_byte_frames(count))
    for count, r in ((130, 1), (130, 63), (130, 64), (130, 65), (130, 127), (130, 128), (130, 129), (70, 64),
                     (65, 64)):
        add(f"gap_{count}_{r}", three_byte_frames(count, r, 1))
        add(f"overlap_{count}_{r}", three_byte_frames(count, r, -1))

    # PADDING / PING runs are skipped 64 bytes per ballot
    for run in list(range(5)) + list(range(60, 70)) + list(range(124, 133)) + [191, 192, 193, 700]:
        mix = bytes((j * 5 + run) % 3 == 0 for j in range(run))
        add(f"run_{run}", b"\x00" * run + _crypto(0, ch[:33]) + mix + _crypto(33, ch[33:70]) + b"\x00" * run)

    # a 17-byte frame head (type, 8-byte offset, 8-byte length) at every position
    # of the 64-byte window, then a frame type written as the varint 40 06
    for s in range(64):
        if s >= 3 and s % 2 == 0:   # the window was filled at 0 by a frame of s bytes ...
            pre, base = _crypto(0, ch[:s - 3]), s - 3
        else:                       # ... or by a run of padding
            pre, base = bytes(j % 4 == 1 for j in range(s)), 0
        n = 5 + s % 7
        body = _crypto(base, ch[base:base + n], 8, 8)
        tail = b"\x40" + _crypto(base + n, ch[base + n:base + n + 9])
        add(f"straddle_{s}", pre + body + tail + b"\x00" * (s % 3))

    for z in (1, 63, 64, 65, 1000):
        add(f"zero_prefix_{z}", _crypto(z, ch[:40]) + b"\x01" + _crypto(z + 40, ch[40:90]))
    return tuple(pkts)


def initial_edge_packets():
    """(name, packet) of client Initials at the edges inside the two kernels:
    DCID lengths around the SHA-256 padding, CRYPTO frame counts around the
    64-lane stride and HYOBFS_QUIC_MAX_FRAMES, a single gap or overlap at each
    lane edge, PADDING/PING runs around the 64-byte ballot, 8-byte varints at
    every alignment of the parse window, and zero prefixes."""
    return list(_initial_edge_packets())


# ------------------------------------------------------------------ grid-stride reuse
GRID_CAP = 1 << 20   # grid_for() in quic.hip: past this many packets a block takes a second one
SLOT = 64            # packet slot of the grid-stride batches; templates are at most SLOT - GAP bytes


def unprotect_templates(seed: int = 25):
    """(cases, classes): 96 packets of at most 57 bytes for the grid-stride batch,
    as unprotect_cases tuples, and a class per template: 0/1 AES / ChaCha OK,
    2/3 AES / ChaCha tag tampered, 4 too small for the sample, 5 unsupported suite."""
    rng = np.random.default_rng(seed)
    cases, classes = [], []

    def make(k, suite, long_hdr, pn_len, plen):
        version = ref.V2 if k % 3 == 1 else ref.V1
        key = ref.ProtectionKey(suite, _rbytes(rng, 32), version)
        pn_max = int(rng.integers(0, 1 << 30))
        pkt, pn_off = _sealed(rng, key, version, long_hdr, pn_len, pn_max + 1 + k % 3, _rbytes(rng, plen))
        assert len(pkt) <= SLOT - GAP
        return key, pkt, pn_off, pn_max

    for k in range(86):
        suite, long_hdr, pn_len = (AES, CHACHA)[k % 2], k // 2 % 2 == 0, 1 + k // 4 % 4
        lo, hi = max(4 - pn_len, 0), (27 if long_hdr else 32) - pn_len
        cases.append((f"t{k}",) + make(k, suite, long_hdr, pn_len, lo + k * 7 % (hi - lo + 1)))
        classes.append(k % 2)
    for k in range(4):
        key, pkt, pn_off, pn_max = make(k, (AES, CHACHA)[k % 2], k < 2, 2, 11 + k)
        bad = bytearray(pkt)
        bad[-1 - 5 * k] ^= 0x40
        cases.append((f"tagflip{k}", key, bytes(bad), pn_off, pn_max))
        classes.append(2 + k % 2)
    for k in range(3):
        key, pkt, pn_off, pn_max = make(k, (AES, CHACHA)[k % 2], k == 0, 1, 9)
        cases.append((f"too_small{k}", key, pkt[:pn_off + 19 - k], pn_off, pn_max))
        classes.append(4)
    for k in range(3):
        key, pkt, pn_off, pn_max = make(k, AES, k == 1, 3, 20)
        cases.append((f"suite{k}", RawKey((0x1302, 0x1304, 0)[k], key.iv, key.key, key.hp), pkt, pn_off, pn_max))
        classes.append(5)
    return cases, np.array(classes)


def initial_templates(seed: int = 26):
    """(packets, classes): 96 client Initials of at most 57 bytes (8-byte DCID, 1
    to 3 CRYPTO frames, some bad) for the grid-stride batch; the class tells the
    paths apart: status, and one frame / several frames among the good ones."""
    rng = np.random.default_rng(seed)
    pkts = []

    def add(name, frames, pn_len, version=None, flip=None):
        version = (ref.V2 if len(pkts) % 2 else ref.V1) if version is None else version
        pkt = bytearray(ref.client_initial(_rbytes(rng, 8), b"", version, b"", 2, pn_len, frames))
        if flip is not None:
            pkt[flip] ^= 0x04
        assert len(pkt) <= SLOT - GAP
        pkts.append((name, bytes(pkt)))

    for k in range(72):
        d = _rbytes(rng, 12)
        pn_len = 1 + k % 2
        nf = 1 + k % 3
        if nf == 1:
            frames = b"\x00" * (k % 5) + _crypto(k % 60, d[:3 + k % 9]) + b"\x01" * (k % 4)
        elif nf == 2:
            a = 1 + k % 7
            two = [_crypto(k % 40, d[:a]), _crypto(k % 40 + a, d[a:])]
            frames = two[k % 4 // 2] + b"\x00" * (k % 3) + two[1 - k % 4 // 2]
        else:
            three = [_crypto(0, d[:4]), _crypto(4, d[4:5]), _crypto(5, d[5:11])]
            frames = b"".join(three[j] for j in rng.permutation(3)) + b"\x00" * (k % 2)
        add(f"t{k}_{nf}", frames, pn_len)
    d = _rbytes(rng, 12)
    for k in range(4):
        add(f"gap{k}", _crypto(0, d[:4]) + _crypto(5 + k, d[4:8]), 1 + k % 2)
        add(f"frame_type{k}", _crypto(0, d[:4 + k]) + bytes([2 + k]) + b"\x00" * 4, 1 + k % 2)
        add(f"frame_eof{k}", _crypto(0, d[:4]) + b"\x06\x04" + bytes([9 + k]) + d[:6], 1 + k % 2)
        add(f"tagflip{k}", _crypto(0, d[:8]) + b"\x00" * k, 1 + k % 2, flip=-1 - 4 * k)
        add(f"version{k}", _crypto(0, d[:8]), 1 + k % 2, version=0xFF00001D - k)
        add(f"no_crypto{k}", b"\x00" * 5 + b"\x01" * (3 * k), 1 + k % 2)
    ids = {}
    classes = []
    for name, pkt in pkts:
        st, _, nf, _ = expected_initial(pkt)
        classes.append(ids.setdefault((st, min(nf, 2) if st == 0 else 0), len(ids)))
    return pkts, np.array(classes)


def grid_stride_pick(classes, n, seed):
    """Template index per packet, such that packet i + GRID_CAP (the second trip
    of block i) never has the class of packet i."""
    rng = np.random.default_rng(seed)
    t = len(classes)
    pick = rng.integers(0, t, n)
    others = [rng.permutation(np.nonzero(classes != classes[j])[0]) for j in range(t)]
    k = min(len(o) for o in others)
    alt = np.stack([o[:k] for o in others])
    first = pick[:n - GRID_CAP]
    pick[GRID_CAP:] = alt[first, rng.integers(0, k, len(first))]
    assert (classes[pick[GRID_CAP:]] != classes[first]).all()
    return pick


def pack_gapped(packets, gap=GAP, fill=SENTINEL):
    """Like pack(), with `gap` bytes of `fill` after every packet (and 64 at the end)."""
    lens = np.array([len(p) for p in packets], np.uint32)
    off = np.zeros(len(packets), np.uint64)
    if len(packets) > 1:
        np.cumsum(lens[:-1].astype(np.uint64) + np.uint64(gap), out=off[1:])
    g = bytes([fill]) * gap
    buf = np.frombuffer(b"".join(p + g for p in packets) + bytes([fill]) * 64, np.uint8).copy()
    return buf, off, lens


@functools.lru_cache(maxsize=None)
def expected_unprotect(key, packet: bytes, pn_offset: int, pn_max: int):
    """(status, hdr_len, plain_len, pn, the packet's bytes after the in-place call)
    by the oracle: OK -> unmasked header, plaintext, the original tag; -46 ->
    unmasked header, the original payload and tag; -45 / -53 -> unchanged."""
    if key.suite not in (AES, CHACHA):
        return -53, 0, 0, 0, packet
    buf = bytearray(packet)
    try:
        hdr, plain, pn = ref.unprotect(key, buf, pn_offset, pn_max)
    except ref.QuicError as e:
        st = status_of(e)   # the oracle unmasks the header in place before the AEAD fails
        hdr_len = pn_offset + (buf[0] & 3) + 1 if st == -46 else 0
        return st, hdr_len, 0, 0, bytes(buf)
    return 0, len(hdr), len(plain), pn, hdr + plain + packet[len(packet) - 16:]


def _first_diff(got, want, off, names):
    bad = np.nonzero(got != want)[0]
    if not len(bad):
        return None
    q = int(bad[0])
    i = int(np.searchsorted(np.asarray(off, np.uint64), np.uint64(q), side="right")) - 1
    return (names[max(i, 0)], q - int(off[max(i, 0)]), int(got[q]), int(want[q]), len(bad))


def check_unprotect_buffer(cases, buf, off, res):
    """The whole device buffer of pack_gapped(cases) after unprotect_batch, and
    the RESULT_DTYPE records, against the oracle: header, plaintext, tag, the
    payload of a packet that failed authentication, untouched error packets and
    the sentinel gaps between neighbours."""
    want = np.full(len(buf), SENTINEL, np.uint8)
    for i, (name, key, pkt, pn_offset, pn_max) in enumerate(cases):
        st, hdr_len, plain_len, pn, after = expected_unprotect(key, pkt, pn_offset, pn_max)
        assert len(after) == len(pkt), name
        o = int(off[i])
        want[o:o + len(pkt)] = np.frombuffer(after, np.uint8)
        r = res[i]
        assert int(r["status"]) == st, (name, int(r["status"]), st)
        assert int(r["plain_len"]) == plain_len, (name, int(r["plain_len"]), plain_len)
        if st == 0:
            assert (int(r["hdr_len"]), int(r["pn"])) == (hdr_len, pn), (name, int(r["hdr_len"]), int(r["pn"]), pn)
    assert len(buf) == len(want)
    assert np.array_equal(buf, want), _first_diff(buf, want, off, [c[0] for c in cases])


@functools.lru_cache(maxsize=None)
def expected_initial(packet: bytes):
    """(status, crypto data, CRYPTO frame count, the packet's bytes after the
    in-place ReadCryptoPayload) by the oracle.  The status and data are
    oracle_read's; the rest retraces payload.go:22-49 with the oracle's parts."""
    st, data = oracle_read(packet)
    try:
        hdr, offset = ref.parse_initial_header(packet)
    except ref.QuicError:
        return st, data, 0, packet
    end = offset + hdr["length"]
    if hdr["version"] not in (ref.V1, ref.V2) or offset == 0 or hdr["length"] == 0 or len(packet) < end:
        return st, data, 0, packet
    key = ref.initial_protection_key(ref.initial_secret(hdr["dcid"], hdr["version"], False), hdr["version"])
    buf = bytearray(packet[:end])
    try:
        h, plain, _ = ref.unprotect(key, buf, offset, 2)
    except ref.QuicError:
        return st, data, 0, bytes(buf) + packet[end:]   # -45: unchanged; -46: header unmasked
    try:
        nf = len(ref.extract_crypto_frames(plain))
    except ref.QuicError:
        nf = 0
    return st, data, nf, h + plain + packet[end - 16:]


def expected_crypto_out(pkts, out_off, caps, size):
    """(out buffer, status[], out_len[]) the device must leave: `size` sentinel
    bytes with the oracle's data at out_off[i] for the packets that read OK.  Two
    device limits have no reference counterpart: more than 256 CRYPTO frames
    (-52) and data larger than out_cap (-51, out_len = the size needed)."""
    out = np.full(size, SENTINEL, np.uint8)
    sts, lens = [], []
    for i, (name, pkt) in enumerate(pkts):
        st, data, nf, _ = expected_initial(pkt)
        n = len(data)
        if st == 0 and nf > 256:
            st, n = -52, 0
        elif st == 0 and n > int(caps[i]):
            st = -51
        elif st == 0:
            o = int(out_off[i])
            out[o:o + n] = np.frombuffer(data, np.uint8)
        sts.append(st)
        lens.append(n if st in (0, -51) else 0)
    return out, sts, lens


def check_crypto_out(pkts, out, out_off, caps, res):
    """Device ReadCryptoPayload against the oracle, over the whole sentinel-filled
    `out`: the data of every OK packet, the zeroed prefix before its first frame,
    and no byte written outside [out_off[i], out_off[i] + out_len[i])."""
    want, sts, lens = expected_crypto_out(pkts, out_off, caps, len(out))
    for i, (name, _) in enumerate(pkts):
        r = res[i]
        assert int(r["status"]) == sts[i], (name, int(r["status"]), sts[i])
        assert int(r["out_len"]) == lens[i], (name, int(r["out_len"]), lens[i])
    assert np.array_equal(out, want), _first_diff(out, want, out_off, [p[0] for p in pkts])


def check_initial_buffer(pkts, buf, off):
    """The packet buffer of pack_gapped(pkts) after read_crypto_payload_batch:
    unmasked header, plaintext in place, tag unchanged, and nothing touched past
    offset + Length, in an error packet or between packets."""
    want = np.full(len(buf), SENTINEL, np.uint8)
    for i, (name, pkt) in enumerate(pkts):
        after = expected_initial(pkt)[3]
        assert len(after) == len(pkt), name
        want[int(off[i]):int(off[i]) + len(pkt)] = np.frombuffer(after, np.uint8)
    assert np.array_equal(buf, want), _first_diff(buf, want, off, [p[0] for p in pkts])
