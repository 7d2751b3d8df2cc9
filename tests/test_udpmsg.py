"""CPU tier of the UDP relay message (include/hyobfs_udpmsg.h): the restatement
(tests/udpmsg_ref.py) and the scalar host ABI against the reference's own test
vectors (tests/golden/udpmsg_vectors.json) and against each other over the case
families of tests/udpmsg_cases.py, the traps one by one, and the device kernels
through a stand-alone AddressSanitizer build (tests/emu/udpmsg_main.cpp +
udpmsg.hip against hip_emu.h, run as a child process)."""
import ctypes
import fcntl
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import udpmsg_cases as uc
import udpmsg_ref as R
from hysteria_amd import _lib, udpmsg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
CLANG = "/opt/rocm/llvm/bin/clang++"
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "udpmsg_vectors.json")))


def _ref(v) -> R.UDPMessage:
    return R.UDPMessage(v["session_id"], v["packet_id"], v["frag_id"], v["frag_count"], v["addr"].encode(),
                        bytes.fromhex(v["data_hex"]))


def _lib_msg(m: R.UDPMessage) -> udpmsg.UDPMessage:
    return udpmsg.UDPMessage(m.session_id, m.packet_id, m.frag_id, m.frag_count, m.addr, m.data)


def _same(a, b) -> bool:
    f = ("session_id", "packet_id", "frag_id", "frag_count", "addr", "data")
    return all(getattr(a, k) == getattr(b, k) for k in f)


def _rec(r) -> tuple:
    return (r.status, r.session_id, r.packet_id, r.frag_id, r.frag_count, r.addr_off, r.addr_len, r.data_off, r.data_len)


# ------------------------------------------------------------------ golden vectors
def test_golden_serialize_and_parse():
    assert len(GOLDEN["serialize"]) == 2
    for v in GOLDEN["serialize"]:
        m, want = _ref(v), bytes.fromhex(v["wire_hex"])
        for impl in (m, _lib_msg(m)):
            assert impl.serialize(R.MAX_UDP_SIZE) == want
            assert impl.size() == len(want) and impl.header_size() == len(want) - len(m.data)
            assert impl.serialize(len(want)) == want and impl.serialize(len(want) - 1) == -1
        assert _same(R.parse(want), m) and _same(udpmsg.parse_udp_message(want), m)
    v = GOLDEN["buffer_too_small"]
    assert _ref(v).serialize(v["cap"]) == -1 and _lib_msg(_ref(v)).serialize(v["cap"]) == -1


def test_golden_malformed():
    want = [R.TRUNCATED, R.TRUNCATED, R.ADDR_LEN, R.TRUNCATED, R.ADDR_LEN]
    data = [bytes.fromhex(v["hex"]) for v in GOLDEN["malformed"]]
    assert data == uc.GOLDEN_MALFORMED
    for d, w in zip(data, want):
        assert R.parse(d) == w
        assert _rec(udpmsg.parse_record(d)) == (w, 0, 0, 0, 0, 0, 0, 0, 0)
        with pytest.raises(udpmsg.UDPMessageError) as e:
            udpmsg.parse_udp_message(d)
        assert e.value.status == w


def test_golden_frag_tables():
    assert [t["name"] for t in GOLDEN["frag"]] == ["no frag", "2 frags", "4 frags"]
    for t in GOLDEN["frag"]:
        m, want = _ref(t["m"]), [_ref(w) for w in t["want"]]
        got_ref, got_lib = R.frag_udp_message(m, t["max_size"]), udpmsg.frag_udp_message(_lib_msg(m), t["max_size"])
        assert len(got_ref) == len(got_lib) == len(want)
        assert all(_same(a, w) and _same(b, w) for a, b, w in zip(got_ref, got_lib, want))


def test_golden_defragger_sequence():
    """TestDefragger: one Defragger fed the whole sequence; the host ABI sees the
    serialised messages and answers with tags, from which the data is rebuilt."""
    d_ref, d_lib, wires = R.Defragger(), udpmsg.Defragger(), []
    assert len(GOLDEN["defrag"]) == 11
    for i, t in enumerate(GOLDEN["defrag"]):
        m = _ref(t["m"])
        want = None if t["want"] is None else _ref(t["want"])
        got = d_ref.feed(m)
        assert (got is None) == (want is None) and (want is None or _same(got, want)), t["name"]
        wires.append(m.serialize(R.MAX_UDP_SIZE))
        st, tags = d_lib.feed(udpmsg.parse_record(wires[i]), i)
        if want is None:
            assert st in (udpmsg.PENDING, udpmsg.ERR_FRAG_ID) and tags == [], t["name"]
            assert (st == udpmsg.ERR_FRAG_ID) == (m.frag_id >= m.frag_count)
        else:
            assert st == (udpmsg.WHOLE if m.frag_count <= 1 else udpmsg.COMPLETE)
            assert b"".join(R.parse(wires[k]).data for k in tags) == want.data, t["name"]
    d_lib.close()


# ------------------------------------------------------------------ restatement against the host ABI
def test_send_families_host_abi():
    """Rule A: hyobfs_udp_send_frags against the restatement over the lattice, the
    capacity family's messages, the scan family and a random sample."""
    msgs = uc.lattice_msgs() + uc.capacity_msgs() + uc.scan_msgs(300) + uc.random_msgs(300)
    seen = set()
    for sid, pid, addr, data, max_size in msgs:
        st, ds = R.send(sid, pid, addr, data, max_size)
        assert udpmsg.send_frags(sid, pid, addr, data, max_size) == (st, ds)
        assert udpmsg.frag_plan(len(addr), len(data), max_size)[0] == R.frag_plan(len(addr), len(data), max_size)[0]
        if st == R.OK:
            assert all(len(d) <= max_size for d in ds)
            if not data:   # sent as it is, and the receiver's P4 then refuses it
                assert [R.parse(d) for d in ds] == [R.MSG_LEN]
                continue
            got = [R.parse(d) for d in ds]
            assert b"".join(g.data for g in got) == data
            assert all((g.session_id, g.addr, g.frag_id, g.frag_count) == (sid, addr, k, len(ds))
                       for k, g in enumerate(got))
            assert all(g.packet_id == (pid if len(ds) > 1 else 0) for g in got)
        seen.add(st)
    assert seen == {R.OK, R.TOO_LARGE, R.NO_ROOM, R.FRAG_COUNT}


def test_frag_plan_matches_restatement():
    for al in uc.ADDR_LENS:
        for mp in uc.MAX_PAYLOADS:
            for dl in uc.data_lens(mp):
                for ms in (uc.header_size(al) + mp, uc.header_size(al), 0, 1200, 0xFFFFFFFF):
                    assert udpmsg.frag_plan(al, dl, ms) == R.frag_plan(al, dl, ms), (al, dl, ms)


def test_lattice_covers_every_residue():
    src, dst = uc.residues(uc.lattice_msgs())
    assert src == set(range(16)) and dst == set(range(16))
    st = [R.send(*m)[0] for m in uc.random_msgs()]
    assert st == [R.OK] * 3000   # by construction: no refusal can hide a failure


def test_parse_family_covers_every_produced_datagram():
    """Every datagram of the send cases is parsed whole and cut at header + 1, and every
    cut at 0 .. header is there up to what the parser can tell apart (both scan reaches)."""
    for reach in (uc.SMALL_SCAN_REACH, uc.SCAN_REACH):
        prod, items = uc.produced_datagrams(reach), uc.parse_datagrams(reach)
        assert len(prod) > 20000 and set(uc.GOLDEN_MALFORMED) <= set(items)
        uc.truncation_coverage(prod, items)
        lens = {uc._header_len(d) - 8 - (1 << (d[8] >> 6)) for d in prod}
        assert lens >= set(uc.ADDR_LENS) | {11}


def test_parse_family_host_abi():
    items = uc.parse_datagrams(uc.SMALL_SCAN_REACH)
    seen = set()
    for d in items:
        want = R.parsed_record(d)
        assert _rec(udpmsg.parse_record(d)) == want, d[:24].hex()
        seen.add(want[0])
    assert seen == {R.OK, R.TRUNCATED, R.ADDR_LEN, R.MSG_LEN}


def test_non_minimal_varints_all_four_widths():
    head = bytes.fromhex("0000002a00070102")
    forms = R.varint_forms(5)
    assert [len(f) for f in forms] == [1, 2, 4, 8]
    for f in forms:
        m = udpmsg.parse_udp_message(head + f + b"addr:" + b"xy")
        assert (m.addr, m.data, m.session_id, m.packet_id, m.frag_id, m.frag_count) == (b"addr:", b"xy", 42, 7, 1, 2)
        assert udpmsg.parse_record(head + f + b"addr:").status == R.MSG_LEN
        assert udpmsg.parse_record(head + f[:-1]).status == R.TRUNCATED
    assert R.varint_put(5) == forms[0] and udpmsg.UDPMessage(addr=b"addr:").header_size() == 14


def test_address_lengths_63_64_2048_2049():
    for al, vl in ((63, 1), (64, 2), (2048, 2), (2049, 2)):
        m = R.UDPMessage(9, 8, 0, 1, uc._addr(al), b"d")
        wire = m.serialize(R.MAX_UDP_SIZE)
        assert wire == _lib_msg(m).serialize() and len(wire) == 8 + vl + al + 1   # any address length serialises
        want = R.ADDR_LEN if al > 2048 else R.OK
        assert R.parsed_record(wire)[0] == udpmsg.parse_record(wire).status == want
    big = bytes.fromhex("0000002a00070102c000000100000005") + b"addr:x"   # 2^32 + 5 must not be taken for 5
    assert udpmsg.parse_record(big).status == R.parse(big) == R.ADDR_LEN


# ------------------------------------------------------------------ the traps
def test_trap_a1_dropped_although_fragments_would_fit():
    addr, data = b"10.0.0.1:53", bytes(4096 - 20 + 1)
    assert R.send(1, 2, addr, data, 1200) == udpmsg.send_frags(1, 2, addr, data, 1200) == (R.TOO_LARGE, [])
    assert len(R.frag_udp_message(R.UDPMessage(1, 2, 0, 1, addr, data), 1200)) == 4   # rule F alone would have split it
    st, ds = udpmsg.send_frags(1, 2, addr, data[:-1], 1200)
    assert st == R.OK and len(ds) == 4


def test_trap_f_more_than_255_fragments():
    m = R.UDPMessage(1, 2, 0, 1, b"a", bytes(256))
    assert R.frag_udp_message(m, 11) == R.FRAG_COUNT and udpmsg.frag_plan(1, 256, 11) == (R.FRAG_COUNT, 0, 0)
    with pytest.raises(udpmsg.UDPMessageError) as e:
        udpmsg.frag_udp_message(_lib_msg(m), 11)
    assert e.value.status == R.FRAG_COUNT
    assert udpmsg.send_frags(1, 2, b"a", bytes(256), 11) == (R.FRAG_COUNT, [])
    assert udpmsg.frag_plan(1, 255, 11) == (R.OK, 255, 1) and len(udpmsg.send_frags(1, 2, b"a", bytes(255), 11)[1]) == 255


def _feed_both(d_ref, d_lib, wires, m):
    wires.append(m.serialize(R.MAX_UDP_SIZE))
    got = d_ref.feed(m)
    st, tags = d_lib.feed(udpmsg.parse_record(wires[-1]), len(wires) - 1)
    assert (got is not None) == (st in (udpmsg.WHOLE, udpmsg.COMPLETE))
    if got is not None:
        assert b"".join(R.parse(wires[k]).data for k in tags) == got.data
    return got, st, tags


def test_trap_d1_whole_message_leaves_an_assembly_alone():
    d_ref, d_lib, w = R.Defragger(), udpmsg.Defragger(), []
    assert _feed_both(d_ref, d_lib, w, R.UDPMessage(1, 50, 0, 2, b"a:1", b"one "))[0] is None
    got, st, tags = _feed_both(d_ref, d_lib, w, R.UDPMessage(1, 0, 0, 1, b"a:1", b"whole"))
    assert got.data == b"whole" and st == udpmsg.WHOLE and tags == [1]
    got, st, tags = _feed_both(d_ref, d_lib, w, R.UDPMessage(1, 50, 1, 2, b"a:1", b"two"))
    assert got.data == b"one two" and st == udpmsg.COMPLETE and tags == [0, 2]


def test_trap_d5_session_and_address_of_the_last_arrival():
    d_ref, d_lib, w = R.Defragger(), udpmsg.Defragger(), []
    _feed_both(d_ref, d_lib, w, R.UDPMessage(7, 50, 1, 2, b"late:2", b"B"))
    got, st, tags = _feed_both(d_ref, d_lib, w, R.UDPMessage(7, 50, 0, 2, b"early:1", b"A"))
    assert (got.addr, got.data, tags) == (b"early:1", b"AB", [1, 0])   # fragment 0 arrived last: its address


def test_trap_d6_state_survives_completion():
    d_ref, d_lib, w = R.Defragger(), udpmsg.Defragger(), []
    _feed_both(d_ref, d_lib, w, R.UDPMessage(1, 50, 0, 2, b"a:1", b"x"))
    assert _feed_both(d_ref, d_lib, w, R.UDPMessage(1, 50, 1, 2, b"a:1", b"y"))[1] == udpmsg.COMPLETE
    for k in (0, 1, 0):   # the same PacketID again: swallowed, nothing completes
        got, st, _ = _feed_both(d_ref, d_lib, w, R.UDPMessage(1, 50, k, 2, b"a:1", b"z"))
        assert got is None and st == udpmsg.PENDING
    _feed_both(d_ref, d_lib, w, R.UDPMessage(1, 51, 0, 2, b"a:1", b"p"))       # another id resets
    assert _feed_both(d_ref, d_lib, w, R.UDPMessage(1, 51, 1, 2, b"a:1", b"q"))[0].data == b"pq"
    assert _feed_both(d_ref, d_lib, w, R.UDPMessage(1, 51, 2, 2, b"a:1", b"q"))[1] == udpmsg.ERR_FRAG_ID   # D2


def test_defrag_stream_host_abi():
    stream = uc.defrag_stream()
    want = uc.expected_defrag(stream)
    recs = [udpmsg.parse_record(d) for d in stream]
    arr = np.frombuffer(b"".join(bytes(r) for r in recs), udpmsg.PARSED_DTYPE)
    lists, last = udpmsg.defrag_plan(arr)
    got = [(int(arr[l]["session_id"]), R.parse(stream[l]).addr, b"".join(R.parse(stream[i]).data for i in t))
           for t, l in zip(lists, last)]
    assert got == want and 10 < len(want) < len(stream)
    assert any(len(t) > 1 for t in lists)


# ------------------------------------------------------------------ ABI surface
def test_structs_match_header(tmp_path):
    body, want = [], []
    for ct, cls in (("hyobfs_udp_header", udpmsg.HyobfsUdpHeader), ("hyobfs_udp_parsed", udpmsg.HyobfsUdpParsed),
                    ("hyobfs_udp_meta", udpmsg.HyobfsUdpMeta)):
        for f, _ in cls._fields_:
            body.append(f'printf("%zu\\n", offsetof({ct}, {f}));')
            want.append(getattr(cls, f).offset)
        body.append(f'printf("%zu\\n", sizeof({ct}));')
        want.append(ctypes.sizeof(cls))
    for ct, dt in (("hyobfs_udp_parsed", udpmsg.PARSED_DTYPE), ("hyobfs_udp_meta", udpmsg.META_DTYPE)):
        for f in dt.names:
            body.append(f'printf("%zu\\n", offsetof({ct}, {f}));')
            want.append(dt.fields[f][1])
    consts = ["HYOBFS_UDP_ERR_TRUNCATED", "HYOBFS_UDP_ERR_ADDR_LEN", "HYOBFS_UDP_ERR_MSG_LEN", "HYOBFS_UDP_ERR_FRAG_ID",
              "HYOBFS_UDP_TOO_LARGE", "HYOBFS_UDP_NO_ROOM", "HYOBFS_UDP_ERR_FRAG_COUNT", "HYOBFS_UDP_ERR_CAP",
              "HYOBFS_UDP_ERR_PLAN", "HYOBFS_UDP_MAX_SIZE", "HYOBFS_UDP_MAX_ADDR", "HYOBFS_UDP_MAX_FRAGS",
              "HYOBFS_UDP_PENDING", "HYOBFS_UDP_WHOLE", "HYOBFS_UDP_COMPLETE", "HYOBFS_SNIFF_ERR_UNRECOGNIZED",
              "HYOBFS_ABI_VERSION"]
    body += [f'printf("%d\\n", (int){c});' for c in consts]
    want += [*range(-68, -77, -1), 4096, 2048, 255, 0, 1, 2, -67, 4]
    assert (udpmsg.ERR_TRUNCATED, udpmsg.ERR_PLAN, udpmsg.MAX_SIZE, udpmsg.MAX_ADDR, udpmsg.MAX_FRAGS) == \
        (R.TRUNCATED, R.PLAN, R.MAX_UDP_SIZE, R.MAX_MESSAGE_LENGTH, 255)
    assert (udpmsg.ERR_ADDR_LEN, udpmsg.ERR_MSG_LEN, udpmsg.ERR_FRAG_ID, udpmsg.TOO_LARGE, udpmsg.NO_ROOM,
            udpmsg.ERR_FRAG_COUNT, udpmsg.ERR_CAP) == (R.ADDR_LEN, R.MSG_LEN, R.FRAG_ID, R.TOO_LARGE, R.NO_ROOM,
                                                       R.FRAG_COUNT, R.CAP)
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hyobfs_udpmsg.h"\n#include "hyobfs_sniff.h"\n'
                   'int main(void){\n' + "\n".join(body) + "\nreturn 0;}\n")
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    vals = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert vals == want


def test_empty_batches_and_null_pointers():
    lib = udpmsg._ulib()
    assert lib.hyobfs_abi_version() == 4
    N = None
    assert lib.hyobfs_udp_parse_batch(N, N, N, 0, N, N) == 0
    assert lib.hyobfs_udp_frag_batch(N, N, N, N, N, 0, N, 0, N, N, 0, N, N, N, N, N) == 0
    assert lib.hyobfs_udp_assemble_batch(N, N, N, 0, N, N, 0, N, N, N, N, N, N) == 0
    assert lib.hyobfs_udp_assemble_batch(N, N, N, 5, N, N, 0, N, N, N, N, N, N) == 0
    assert lib.hyobfs_udp_parse_batch(N, N, N, 1, N, N) == _lib.HYOBFS_ERR_INVALID
    assert lib.hyobfs_udp_frag_batch(N, N, N, N, N, 1, N, 0, N, N, 0, N, N, N, N, N) == _lib.HYOBFS_ERR_INVALID
    assert lib.hyobfs_udp_assemble_batch(N, N, N, 0, N, N, 1, N, N, N, N, N, N) == _lib.HYOBFS_ERR_INVALID
    assert lib.hyobfs_udp_frag_workspace_size(0) == 16 and lib.hyobfs_udp_frag_workspace_size(257) == (2 * 3 + 5) * 8
    assert lib.hyobfs_udp_parse(N, 0, N) == _lib.HYOBFS_ERR_INVALID
    c = ctypes.c_uint32()
    assert lib.hyobfs_udp_frag_plan(1, 1, 100, N, ctypes.byref(c)) == _lib.HYOBFS_ERR_INVALID
    assert lib.hyobfs_udp_serialize(N, N, 0, N, 0, N, 0) == -1
    assert lib.hyobfs_udp_send_frags(N, N, N, 0, N, 0, N, N) == _lib.HYOBFS_ERR_INVALID
    assert lib.hyobfs_udp_defragger_feed(N, N, 0, N, N) == _lib.HYOBFS_ERR_INVALID
    lib.hyobfs_udp_defragger_free(N)


def test_package_exports():
    import hysteria_amd
    for name in ("udpmsg", "UDPMessage", "UDPMessageError", "parse_udp_message", "frag_udp_message", "Defragger",
                 "relay_quic_snis", "UDP_PARSED_DTYPE", "UDP_META_DTYPE"):
        assert name in hysteria_amd.__all__ and hasattr(hysteria_amd, name)
    for name in ("parse_batch", "frag_batch", "assemble_batch", "frag_workspace_size", "send_frags", "HyobfsUdpMeta"):
        assert hasattr(udpmsg, name)


# ------------------------------------------------------------------ the kernels on the CPU
def _build_main(name, defines=()):
    """tests/emu/build/<name>: udpmsg.hip + the driver, compiled for the host with
    AddressSanitizer (a program with its own main: nothing is preloaded).  Rebuilt when a
    source is newer."""
    if not os.path.exists(CLANG):
        pytest.skip("no host clang for the emulated build")
    csrc = os.path.join(ROOT, "hysteria_amd", "csrc")
    srcs = [os.path.join(EMU, "udpmsg_main.cpp"), os.path.join(csrc, "udpmsg.hip")]
    deps = srcs + [os.path.join(EMU, "hip_emu.h"), os.path.join(csrc, "kernels.h"), os.path.join(csrc, "udpmsg_rules.h"),
                   os.path.join(csrc, "salamander_device.h"), os.path.join(ROOT, "include", "hyobfs_udpmsg.h")]
    os.makedirs(os.path.join(EMU, "build"), exist_ok=True)
    exe = os.path.join(EMU, "build", name)
    with open(os.path.join(EMU, "build", f".{name}.lock"), "w") as lk:
        fcntl.flock(lk, fcntl.LOCK_EX)
        if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(d) for d in deps):
            tmp = exe + ".tmp"
            subprocess.run([CLANG, "-std=c++20", "-O1", "-g", "-DHYOBFS_EMULATE", "-I" + EMU, "-I" + csrc, "-x", "c++",
                            "-fsanitize=address", "-fno-omit-frame-pointer", "-pthread",
                            "-Wno-unused-command-line-argument", *defines, *srcs, "-o", tmp], check=True,
                           capture_output=True)
            os.replace(tmp, exe)
    return exe


@pytest.fixture(scope="module")
def udpmsg_main():
    return _build_main("udpmsg_main")


@pytest.fixture(scope="module")
def udpmsg_main_small_scan():
    """The same sources with 64-message tiles and 64-tile scan passes: a batch beyond one
    pass of the scan is 4097 messages instead of 65537 (a workgroup costs 256 host threads here)."""
    return _build_main("udpmsg_main_small_scan", ("-DHY_UDP_TILE_MSGS=64", "-DHY_UDP_SCAN_TILES=64"))


def _run(exe, tmp_path, blob: bytes) -> bytes:
    src, dst = tmp_path / "cases.bin", tmp_path / "results.bin"
    src.write_bytes(blob)
    r = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.splitlines()[-1:] == ["done"], r.stderr[-4000:]
    return dst.read_bytes()


class _Reader:
    def __init__(self, b):
        self.b, self.at = b, 0

    def arr(self, dtype, n):
        a = np.frombuffer(self.b, dtype, n, self.at)
        self.at += a.nbytes
        return a

    def done(self):
        return self.at == len(self.b)


def check_send_result(case, rc, status, first, totals, dgram_off, dgram_len, lead, out):
    """One hyobfs_udp_frag_batch run against the restatement, bit for bit; what is not
    stated to be written must still hold the guard byte.  Shared with the GPU tier."""
    e_status, e_first, e_totals, e_out, entries, oc, dc = uc.expected_send(case)
    name = case["name"]
    assert rc == 0, name
    assert list(status) == e_status, (name, [i for i, (a, b) in enumerate(zip(status, e_status)) if a != b][:8])
    assert list(first) == e_first and tuple(totals) == e_totals, name
    assert len(dgram_off) == len(dgram_len) == dc
    guard64, guard32 = int.from_bytes(bytes([uc.GUARD]) * 8, "little"), int.from_bytes(bytes([uc.GUARD]) * 4, "little")
    want_off = np.full(dc, guard64, np.uint64)
    want_len = np.full(dc, guard32, np.uint32)
    for d, (o, ln) in entries.items():
        want_off[d], want_len[d] = o, ln
    assert np.array_equal(dgram_off, want_off) and np.array_equal(dgram_len, want_len), name
    assert bytes(lead) == bytes([uc.GUARD]) * len(lead), name
    if bytes(out) != e_out:
        a, b = np.frombuffer(bytes(out), np.uint8), np.frombuffer(e_out, np.uint8)
        bad = np.flatnonzero(a != b)
        raise AssertionError((name, "first differing output byte", int(bad[0]), "of", len(bad)))


def _check_send_cases(exe, tmp_path, cases):
    res = _Reader(_run(exe, tmp_path, b"".join(uc.blob_send(c) for c in cases)))
    for c in cases:
        n = len(c["msgs"])
        _, _, _, _, _, oc, dc = uc.expected_send(c)
        rc = int(res.arr(np.int32, 1)[0])
        status, first, totals = res.arr(np.int32, n), res.arr(np.uint64, n + 1), res.arr(np.uint64, 2)
        dgram_off, dgram_len = res.arr(np.uint64, dc), res.arr(np.uint32, dc)
        buf = res.arr(np.uint8, c["out_mis"] + oc if oc else 0)
        check_send_result(c, rc, status, first, totals, dgram_off, dgram_len, buf[:c["out_mis"] if oc else 0],
                          buf[c["out_mis"] if oc else 0:])
    assert res.done()


def test_emulated_frag_lattice(udpmsg_main, tmp_path):
    _check_send_cases(udpmsg_main, tmp_path, uc.lattice_cases())


def test_emulated_frag_inputs_in_poisoned_slots(udpmsg_main, tmp_path):
    """The lattice, the capacity messages and a random sample again with every payload and
    every message's address in a slot of its own, the bytes up to the next slot poisoned: a
    load that leaves its payload or address, even into a neighbour, stops the driver."""
    cases = [dict(uc.lattice_cases()[1], name="lattice_spread", spread=1),
             dict(uc.capacity_cases()[0], name="capacity_spread", spread=1),
             dict(uc.random_case(600), name="random_spread", spread=1)]
    _check_send_cases(udpmsg_main, tmp_path, cases)


def test_emulated_frag_capacity(udpmsg_main, tmp_path):
    cases = uc.capacity_cases()
    assert len(cases) == 10
    _check_send_cases(udpmsg_main, tmp_path, cases)


def test_emulated_frag_scan_edges(udpmsg_main, udpmsg_main_small_scan, tmp_path):
    cases = uc.scan_cases(uc.SMALL_SCAN_REACH)
    assert max(len(c["msgs"]) for c in cases) == 64 * 64 + 1
    _check_send_cases(udpmsg_main_small_scan, tmp_path, cases)
    _check_send_cases(udpmsg_main, tmp_path, [c for c in cases if len(c["msgs"]) <= 257])   # the shipped widths


def test_emulated_frag_random(udpmsg_main, tmp_path):
    _check_send_cases(udpmsg_main, tmp_path, [uc.random_case()])


def test_emulated_parse(udpmsg_main, tmp_path):
    items = uc.parse_datagrams(uc.SMALL_SCAN_REACH)   # the GPU tier parses the family of the shipped scan reach
    res = _Reader(_run(udpmsg_main, tmp_path, uc.blob_parse(items)))
    assert int(res.arr(np.int32, 1)[0]) == 0
    got = res.arr(udpmsg.PARSED_DTYPE, len(items))
    assert res.done()
    for d, g in zip(items, got):
        assert tuple(int(g[f]) for f in udpmsg.PARSED_DTYPE.names[:-1]) == R.parsed_record(d), d[:24].hex()
        assert int(g["reserved_"]) == 0


def assemble_inputs():
    """(datagrams, lists, caps, gaps, expected statuses, expected data): the defragmented
    stream with out_cap[j] exact and, for some, one short; then the ERR_PLAN causes."""
    stream = uc.defrag_stream() + [bytes(12)]   # the last one does not parse
    arr = np.frombuffer(b"".join(bytes(udpmsg.parse_record(d)) for d in stream), udpmsg.PARSED_DTYPE)
    lists, _ = udpmsg.defrag_plan(arr)
    want = [d for _, _, d in uc.expected_defrag(stream)]
    caps = [len(d) - (1 if j % 4 == 3 else 0) for j, d in enumerate(want)]
    exp_st = [R.CAP if j % 4 == 3 else R.OK for j in range(len(want))]
    ok_idx = [i for i in range(len(stream)) if arr[i]["status"] == 0][:2]
    plists, pexp = uc.assemble_plan_cases(len(stream), ok_idx, len(stream) - 1)
    for l, e in zip(plists, pexp):
        data = b"".join(R.parse(stream[i]).data for i in l) if e is None else b""
        lists.append(l)
        want.append(data)
        caps.append(len(data) + (2 if e is None else 64))
        exp_st.append(R.OK if e is None else e)
    want = [d if s == R.OK else b"" for d, s in zip(want, exp_st)]
    gaps = [(5 * j + 1) % 23 for j in range(len(lists))]
    return stream, lists, caps, gaps, exp_st, want


def check_assemble_result(status, out_len, out, caps, gaps, exp_st, want):
    assert list(status) == exp_st
    assert list(out_len) == [len(d) for d in want]
    exp, at = bytearray(), 0
    for c, g, d in zip(caps, gaps, want):
        exp += bytes([uc.GUARD]) * g + d + bytes([uc.GUARD]) * (c - len(d))
    assert bytes(out) == bytes(exp)


def test_emulated_assemble(udpmsg_main, tmp_path):
    stream, lists, caps, gaps, exp_st, want = assemble_inputs()
    assert {R.OK, R.CAP, R.PLAN} == set(exp_st) and any(len(l) > 2 for l, s in zip(lists, exp_st) if s == R.OK)
    res = _Reader(_run(udpmsg_main, tmp_path, uc.blob_assemble(stream, lists, caps, gaps)))
    assert list(res.arr(np.int32, 2)) == [0, 0]
    m = len(lists)
    status, out_len = res.arr(np.int32, m), res.arr(np.uint32, m)
    total = int(res.arr(np.uint64, 1)[0])
    out = res.arr(np.uint8, total)
    assert res.done()
    check_assemble_result(status, out_len, out, caps, gaps, exp_st, want)
