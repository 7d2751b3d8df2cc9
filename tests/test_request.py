"""CPU tier of the request hook (include/hyobfs_request.h): the restatement
(tests/request_ref.py) against the reference's own test tables, the golden file
(tests/golden/request_vectors.json) against the restatement, the scalar host ABI
against the restatement over the lattices of tests/request_cases.py, and the four
device kernels through a stand-alone AddressSanitizer / UndefinedBehaviorSanitizer
build (tests/emu/request_main.cpp + request.hip against hip_emu.h, run as a child
process) over every lattice case, in guarded and poisoned buffers."""
import ctypes
import fcntl
import json
import os
import re
import subprocess

import numpy as np
import pytest

import request_cases as rc
import request_ref as R
from hysteria_amd import _lib, request, sniff

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
CLANG = "/opt/rocm/llvm/bin/clang++"
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "request_vectors.json")))
GO = GOLDEN["go"]


# ------------------------------------------------------------------ the restatement against the reference's tables
def test_restatement_agrees_with_the_reference_tables():
    for t in GO["read_tcp_request"]:
        b = bytes.fromhex(t["data"])
        st, need, ao, al, used = R.read_tcp_request(b)
        assert (st != R.OK) == t["err"] and b[ao:ao + al].decode() == t["want"], t["name"]
        if t["err"]:
            assert st == R.NEED_MORE and need > len(b)
    for t in GO["write_tcp_request"]:
        w = R.write_tcp_request(t["addr"].encode(), 64, 1, 2)
        assert w.startswith(bytes.fromhex(t["prefix"])) and len(w) > len(t["prefix"]) // 2, t["name"]
    for t in GO["read_tcp_response"]:
        b = bytes.fromhex(t["data"])
        st, need, ok, mo, ml, used = R.read_tcp_response(b)
        assert ((st != R.OK), bool(ok), b[mo:mo + ml].decode()) == (t["err"], t["ok"], t["msg"]), t["name"]
    for t in GO["write_tcp_response"]:
        w = R.write_tcp_response(t["ok"], t["msg"].encode(), 128, 1, 2)
        assert w.startswith(bytes.fromhex(t["prefix"])) and len(w) > len(t["prefix"]) // 2, t["name"]
    for t in GO["sniffer_check"]:
        tcp, udp = ([tuple(r) for r in u] if u is not None else None for u in (t["tcp"], t["udp"]))
        assert R.check(t["addr"].encode(), t["is_udp"], t["rewrite_domain"], tcp, udp) == t["want"], t
    for t in GO["parse_port_union"]:
        want = None if t["want"] is None else [tuple(r) for r in t["want"]]
        assert R.parse_port_union(t["s"].encode()) == want, t["name"]


def test_restatement_agrees_with_the_python_sniffer():
    """hysteria_amd.sniff.Sniffer.check stays as it is, and says the same over every text within its reach."""
    n = 0
    for k, u in enumerate(rc.UNIONS):
        s = sniff.Sniffer(rewrite_domain=bool(k % 2), tcp_ports=u, udp_ports=rc.UNIONS[-1 - k])
        for t in rc.check_items():
            try:
                text = t.decode("ascii")
            except UnicodeDecodeError:
                continue
            if len(t) > R.MAX_ADDR:   # the LIMIT is this library's
                continue
            m = re.search(rb":([+-]?[0-9]+)$", t)
            if m and R.atoi(m.group(1)) is None:   # the mirror takes its port as a Python integer: no ErrRange
                continue
            for is_udp in (False, True):
                assert s.check(is_udp, text) == R.check(t, is_udp, s.rewrite_domain, s.tcp_ports, s.udp_ports), (t, is_udp)
                n += 1
    assert n > 3000


def test_golden_file_is_the_restatements():
    assert json.loads(json.dumps(rc.golden_lattice())) == GOLDEN["lattice"]
    assert all(len(GOLDEN["lattice"][k]) >= 3 for k in ("request", "response", "union", "check", "rewrite", "padding"))


# ------------------------------------------------------------------ the scalar ABI
def test_scalar_against_the_reference_tables():
    for t in GO["read_tcp_request"]:
        b = bytes.fromhex(t["data"])
        if t["err"]:
            with pytest.raises(request.RequestError) as e:
                request.read_tcp_request(b)
            assert e.value.status == request.ERR_NEED_MORE and e.value.need > len(b)
        else:
            assert request.read_tcp_request(b) == (t["want"].encode(), len(b))
    for t in GO["write_tcp_request"]:
        assert request.write_tcp_request(t["addr"], 64).startswith(bytes.fromhex(t["prefix"]))
    for t in GO["read_tcp_response"]:
        b = bytes.fromhex(t["data"])
        if t["err"]:
            with pytest.raises(request.RequestError):
                request.read_tcp_response(b)
        else:
            assert request.read_tcp_response(b) == (t["ok"], t["msg"].encode(), len(b))
    for t in GO["write_tcp_response"]:
        assert request.write_tcp_response(t["ok"], t["msg"], 128).startswith(bytes.fromhex(t["prefix"]))
    for t in GO["sniffer_check"]:
        assert request.check(t["addr"], t["is_udp"], t["rewrite_domain"], t["tcp"], t["udp"]) == t["want"], t
    for t in GO["parse_port_union"]:
        want = None if t["want"] is None else [tuple(r) for r in t["want"]]
        assert request.parse_port_union(t["s"]) == want, t["name"]


def test_scalar_request_and_response_parse():
    for t in rc.parse_items():
        assert request.tcp_request_record(t) == R.read_tcp_request(t), t[:40]
    frames = [rc.response_one(x, i) for i, x in enumerate(rc.response_items()) if x[1] < len(rc.MSGS)]
    frames += [R.varint(0, 8).join([b"\x00", R.varint(2049, 2)]), b"\x01" + R.varint(2049, 4), b"\x00\x01m" + R.varint(4097, 8),
               b"\x07" + R.varint(2048, 8) + b"m" * 2048 + R.varint(4096, 8) + b"p" * 4096 + b"rest"]
    n = 0
    for f in frames:
        cuts = range(len(f) + 1) if len(f) < 300 else (0, 1, 2, 3, 4, len(f) // 2, len(f) - 1, len(f))
        for cut in cuts:
            assert request.tcp_response_record(f[:cut]) == R.read_tcp_response(f[:cut]), (f[:20], cut)
            n += 1
    assert n > 2000
    for g in GOLDEN["lattice"]["request"]:
        assert list(request.tcp_request_record(bytes.fromhex(g["hex"]))) == g["result"]
    for g in GOLDEN["lattice"]["response"]:
        if "parse" in g:
            assert list(request.tcp_response_record(bytes.fromhex(g["parse"]))) == g["result"]


def test_scalar_builds_and_padding():
    for i, (ok, m, p) in enumerate(rc.response_items()):
        if m >= len(rc.MSGS):
            continue
        e = R.write_tcp_response(bool(ok), rc.MSGS[m], p, rc.SEED, i)
        assert request.write_tcp_response(bool(ok), rc.MSGS[m], p, rc.SEED, i) == e
        assert request.write_tcp_response(bool(ok), rc.MSGS[m], p, rc.SEED, i, cap=len(e)) == e
        assert request.write_tcp_response(bool(ok), rc.MSGS[m], p, rc.SEED, i, cap=len(e) - 1) == -1
        assert request.read_tcp_response(e + b"x") == (bool(ok), rc.MSGS[m], len(e))
    for i, a in enumerate((b"", b"a:1", b"h" * 63, b"h" * 64, b"h" * 2048, b"h" * 5000)):   # no length is validated on writing
        for p in (0, 1, 63, 64, 511, 5000):
            e = R.write_tcp_request(a, p, 5, i)
            assert request.write_tcp_request(a, p, 5, i) == e and request.write_tcp_request(a, p, 5, i, cap=len(e) - 1) == -1
            if 1 <= len(a) <= 2048 and p <= 4096:
                assert request.read_tcp_request(e[2:]) == (a, len(e) - 2)
    for seed, item in ((0, 0), (1, 0), (0, 1), (rc.SEED, 12345), ((1 << 64) - 1, (1 << 64) - 1)):
        pad = request.padding(seed, item, 301)
        assert pad == R.padding(seed, item, 301) and set(pad) <= set(R.PADDING_CHARS)
        assert request.padding(seed, item, 7) == pad[:7]   # a function of (seed, item, k) only
    assert len(set(R.padding(3, 4, 4000))) == 62 and R.padding(3, 4, 64) != R.padding(3, 5, 64) != R.padding(4, 4, 64)
    for g in GOLDEN["lattice"]["padding"]:
        assert request.padding(g["seed"], g["item"], len(g["text"])) == g["text"].encode()
    for g in GOLDEN["lattice"]["response"]:
        if "hex" in g:
            assert request.write_tcp_response(bool(g["ok"]), bytes.fromhex(g["msg"]), g["pad_len"], rc.SEED,
                                              g["item"]).hex() == g["hex"]


def test_scalar_port_union():
    for t in rc.UNION_TEXTS:
        assert request.parse_port_union(t) == R.parse_port_union(t), t
    for g in GOLDEN["lattice"]["union"]:
        assert request.parse_port_union(g["text"]) == (None if g["ranges"] is None else [tuple(r) for r in g["ranges"]])
    lib = request._rqlib()
    out, n = np.zeros(4, request.PORT_RANGE_DTYPE), ctypes.c_uint32()
    t = b"1,3,5,7"
    assert lib.hyobfs_port_union_parse(t, len(t), out.ctypes.data, 3, ctypes.byref(n)) == request.ERR_CAP and n.value == 4
    assert not out.view(np.uint8).any()
    for u in rc.UNIONS:
        for port in (0, 1, 69, 70, 79, 80, 81, 85, 86, 89, 100, 101, 443, 65534, 65535):
            assert request.port_union_contains(u, port) == R.contains(u, port), (u, port)


def test_scalar_check():
    n = 0
    for k, t in enumerate(rc.check_items()):
        for j in range(4):
            tcp, udp = rc.UNIONS[(k + j) % len(rc.UNIONS)], rc.UNIONS[(k + 2 * j + 1) % len(rc.UNIONS)]
            for is_udp in (False, True):
                e = R.check(t, is_udp, bool(j & 1), tcp, udp)
                assert request.check(t, is_udp, bool(j & 1), tcp, udp) == e, (t[:90], is_udp, j, tcp, udp)
                n += e
    assert n > 500
    for g in GOLDEN["lattice"]["check"]:
        t = bytes.fromhex(g["hex"])
        assert [int(request.check(t, bool(k & 1), bool(k & 2), rc.UNIONS[3], rc.UNIONS[5])) for k in range(4)] == g["verdicts"]
    # C5: the low 16 bits of the two's complement
    for port, want in ((b"-1", 65535), (b"65536", 0), (b"65616", 80), (b"-65456", 80), (b"+80", 80), (b"-0", 0),
                       (b"9223372036854775807", 65535), (b"-9223372036854775808", 0)):
        assert request.check(b"1.2.3.4:" + port, False, False, [(want, want)], []) is True
        assert request.check(b"1.2.3.4:" + port, False, False, [((want + 1) % 65536,) * 2], None) is False


def test_scalar_rewrite():
    for item in rc.rewrite_items():
        a, chk, nm, nlen, sst = item
        st, text, rew = rc.rewrite_one(item)
        name = nm if sst == rc.OK_ else b""
        if st != R.OK:
            with pytest.raises(request.RequestError) as e:
                request.rewrite(a, bool(chk), name, sst)
            assert e.value.status == st
            continue
        assert request.rewrite(a, bool(chk), name, sst) == (text, bool(rew)), item[:2]
        assert request.rewrite(a, bool(chk), name, sst, cap=len(text)) == (text, bool(rew))
        if text:
            assert request.rewrite(a, bool(chk), name, sst, cap=len(text) - 1) == -1
    assert request.rewrite("1.2.3.4:+80", True, b"example.org") == (b"example.org:+80", True)
    assert request.rewrite("1.2.3.4:80", True, b"1.2.3.4") == (b"1.2.3.4:80", True)   # what Outbound.TCP parses as an IP again
    for g in GOLDEN["lattice"]["rewrite"]:
        name = bytes.fromhex(g["name"])
        try:
            got = request.rewrite(bytes.fromhex(g["addr"]), bool(g["check"]), name, g["sniff_status"])
            assert (R.OK, got[0].hex(), int(got[1])) == (g["status"], g["text"], g["rewritten"])
        except request.RequestError as e:
            assert e.status == g["status"]


def test_status_strings_empty_batches_and_null_pointers():
    for st in range(-86, -94, -1):
        assert _lib.status_string(st) not in ("", "unknown status") and _lib.status_string(st) != _lib.status_string(-85)
    assert _lib.status_string(request.ERR_ADDR_LEN) == "invalid address length"      # the reference's ProtocolError texts
    assert _lib.status_string(request.ERR_PADDING_LEN) == "invalid padding length"
    assert _lib.status_string(request.ERR_MSG_LEN) == "invalid message length"
    lib, N = request._rqlib(), None
    assert lib.hyobfs_tcp_request_parse_batch(N, N, N, 0, N, N, N, N, N, N, N) == 0
    assert lib.hyobfs_sniff_check_batch(N, N, N, N, 0, 0, 0, N, N, N) == 0
    assert lib.hyobfs_request_rewrite_batch(N, N, N, N, N, N, 0, N, 0, N, 0, 0, N, N, N, N, N) == 0
    assert lib.hyobfs_tcp_response_build_batch(N, N, N, N, N, 0, N, 0, 0, N, 0, N, N, N) == 0
    inv = _lib.HYOBFS_ERR_INVALID
    assert lib.hyobfs_tcp_request_parse_batch(N, N, N, 1, N, N, N, N, N, N, N) == inv
    assert lib.hyobfs_sniff_check_batch(N, N, N, N, 1, 0, 0, N, N, N) == inv
    assert lib.hyobfs_request_rewrite_batch(N, N, N, N, N, N, 0, N, 1, N, 64, 0, N, N, N, N, N) == inv
    assert lib.hyobfs_tcp_response_build_batch(N, N, N, N, N, 0, N, 0, 1, N, 64, N, N, N) == inv
    u32 = ctypes.c_uint32()
    assert lib.hyobfs_tcp_request_parse(N, 0, N, N, N, N) == inv
    assert lib.hyobfs_tcp_request_parse(N, 0, *[ctypes.byref(u32)] * 4) == request.ERR_NEED_MORE and u32.value == 0
    assert lib.hyobfs_tcp_response_parse(N, 0, N, N, N, N, N) == inv
    assert lib.hyobfs_port_union_parse(N, 0, N, 0, N) == inv
    assert lib.hyobfs_port_union_parse(N, 0, N, 0, ctypes.byref(u32)) == request.ERR_UNION
    assert lib.hyobfs_port_union_contains(N, -1, 5) == 1 and lib.hyobfs_port_union_contains(N, 0, 5) == 0
    assert lib.hyobfs_sniff_check(N, 0, 0, 1, N, -1, N, -1) == 0
    assert lib.hyobfs_request_rewrite(N, 0, 0, N, 0, 0, N, 0, N) == inv
    assert lib.hyobfs_portset_new(N, 0, 0, N) == inv
    lib.hyobfs_portset_free(N)


def test_package_exports():
    import hysteria_amd
    for name in ("request", "PortSet", "RequestError", "tcp_request_decisions", "hooked_relay_acl_decisions"):
        assert name in hysteria_amd.__all__ and hasattr(hysteria_amd, name)
    for name in ("read_tcp_request", "write_tcp_request", "read_tcp_response", "write_tcp_response", "parse_port_union",
                 "check", "rewrite", "padding", "PortSet", "tcp_request_parse_batch", "sniff_check_batch",
                 "request_rewrite_batch", "tcp_response_build_batch", "tcp_request_decisions", "hooked_relay_acl_decisions"):
        assert hasattr(request, name)
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hyobfs_request.h")).read(), flags=re.S)
    assert set(_lib._REQ_SIG) == set(re.findall(r"\b(hyobfs_[a-z0-9_]+)\s*\(", text))


# ------------------------------------------------------------------ the kernels on the CPU
@pytest.fixture(scope="module")
def request_main():
    """tests/emu/build/request_main: request.hip, request_host.cpp, addr.hip, addr_host.cpp and the driver, compiled
    for the host with AddressSanitizer and UndefinedBehaviorSanitizer (a program with its own main: nothing is
    preloaded).  Rebuilt when a source is newer."""
    if not os.path.exists(CLANG):
        pytest.skip("no host clang for the emulated build")
    csrc = os.path.join(ROOT, "hysteria_amd", "csrc")
    srcs = [os.path.join(EMU, "request_main.cpp")] + [os.path.join(csrc, f) for f in
                                                      ("request.hip", "request_host.cpp", "addr.hip", "addr_host.cpp")]
    deps = srcs + [os.path.join(EMU, "hip_emu.h")] + [os.path.join(csrc, f) for f in (
        "kernels.h", "request_rules.h", "addr_rules.h", "udpmsg_rules.h", "salamander_device.h")] + [
        os.path.join(ROOT, "include", f) for f in ("hyobfs_request.h", "hyobfs_addr.h", "hyobfs_sniff.h", "hyobfs_udpmsg.h")]
    os.makedirs(os.path.join(EMU, "build"), exist_ok=True)
    exe = os.path.join(EMU, "build", "request_main")
    with open(os.path.join(EMU, "build", ".request_main.lock"), "w") as lk:
        fcntl.flock(lk, fcntl.LOCK_EX)
        if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(d) for d in deps):
            tmp = exe + ".tmp"
            subprocess.run([CLANG, "-std=c++20", "-O1", "-g", "-DHYOBFS_EMULATE", "-I" + EMU, "-I" + csrc, "-x", "c++",
                            "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                            "-pthread", "-Wno-unused-command-line-argument", *srcs, "-o", tmp], check=True,
                           capture_output=True)
            os.replace(tmp, exe)
    return exe


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

    def rc(self, k=1):
        return [int(x) for x in self.arr(np.int32, k)]

    def guarded(self, dtype, n, mis=0):
        """An output array with its guards: the guards (and the bytes in front of a misaligned payload) must be intact."""
        lead, body, tail = self.arr(np.uint8, rc.GUARD_BYTES + mis), self.arr(dtype, n), self.arr(np.uint8, rc.GUARD_BYTES)
        assert bytes(lead) == bytes([rc.GUARD]) * len(lead) and bytes(tail) == bytes([rc.GUARD]) * len(tail)
        return body

    def done(self):
        return self.at == len(self.b)


def test_lattices_cover_the_batch_sizes_and_alignments():
    for cases in (rc.parse_cases(), rc.check_cases(), rc.rewrite_cases(), rc.response_cases()):
        assert set(rc.NS) <= {len(c["items"]) for c in cases}
    _, off, _ = rc.layout(rc.parse_items())
    assert {o % 16 for o in off} == set(range(16))
    assert {c["mis"] for c in rc.rewrite_cases()} == {c["mis"] for c in rc.response_cases()} == {0, 1, 2, 3}
    sts = {R.read_tcp_request(t)[0] for t in rc.parse_items()}
    assert sts == {R.OK, R.NEED_MORE, R.ADDR_LEN, R.PADDING_LEN}
    assert {rc.rewrite_one(x)[0] for x in rc.rewrite_items()} == {R.OK, R.HOST, -78}


def test_emulated_request_parse(request_main, tmp_path):
    cases = rc.parse_cases()
    res = _Reader(_run(request_main, tmp_path, b"".join(rc.blob_parse(c) for c in cases)))
    for c in cases:
        n = len(c["items"])
        assert res.rc() == [0]
        got = {k: res.guarded(dt, n) for k, dt in rc.PARSE_OUT}
        rc.check_parse(c["name"], c["items"], rc.layout(c["items"])[1], got)
    assert res.done()


def test_emulated_check(request_main, tmp_path):
    cases = rc.check_cases()
    res = _Reader(_run(request_main, tmp_path, b"".join(rc.blob_check(c) for c in cases)))
    passed = 0
    for c in cases:
        assert res.rc(2) == [0, 0]
        got = res.guarded(np.uint8, len(c["items"]))
        rc.verify_check(c, got)
        passed += int(got.sum())
    assert res.done() and passed > 200


def test_emulated_rewrite(request_main, tmp_path):
    cases = rc.rewrite_cases()
    res = _Reader(_run(request_main, tmp_path, b"".join(rc.blob_rewrite(c) for c in cases)))
    for c in cases:
        n = len(c["items"])
        assert res.rc() == [0]
        status, out_len, rew, row_off = (res.guarded(np.int32, n), res.guarded(np.uint32, n), res.guarded(np.uint8, n),
                                         res.guarded(np.uint64, n))
        rc.verify_rewrite(c, status, out_len, rew, row_off, res.guarded(np.uint8, n * c["stride"], c["mis"]))
    assert res.done()


def test_emulated_response_build(request_main, tmp_path):
    cases = rc.response_cases()
    res = _Reader(_run(request_main, tmp_path, b"".join(rc.blob_response(c) for c in cases)))
    for c in cases:
        n = len(c["items"])
        assert res.rc() == [0]
        status, out_len = res.guarded(np.int32, n), res.guarded(np.uint32, n)
        rc.verify_response(c, status, out_len, res.guarded(np.uint8, n * c["stride"], c["mis"]),
                           parse_back=request.tcp_response_record)
    assert res.done()
