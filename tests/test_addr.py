"""CPU tier of the request address (include/hyobfs_addr.h): the restatement
(tests/addr_ref.py) against Python's own address parsers and printers and against
the repository's other restatements of net.SplitHostPort, the scalar host ABI
against the restatement and the golden file (tests/golden/addr_vectors.json) over
the lattice of tests/addr_cases.py, and the device kernels through a stand-alone
AddressSanitizer build (tests/emu/addr_main.cpp + addr.hip against hip_emu.h, run
as a child process)."""
import ctypes
import fcntl
import ipaddress
import json
import os
import random
import re
import socket
import subprocess

import numpy as np
import pytest

import addr_cases as ac
import addr_ref as R
import http_ref
from hysteria_amd import _lib, addr, sniff

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
CLANG = "/opt/rocm/llvm/bin/clang++"
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "addr_vectors.json")))


# ------------------------------------------------------------------ the restatement against Python's parsers
def _mutations(n=20000, seed=0x1F):
    rng = random.Random(seed)
    valid = [s for s in ac.I_CORPUS if R.parse_ip(s) is not None]
    assert len(valid) >= 20
    alphabet = b"0123456789abcdefABCDEF:.%g[] x"
    out = []
    for _ in range(n):
        s = bytearray(rng.choice(valid))
        for _ in range(rng.randint(1, 3)):
            op, pos = rng.randrange(3), rng.randrange(len(s) + 1)
            if op == 0:
                s.insert(pos, rng.choice(alphabet))
            elif s and op == 1:
                del s[min(pos, len(s) - 1)]
            elif s:
                s[min(pos, len(s) - 1)] = rng.choice(alphabet)
        out.append(bytes(s))
    return out


@pytest.fixture(scope="module")
def ip_corpus():
    return ac.I_CORPUS + _mutations()


def _pton(s: bytes):
    try:
        t = s.decode("ascii")
    except UnicodeDecodeError:
        return None
    for fam in (socket.AF_INET, socket.AF_INET6):
        try:
            b = socket.inet_pton(fam, t)
            return R.V4_IN_V6 + b if fam == socket.AF_INET else b
        except (OSError, ValueError):
            pass
    return None


def test_restatement_agrees_with_inet_pton(ip_corpus):
    passed = 0
    for s in ip_corpus:
        assert R.parse_ip(s) == _pton(s), s
        passed += R.parse_ip(s) is not None
    assert 1000 < passed < len(ip_corpus) - 1000   # the mutations land on both sides


def test_restatement_agrees_with_ipaddress(ip_corpus):
    """ipaddress accepts a zone ("fe80::1%eth0"), ParseIP refuses it: the strings with a '%' are the only exclusion."""
    excluded = 0
    for s in ip_corpus:
        if b"%" in s:
            excluded += 1
            assert R.parse_ip(s) is None
            continue
        try:
            ip = ipaddress.ip_address(s.decode("ascii"))
            want = R.V4_IN_V6 + ip.packed if ip.version == 4 else ip.packed
        except ValueError:
            want = None
        assert R.parse_ip(s) == want, s
    assert excluded == sum(1 for s in ip_corpus if b"%" in s) and excluded > 100


def test_rule_i_corpus_verdicts():
    assert all(R.parse_ip(s) is not None for s in ac.I_PASS)
    assert all(R.parse_ip(s) is None for s in ac.I_REFUSE)
    assert R.parse_ip(b"::ffff:1.2.3.4") == R.parse_ip(b"1.2.3.4") == R.parse_ip(b"::ffff:102:304")
    assert R.parse_ip(b"1::2:1.2.3.4") == ipaddress.ip_address("1::2:102:304").packed


def _format_ips(n=20000, seed=0xF6):
    rng = random.Random(seed)
    ips = [ip for ip, fam, _ in ac.format_items() if fam == 16]
    for _ in range(n):
        ips.append(b"".join(rng.choice((b"\0\0", b"\0\0", b"\0" + bytes([rng.randrange(256)]), rng.randbytes(2)))
                            for _ in range(8)))
    return ips


def test_format_agrees_with_ipaddress():
    checked = dotted = 0
    for ip in _format_ips():
        if R.to4(ip) is None:
            assert R.ip_string(ip) == ipaddress.IPv6Address(ip).compressed.encode(), ip.hex()
            checked += 1
        else:
            assert R.ip_string(ip) == b"%d.%d.%d.%d" % tuple(ip[12:])
            dotted += 1
    assert checked > 20000 and dotted >= 1
    for ip, fam, port in ac.F_CORPUS:
        if fam == 4:
            assert R.format(ip, 4, port) == b"%d.%d.%d.%d:%d" % (*ip[:4], port)
    assert R.format(ac._ip("2001:db8:0:0:1:0:0:1"), 16, 1) == b"[2001:db8::1:0:0:1]:1"
    assert R.format(ac._ip("2001:0:0:1:0:0:0:1"), 16, 1) == b"[2001:0:0:1::1]:1"
    assert R.format(ac._ip("1:0:2:3:4:5:6:7"), 16, 1) == b"[1:0:2:3:4:5:6:7]:1"
    assert R.format(ac._ip("::ffff:1.2.3.4"), 16, 1) == b"1.2.3.4:1" and R.format(ac._ip("::1.2.3.4"), 16, 1) == b"[::102:304]:1"
    assert len(R.format(b"\xff" * 16, 16, 65535)) == R.FORMAT_MAX == addr.FORMAT_MAX
    assert R.format(bytes(16), 6, 1) == R.FAMILY


def test_split_restatements_agree():
    """addr_ref.split, sniff.split_host_port and http_ref.split_host over the rule-H corpus and the lattice."""
    messages = {R.MISSING_PORT: "missing port", R.TOO_MANY_COLONS: "too many colons", R.MISSING_BRACKET: "missing ']'",
                R.UNEXPECTED_LBRACKET: "unexpected '['", R.UNEXPECTED_RBRACKET: "unexpected ']'"}
    seen = set()
    for t in ac.H_CORPUS + [x for x in ac.all_items() if len(x) <= R.MAX_ADDR]:
        st, ho, hl, po, pl = R.split(t)
        seen.add(st)
        text = t.decode("latin-1")
        h = http_ref.split_host(t)
        if st == R.OK:
            assert sniff.split_host_port(text) == (text[ho:ho + hl], text[po:po + pl])
            assert h == (ho, t[ho:ho + hl])
        else:
            with pytest.raises(ValueError, match=re.escape(messages[st])):
                sniff.split_host_port(text)
            assert h is None
    assert seen == {R.OK, *messages}


def test_rule_h_order():
    want = {b"": R.MISSING_PORT, b":": R.OK, b":80": R.OK, b"host:": R.OK, b"a:b:80": R.TOO_MANY_COLONS, b"[::1]:80": R.OK,
            b"[::1]": R.MISSING_PORT, b"[::1]80": R.MISSING_PORT, b"[::1]::80": R.TOO_MANY_COLONS,
            b"[::1": R.MISSING_BRACKET, b"[a]b:80": R.MISSING_PORT, b"a[b:80": R.UNEXPECTED_LBRACKET,
            b"[a[b]:80": R.UNEXPECTED_LBRACKET, b"a]b:80": R.UNEXPECTED_RBRACKET, b"[a]:8]0": R.UNEXPECTED_RBRACKET,
            b"[]:80": R.OK, b"@SpeedTest": R.MISSING_PORT, b"a:b[:8]0": R.TOO_MANY_COLONS,
            b"a[b]:80": R.UNEXPECTED_LBRACKET, b"[a[b]]:80": R.MISSING_PORT, b"[a]:[8]0": R.UNEXPECTED_LBRACKET}
    for t, st in want.items():
        assert t in ac.H_CORPUS and R.split(t)[0] == st == addr.split_record(t)[0], t
    assert R.split(b"[]:80") == (R.OK, 1, 0, 3, 2) and R.split(b"host:") == (R.OK, 0, 4, 5, 0)


# ------------------------------------------------------------------ the scalar ABI
def test_golden_file_is_the_restatement():
    assert GOLDEN == json.loads(json.dumps(ac.golden()))


def test_scalar_abi_against_golden():
    for v in GOLDEN["split"]:
        t = bytes.fromhex(v["hex"])
        assert addr.split_record(t) == (v["status"], *v["host"], *v["port"]), t
    for v in GOLDEN["port"]:
        t = bytes.fromhex(v["hex"])
        if v["value"] is None:
            with pytest.raises(addr.AddrError) as e:
                addr.parse_port(t)
            assert e.value.status == addr.ERR_PORT
        else:
            assert addr.parse_port(t) == v["value"]
    for v in GOLDEN["ip"]:
        got = addr.parse_ip(bytes.fromhex(v["hex"]))
        assert got == (None if v["ip16"] is None else bytes.fromhex(v["ip16"])), v["text"]
    for v in GOLDEN["parse"]:
        assert addr.parse_record(bytes.fromhex(v["hex"])) == (v["status"], *v["name"], bytes.fromhex(v["ipv4"]),
                                                              bytes.fromhex(v["ipv6"]), v["ip_flags"], v["port"]), v["text"]
    for v in GOLDEN["format"]:
        ip = bytes.fromhex(v["ip16"])
        n = ctypes.c_uint8 * 64
        out, src = n(), (ctypes.c_uint8 * 16).from_buffer_copy(ip)
        got = addr._adlib().hyobfs_addr_format(ctypes.addressof(src), v["family"], v["port"], ctypes.addressof(out), 64)
        if isinstance(v["text"], int):
            assert got == v["text"] == addr.ERR_FAMILY
        else:
            assert bytes(out[:got]) == v["text"].encode("latin-1")
            assert addr._adlib().hyobfs_addr_format(ctypes.addressof(src), v["family"], v["port"], ctypes.addressof(out),
                                                    got - 1) == -1


def test_scalar_abi_against_restatement(ip_corpus):
    seen = set()
    for t in ac.all_items():
        want = R.parse(t)
        assert addr.parse_record(t) == want, t[:80]
        assert addr.split_record(t) == R.split(t), t[:80]
        seen.add(want[0])
    assert seen == {R.OK, R.MISSING_PORT, R.TOO_MANY_COLONS, R.MISSING_BRACKET, R.UNEXPECTED_LBRACKET,
                    R.UNEXPECTED_RBRACKET, R.PORT, R.TOO_LONG}
    for s in ip_corpus:
        assert addr.parse_ip(s) == R.parse_ip(s), s
    for p in ac.P_CORPUS:
        v = R.parse_port(p)
        if v is None:
            with pytest.raises(addr.AddrError):
                addr.parse_port(p)
        else:
            assert addr.parse_port(p) == v
    for ip, fam, port in ac.format_items():
        want = R.format(ip, fam, port)
        out, src = (ctypes.c_uint8 * 47)(), (ctypes.c_uint8 * 16).from_buffer_copy(ip)
        got = addr._adlib().hyobfs_addr_format(ctypes.addressof(src), fam, port, ctypes.addressof(out), 47)
        assert (got if got < 0 else bytes(out[:got])) == want, (ip.hex(), fam, port)


def test_python_layer():
    assert addr.split_host_port("[2001:db8::1]:443") == (b"2001:db8::1", b"443")
    assert addr.parse("1.2.3.4:53") == (b"1.2.3.4", bytes([1, 2, 3, 4]), None, 53)
    assert addr.parse(b"[::1.2.3.4]:0080") == (b"::1.2.3.4", None, bytes(12) + bytes([1, 2, 3, 4]), 80)
    assert addr.parse("example.com:443") == (b"example.com", None, None, 443)
    with pytest.raises(addr.AddrError) as e:
        addr.parse("@SpeedTest")
    assert e.value.status == addr.ERR_MISSING_PORT
    assert addr.format(bytes([10, 0, 0, 1]), 53) == b"10.0.0.1:53" and addr.format(bytes(15) + b"\1", 9) == b"[::1]:9"
    assert addr.format(bytes(16), 0, cap=5) == -1
    with pytest.raises(addr.AddrError):
        addr.format(bytes(5), 1)
    for st, name in addr.STATUS_NAMES.items():
        if st:
            assert _lib.status_string(st) == addr.ERRORS[st] and name in ("NO_ADDR", "MISSING_PORT", "TOO_MANY_COLONS",
                                                                         "MISSING_BRACKET", "UNEXPECTED_LBRACKET",
                                                                         "UNEXPECTED_RBRACKET", "PORT", "TOO_LONG", "FAMILY")


# ------------------------------------------------------------------ ABI surface
_CTYPES = {"size_t": ctypes.c_size_t, "uint64_t": ctypes.c_uint64, "uint32_t": ctypes.c_uint32, "uint16_t": ctypes.c_uint16,
           "int": ctypes.c_int}


def test_header_and_bindings_agree(tmp_path):
    consts = ["HYOBFS_ADDR_ERR_NO_ADDR", "HYOBFS_ADDR_ERR_MISSING_PORT", "HYOBFS_ADDR_ERR_TOO_MANY_COLONS",
              "HYOBFS_ADDR_ERR_MISSING_BRACKET", "HYOBFS_ADDR_ERR_UNEXPECTED_LBRACKET",
              "HYOBFS_ADDR_ERR_UNEXPECTED_RBRACKET", "HYOBFS_ADDR_ERR_PORT", "HYOBFS_ADDR_ERR_TOO_LONG",
              "HYOBFS_ADDR_ERR_FAMILY", "HYOBFS_ADDR_LITERAL_MAX", "HYOBFS_ADDR_FORMAT_MAX", "HYOBFS_ADDR_HAS_IPV4",
              "HYOBFS_ADDR_HAS_IPV6", "HYOBFS_UDP_MAX_ADDR", "HYOBFS_UDP_ERR_PLAN", "HYOBFS_ABI_VERSION"]
    want = [*range(-77, -86, -1), 45, 47, 1, 2, 2048, -76, 4]
    assert want[:13] == [addr.ERR_NO_ADDR, addr.ERR_MISSING_PORT, addr.ERR_TOO_MANY_COLONS, addr.ERR_MISSING_BRACKET,
                         addr.ERR_UNEXPECTED_LBRACKET, addr.ERR_UNEXPECTED_RBRACKET, addr.ERR_PORT, addr.ERR_TOO_LONG,
                         addr.ERR_FAMILY, addr.LITERAL_MAX, addr.FORMAT_MAX, addr.HAS_IPV4, addr.HAS_IPV6]
    assert want[:11] == [R.NO_ADDR, R.MISSING_PORT, R.TOO_MANY_COLONS, R.MISSING_BRACKET, R.UNEXPECTED_LBRACKET,
                         R.UNEXPECTED_RBRACKET, R.PORT, R.TOO_LONG, R.FAMILY, R.LITERAL_MAX, R.FORMAT_MAX]
    assert (addr.MAX_ADDR, R.MAX_ADDR, ac.META_DTYPE) == (2048, 2048, __import__("hysteria_amd").udpmsg.META_DTYPE)
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include "hyobfs_addr.h"\nint main(void){\n'
                   + "\n".join(f'printf("%d\\n", (int){c});' for c in consts) + "\nreturn 0;}\n")
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    assert [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()] == want
    # every prototype of the header: the same number of arguments, pointers where the header has pointers and
    # the scalar of the header's width elsewhere
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hyobfs_addr.h")).read(), flags=re.S)
    protos = re.findall(r"\bint\s+(hyobfs_addr_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text)
    assert sorted(n for n, _ in protos) == sorted(_lib._ADDR_SIG) and len(protos) == 8
    for name, params in protos:
        res, args = _lib._ADDR_SIG[name]
        assert res is ctypes.c_int
        params = [p.strip() for p in params.split(",")]
        assert len(params) == len(args), name
        for p, a in zip(params, args):
            if "*" in p:
                assert a is ctypes.c_void_p or issubclass(a, ctypes._Pointer), (name, p)
            else:
                assert a is _CTYPES[p.replace("const ", "").split()[0]], (name, p)
    lib = addr._adlib()
    assert lib.hyobfs_abi_version() == 4
    assert all(getattr(lib, n).argtypes is not None for n in _lib._ADDR_SIG)


def test_empty_batches_and_null_pointers():
    lib, N = addr._adlib(), None
    assert lib.hyobfs_addr_parse_batch(N, N, N, 0, N, N, N, N, N, N, N, N) == 0
    assert lib.hyobfs_addr_parse_udp_batch(N, N, N, 0, N, N, N, N, N, N, N, N) == 0
    assert lib.hyobfs_addr_format_batch(N, N, N, 0, N, 0, 0, N, N, N, N) == 0
    assert lib.hyobfs_addr_parse_batch(N, N, N, 1, N, N, N, N, N, N, N, N) == _lib.HYOBFS_ERR_INVALID
    assert lib.hyobfs_addr_parse_udp_batch(N, N, N, 1, N, N, N, N, N, N, N, N) == _lib.HYOBFS_ERR_INVALID
    assert lib.hyobfs_addr_format_batch(N, N, N, 1, N, 47, 0, N, N, N, N) == _lib.HYOBFS_ERR_INVALID
    u32, u16, u8 = ctypes.c_uint32(), ctypes.c_uint16(), ctypes.c_uint8()
    assert lib.hyobfs_addr_split(N, 0, N, N, N, N) == _lib.HYOBFS_ERR_INVALID
    assert lib.hyobfs_addr_split(N, 0, *[ctypes.byref(u32)] * 4) == addr.ERR_MISSING_PORT
    assert lib.hyobfs_addr_parse_port(N, 0, N) == _lib.HYOBFS_ERR_INVALID
    assert lib.hyobfs_addr_parse_port(N, 0, ctypes.byref(u16)) == addr.ERR_PORT
    assert lib.hyobfs_addr_parse_ip(N, 0, N) == _lib.HYOBFS_ERR_INVALID
    assert lib.hyobfs_addr_parse(N, 0, N, N, N, N, ctypes.byref(u8), N) == _lib.HYOBFS_ERR_INVALID
    assert lib.hyobfs_addr_format(N, 4, 1, N, 0) == _lib.HYOBFS_ERR_INVALID


def test_package_exports():
    import hysteria_amd
    for name in ("addr", "AddrError", "relay_acl_decisions"):
        assert name in hysteria_amd.__all__ and hasattr(hysteria_amd, name)
    for name in ("split_host_port", "parse_port", "parse_ip", "parse", "format", "parse_batch", "parse_udp_batch",
                 "format_batch", "relay_acl_decisions", "STATUS_NAMES"):
        assert hasattr(addr, name)
    assert sniff.split_host_port("a:1") == ("a", "1")   # stays


# ------------------------------------------------------------------ the kernels on the CPU
@pytest.fixture(scope="module")
def addr_main():
    """tests/emu/build/addr_main: addr.hip, udpmsg.hip and the driver, compiled for the host with
    AddressSanitizer (a program with its own main: nothing is preloaded).  Rebuilt when a source is newer."""
    if not os.path.exists(CLANG):
        pytest.skip("no host clang for the emulated build")
    csrc = os.path.join(ROOT, "hysteria_amd", "csrc")
    srcs = [os.path.join(EMU, "addr_main.cpp"), os.path.join(csrc, "addr.hip"), os.path.join(csrc, "udpmsg.hip")]
    deps = srcs + [os.path.join(EMU, "hip_emu.h"), os.path.join(csrc, "kernels.h"), os.path.join(csrc, "addr_rules.h"),
                   os.path.join(csrc, "udpmsg_rules.h"), os.path.join(csrc, "salamander_device.h"),
                   os.path.join(ROOT, "include", "hyobfs_addr.h"), os.path.join(ROOT, "include", "hyobfs_udpmsg.h")]
    os.makedirs(os.path.join(EMU, "build"), exist_ok=True)
    exe = os.path.join(EMU, "build", "addr_main")
    with open(os.path.join(EMU, "build", ".addr_main.lock"), "w") as lk:
        fcntl.flock(lk, fcntl.LOCK_EX)
        if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(d) for d in deps):
            tmp = exe + ".tmp"
            subprocess.run([CLANG, "-std=c++20", "-O1", "-g", "-DHYOBFS_EMULATE", "-I" + EMU, "-I" + csrc, "-x", "c++",
                            "-fsanitize=address", "-fno-omit-frame-pointer", "-pthread",
                            "-Wno-unused-command-line-argument", *srcs, "-o", tmp], check=True, capture_output=True)
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

    def guarded(self, dtype, n, mis=0):
        """An output array with its guards: the guards (and the bytes in front of a misaligned payload) must be intact."""
        lead, body, tail = self.arr(np.uint8, ac.GUARD_BYTES + mis), self.arr(dtype, n), self.arr(np.uint8, ac.GUARD_BYTES)
        assert bytes(lead) == bytes([ac.GUARD]) * len(lead) and bytes(tail) == bytes([ac.GUARD]) * len(tail)
        return body

    def parse_outputs(self, n):
        mis = n % 4
        return {name: self.guarded(dt, n * w, mis if name in ("ipv4", "ipv6") else 0) for name, dt, w in ac.PARSE_OUT}

    def done(self):
        return self.at == len(self.b)


def test_emulated_parse(addr_main, tmp_path):
    cases = ac.parse_cases()
    assert sorted(len(c["items"]) for c in cases)[:8] == sorted(ac.NS) and {c["mode"] for c in cases} == {"poison", "packed"}
    assert {layout_off % 4 for layout_off in ac.layout(cases[0])[1]} == {0, 1, 2, 3}
    res = _Reader(_run(addr_main, tmp_path, b"".join(ac.blob_parse(c) for c in cases)))
    for c in cases:
        assert int(res.arr(np.int32, 1)[0]) == 0
        ac.check_parse(c["name"], c["items"], ac.layout(c)[1], res.parse_outputs(len(c["items"])))
    assert res.done()


def test_emulated_parse_udp(addr_main, tmp_path):
    ds, addrs, at = ac.udp_datagrams()
    assert sum(a is None for a in addrs) == 6
    res = _Reader(_run(addr_main, tmp_path, ac.blob_parse_udp(ds)))
    assert list(res.arr(np.int32, 2)) == [0, 0]
    got = res.parse_outputs(len(ds))
    assert res.done()
    _, offs, _ = ac.layout(dict(items=ds, mode="poison"))
    check_parse_udp(addrs, [o + a for o, a in zip(offs, at)], got)


def check_parse_udp(addrs, at, got) -> None:
    """Shared with the GPU tier: ``at`` is where each address starts in the buffer; a datagram that does not
    parse is NO_ADDR with zeros."""
    items = [b"" if a is None else a for a in addrs]
    exp = ac.expected_parse(items, at)
    for i, a in enumerate(addrs):
        if a is None:
            exp[i] = (R.NO_ADDR, 0, 0, bytes(4), bytes(16), 0, 0)
    for i, e in enumerate(exp):
        g = (int(got["status"][i]), int(got["name_off"][i]), int(got["name_len"][i]), bytes(got["ipv4"][4 * i:4 * i + 4]),
             bytes(got["ipv6"][16 * i:16 * i + 16]), int(got["ip_flags"][i]), int(got["port"][i]))
        assert g == e, (i, items[i][:80], g, e)


def _format_results(res, case):
    n = len(case["items"])
    assert int(res.arr(np.int32, 1)[0]) == 0
    status, out_len = res.guarded(np.int32, n), res.guarded(np.uint32, n)
    meta = res.guarded(ac.META_DTYPE, n) if case["meta"] else None
    return status, out_len, meta, res.guarded(np.uint8, n * case["stride"], case["mis"])


def test_emulated_format(addr_main, tmp_path):
    cases = ac.format_cases()
    res = _Reader(_run(addr_main, tmp_path, b"".join(ac.blob_format(c) for c in cases)))
    for c in cases:
        ac.check_format(c, *_format_results(res, c))
    assert res.done()


def test_emulated_parse_of_format_round_trip(addr_main, tmp_path):
    """parse(format(ip, port)) gives back the port and the address under rule T."""
    case = dict(name="round_trip", items=[x for x in ac.format_items() if x[1] in (4, 16)], stride=47, mis=0, meta=False)
    res = _Reader(_run(addr_main, tmp_path, ac.blob_format(case)))
    _, out_len, _, out = _format_results(res, case)
    texts = [bytes(out[47 * i:47 * i + int(n)]) for i, n in enumerate(out_len)]
    pcase = dict(name="round_trip_parse", items=texts, mode="poison")
    res = _Reader(_run(addr_main, tmp_path, ac.blob_parse(pcase)))
    assert int(res.arr(np.int32, 1)[0]) == 0
    got = res.parse_outputs(len(texts))
    for i, (ip, fam, port) in enumerate(case["items"]):
        ip16 = R.V4_IN_V6 + ip[:4] if fam == 4 else ip
        assert int(got["status"][i]) == R.OK and int(got["port"][i]) == port
        if R.to4(ip16) is not None:
            assert int(got["ip_flags"][i]) == R.HAS_IPV4 and bytes(got["ipv4"][4 * i:4 * i + 4]) == ip16[12:]
        else:
            assert int(got["ip_flags"][i]) == R.HAS_IPV6 and bytes(got["ipv6"][16 * i:16 * i + 16]) == ip16
